"""Subprocess of tests/test_gpu_msm_windows.py: the c = 5 bucket MSM's window sums
(k_msm_windows_w4, grandine_amd/csrc/k_msm_w4.hip) at the smallest shapes at which they can go
wrong.  A submission takes the MSM only when EVERY segment holds at least GBLS_MSM_MIN sets, so the
plan runs in three children, each a fresh engine:

    --set main    GBLS_MSM_MIN=1: every case whose segments are all nonempty
    --set empty   GBLS_MSM_MIN=0: the cases with an empty segment (0 >= 0 holds)
    --set engine  GBLS_MSM_MIN=1, GBLS_MSM_R28=0: the engine-form partials (w4::load) on the grid

Every case is a gbls_multi_verify_segments call whose per-segment verdicts are compared with the C
oracle's ref_multi_verify of the same segment, once as planned and once with one message of every
nonempty segment corrupted (the twin, which must fail).  Every call also reports how often the
stage timers saw the MSM stage and the per-set signature sum ("stages": [k_msm, k_g2sum] calls),
so that the test can assert the path and not only the verdict.  Keys and signatures come from the
C oracle, so the plan is the same on a machine without a GPU:

    python3 tests/gpu_msm_windows.py --set main --oracle    # the oracle's verdicts, no engine

prints one JSON line."""
import ctypes
import hashlib
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SET = sys.argv[sys.argv.index("--set") + 1] if "--set" in sys.argv else "main"
os.environ["GBLS_MSM_MIN"] = "0" if SET == "empty" else "1"
if SET == "engine":
    os.environ["GBLS_MSM_R28"] = "0"

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
M64 = (1 << 64) - 1
POOL = 358


def u64(v):
    return (ctypes.c_uint64 * len(v))(*v)


def u32(v):
    return (ctypes.c_uint32 * len(v))(*v)


class Oracle:
    def __init__(self):
        C = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libbls_ref.so"))
        C.ref_multi_verify.argtypes = [ctypes.c_char_p] * 3 + [ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
                                                               ctypes.c_int]
        C.ref_sk_to_pk.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        C.ref_sign.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
        self.C = C
        self.memo = {}

    def keypair(self, sk, msg):
        pk, sig = ctypes.create_string_buffer(96), ctypes.create_string_buffer(192)
        skb = sk.to_bytes(32, "big")
        self.C.ref_sk_to_pk(skb, pk)
        self.C.ref_sign(skb, msg, 32, sig)
        return pk.raw, sig.raw

    @staticmethod
    def key(sets):
        return hashlib.sha256(b"".join(m + s + p + r.to_bytes(8, "little") for m, s, p, r in sets)).digest()

    def verdict(self, sets):
        """ref_multi_verify of one segment (a list of sets): True = valid.  An empty one is invalid."""
        key = self.key(sets)
        if key not in self.memo:
            m = b"".join(x[0] for x in sets)
            s = b"".join(x[1] for x in sets)
            p = b"".join(x[2] for x in sets)
            nt = 4 if len(sets) > 64 else 1
            self.memo[key] = bool(self.C.ref_multi_verify(m, s, p, u64([x[3] for x in sets]), len(sets), nt))
        return self.memo[key]

    def warm(self, segments):
        """The verdicts of many segments side by side (the library call releases the interpreter lock)."""
        todo = {self.key(s): s for s in segments}
        with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as ex:
            list(ex.map(self.verdict, todo.values()))


def rand64(tag, i):
    return int.from_bytes(hashlib.sha256(b"msmw/r/%s/%d" % (tag, i)).digest()[:8], "little") or 1


def plan(O):
    """[(name, sets, offsets, forced)]: sets = [(msg, sig, pk, r)], forced = {segment: status} where
    the engine's flag and not the oracle decides (a zero scalar)."""
    sk = [int.from_bytes(hashlib.sha256(b"msmw/sk/%d" % i).digest(), "big") % R_ORDER or 1 for i in range(POOL)]
    msg = [hashlib.sha256(b"msmw/m/%d" % i).digest() for i in range(POOL)]
    made = {}

    class Pool:  # a set's key and signature are made when a case first uses it
        def __getitem__(self, i):
            if i not in made:
                pk, sig = O.keypair(sk[i], msg[i])
                made[i] = (msg[i], sig, pk)
            return made[i]

    pool = Pool()

    def sets(idx, rs):
        return [pool[i] + (r,) for i, r in zip(idx, rs)]

    # one bucket of one window per segment: r = (b + 1) 2^(5 w) (16 * 2^60 does not fit 64 bits)
    grid = [(b + 1) << (5 * w) for w in range(13) for b in range(16) if (b + 1) << (5 * w) <= M64]
    assert len(grid) == 13 * 16 - 1
    cases = [("grid", sets(range(len(grid)), grid), list(range(len(grid) + 1)), {})]
    if SET == "engine":
        return cases
    # offsets with an empty segment (the MSM takes them only with GBLS_MSM_MIN=0), and without
    seg_off = [0, 1, 1, 18, 58, 358] if SET == "empty" else [0, 1, 18, 58, 358]
    rs = [rand64(b"segs", i) for i in range(POOL)]
    inf = sets(range(POOL), rs)
    inf[5] = (inf[5][0], bytes(192), inf[5][2], inf[5][3])
    zero = sets(range(POOL), rs)
    zero[20] = zero[20][:3] + (0,)
    zseg = seg_off.index(58) - 1  # the segment [18, 58)
    tail = [("infinite signature", inf, seg_off, {}), ("zero scalar", zero, seg_off, {zseg: 5})]
    if SET == "empty":  # a one-set segment, an empty one, mixed sizes
        return [("segments", sets(range(POOL), rs), seg_off, {})] + tail
    # signed digits and carries: 17 * 2^(5 w) (digit -15, carry), 2^64 - 1 (digits -1, top digit 16), 2^63, 1
    sd = [17 << (5 * w) for w in range(12)] + [M64, 1 << 63, 1]
    cases.append(("signed", sets(range(len(sd)), sd), list(range(len(sd) + 1)), {}))
    # a full window: every bucket of window 0; buckets 0..14 of window 12
    full = [b + 1 for b in range(16)] + [(b + 1) << 60 for b in range(15)]
    cases.append(("full", sets(range(31), full), [0, 16, 31], {}))
    # addition special cases inside the fold
    neg_pk, neg_sig = O.keypair(R_ORDER - sk[0], msg[0])  # (-pk_0, m_0, -sig_0): a valid set
    r = rand64(b"special", 0)
    twice = [pool[1] + (r,), pool[1] + (r,)]                      # equal points
    cancel = [pool[0] + (r,), (msg[0], neg_sig, neg_pk, r)]       # one bucket sum is infinity
    third = [pool[2] + (rand64(b"special", 1),)]
    cases.append(("special", twice + cancel + third + cancel, [0, 2, 5, 7], {}))
    # several runs per bucket: 40 sets in bucket 0 of window 0 (K = 4: 10 chunks, two runs); 300 random scalars
    runs = [1] * 40 + [rand64(b"runs", i) for i in range(300)]
    cases.append(("runs", sets(range(340), runs), [0, 40, 340], {}))
    cases += tail
    # more than 1024 windows: the window sums go affine through launch_lines
    wide = [rand64(b"wide", i) for i in range(80)]
    cases.append(("80 segments", sets(range(80), wide), list(range(81)), {}))
    return cases


def twin(sets, off):
    """One message of every nonempty segment corrupted (the last set's)."""
    out = list(sets)
    for s in range(len(off) - 1):
        if off[s + 1] > off[s]:
            i = off[s + 1] - 1
            m = bytearray(out[i][0])
            m[7] ^= 0x10
            out[i] = (bytes(m),) + out[i][1:]
    return out


def expected(O, sets, off, forced):
    return [forced[s] if s in forced else (0 if O.verdict(sets[off[s]:off[s + 1]]) else 5)
            for s in range(len(off) - 1)]


def stage_calls(L):
    """[k_msm, k_g2sum] stage-timer calls since the last reset."""
    calls = (ctypes.c_uint32 * 64)()
    ns = L.gbls_profile_read(None, calls, 64)
    names = [L.gbls_stage_name(i).decode() for i in range(ns)]
    L.gbls_profile_reset()
    return [calls[names.index("k_msm")], calls[names.index("k_g2sum")]]


def engine_verdicts(G, L, sets, off):
    n, nseg = len(sets), len(off) - 1
    m = b"".join(x[0] for x in sets)
    s = b"".join(x[1] for x in sets)
    p = b"".join(x[2] for x in sets)
    vs = G.i32_array(nseg)
    G.check(L.gbls_multi_verify_segments(m, s, p, u64([x[3] for x in sets]), n, u32(off), nseg, vs), "segments")
    return [vs[i] for i in range(nseg)]


def engine_partials_verdicts(G, L, sets, off):
    """The other convention for an empty segment (no error, the identity partial): Miller partials
    through gbls_multi_verify_partials_device, then one final exponentiation per segment."""
    import torch

    dev = torch.device("cuda", 0)
    n, nseg = len(sets), len(off) - 1
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    m, s, p = (up(b"".join(x[k] for x in sets)) for k in range(3))
    r = torch.tensor([x[3] - (1 << 64) if x[3] >= 1 << 63 else x[3] for x in sets], dtype=torch.int64, device=dev)
    parts = torch.zeros(nseg * 576, dtype=torch.uint8, device=dev)
    errs = torch.full((nseg,), -1, dtype=torch.int32, device=dev)
    v = torch.full((nseg,), -1, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    G.check(L.gbls_multi_verify_partials_device(m.data_ptr(), s.data_ptr(), p.data_ptr(), r.data_ptr(), n, u32(off),
                                                nseg, parts.data_ptr(), errs.data_ptr(), st), "partials")
    G.check(L.gbls_final_verify_partials_device(parts.data_ptr(), errs.data_ptr(), 1, nseg, v.data_ptr(), st), "final")
    torch.cuda.synchronize()
    return [int(x) for x in v.cpu()]


def main():
    oracle_only = "--oracle" in sys.argv[1:]
    O = Oracle()
    cases = plan(O)
    G = L = None
    if not oracle_only:
        from grandine_amd import _lib as G
        G.enable_tuning()  # the engine reads the knob set above
        L = G.lib()
        L.gbls_profile(1)
        L.gbls_profile_reset()
    runs = [(n, ss, off, f) for n, sets, off, f in cases for ss in (sets, twin(sets, off))]
    O.warm([ss[off[s]:off[s + 1]] for _, ss, off, f in runs for s in range(len(off) - 1) if s not in f])
    res = {"set": SET, "cases": []}
    for name, sets, off, forced in cases:
        for label, ss in ((name, sets), (name + " / twin", twin(sets, off))):
            row = {"name": label, "ref": expected(O, ss, off, forced)}
            if L:
                row["gpu"] = engine_verdicts(G, L, ss, off)
                row["stages"] = stage_calls(L)
            res["cases"].append(row)
            if name == "segments":  # an empty segment is the identity partial, not an error
                want = [0 if off[s + 1] == off[s] else v for s, v in enumerate(row["ref"])]
                row = {"name": label + " / partials", "ref": want}
                if L:
                    row["gpu"] = engine_partials_verdicts(G, L, ss, off)
                    row["stages"] = stage_calls(L)
                res["cases"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
