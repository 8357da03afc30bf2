"""Subprocess of tests/test_gpu_each.py, with an engine of its own.

replicas: two engines on the one GPU (gbls_init flags = 2).  4200 independent checks over
two-committee spans through gbls_verify_each_spans (whole segments per engine, each shard in the
grouped regime, each writing its slice of both status arrays): a bad signature at 3000, malformed
strings at 100 and 4000.  Then gbls_verify_items_spans over two 1100-set items, one per engine, the
second holding a bad signature.

threads: eight threads, started together behind a barrier, each making 20 items calls of its own
9-set, 3-item batch; thread 3's second item holds a swapped signature, thread 5's set 7 a malformed
string, thread 6's set 0 a signature that does not decode.  Counts the calls whose verdicts and
statuses are exactly the caller's own.  (Whether calls were merged is the business of
tests/test_each_sched.py.)

Prints one JSON line."""
import ctypes
import json
import os
import random
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODE = sys.argv[1]

from grandine_amd import _lib as G  # noqa: E402
from grandine_amd import factory as F  # noqa: E402

NREG = 600
KINDS = ["full", "one-clear", "one-set", "half", "most", "few"]
COMS = [[(9 * c + j) % NREG for j in range(3 + c % 7)] for c in range(16)]   # 3..9 members


def u64(v):
    return (ctypes.c_uint64 * len(v))(*v)


def flat(lists):
    off = [0]
    for v in lists:
        off.append(off[-1] + len(v))
    return [i for v in lists for i in v], off


def encode(bits, bitlist):
    m = len(bits)
    out = bytearray(m // 8 + 1 if bitlist else (m + 7) // 8)
    for j, b in enumerate(bits):
        out[j >> 3] |= b << (j & 7)
    if bitlist:
        out[m >> 3] |= 1 << (m & 7)
    return bytes(out)


def mask_bytes(named):
    out = bytearray(8)
    for c in named:
        out[c >> 3] |= 1 << (c & 7)
    return bytes(out)


def committee_bits(m, kind, rng):
    if kind == "full":
        return [1] * m
    if kind == "one-clear":
        return [int(j != m // 3 or m == 1) for j in range(m)]
    if kind == "one-set":
        return [int(j == (2 * m) // 3) for j in range(m)]
    if kind == "half":
        chosen = set(rng.sample(range(m), max(1, m // 2)))
        return [int(j in chosen) for j in range(m)]
    bits = [int(rng.random() < (0.9 if kind == "most" else 0.25)) for _ in range(m)]
    bits[rng.randrange(m)] = 1
    return bits


def compress(L, sigs):
    n = len(sigs) // 192
    out = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, out), "compress")
    return out.raw


def decode_statuses(L, comp):
    n = len(comp) // 96
    out, st = ctypes.create_string_buffer(192 * n), G.i32_array(n)
    G.check(L.gbls_g2_decompress(comp, n, out, st), "decompress")
    return [st[i] for i in range(n)]


def setup(L, seed):
    sks, comp = F.registry(NREG, seed=seed)
    assert not F.load_registry(comp).any()
    idx, off = flat(COMS)
    st = G.i32_array(len(COMS))
    rc = L.gbls_committees_set_members(0, G.u32_array(idx), G.u32_array(off), len(COMS), st)
    assert rc == 0 and not any(st[c] for c in range(len(COMS))), (rc, L.gbls_last_error())
    return sks


def span_sets(sks, n, rng, tag, shift=0):
    """n two-committee spans: (bases, masks, fields, signing keys, messages)."""
    bases, masks, fields, sums = [], [], [], []
    for i in range(n):
        base, second = (i + shift) % 13, 1 + i % 3
        per = [committee_bits(len(COMS[base + c]), KINDS[(i + c + shift) % len(KINDS)], rng) for c in (0, second)]
        bases.append(base)
        masks.append(mask_bytes([0, second]))
        fields.append(encode(per[0] + per[1], (i + shift) % 2 == 0))
        sums.append(sum(sks[v] for c, b in zip((0, second), per) for v, x in zip(COMS[base + c], b) if x) % F.R_ORDER)
    return bases, masks, fields, sums, F.messages(n, tag)


def call_args(msgs, sigs, bases, masks, fields):
    _, boff = flat(fields)
    return (msgs, sigs, G.u32_array(bases), G.buf(b"".join(masks)), G.buf(b"".join(fields)), G.u32_array(boff), None, None)


def replicas():
    L = G.lib(0, 2)
    res = {"engines": L.gbls_device_count()}
    sks = setup(L, b"each/child")
    rng = random.Random("each/replicas")
    n = 4200
    bases, masks, fields, sums, msgs = span_sets(sks, n, rng, b"each/big")
    sig = bytearray(compress(L, F.sign(sums, msgs)))
    sig[96 * 3000:96 * 3001] = sig[96 * 10:96 * 11]   # a valid signature of another set, in the second shard
    clean = list(fields)
    for i in (100, 4000):                             # one malformed string per shard: its last byte dropped
        fields[i] = fields[i][:-1]
    st, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
    rc = L.gbls_verify_each_spans(*call_args(msgs, bytes(sig), bases, masks, fields), n, st, kst, v)
    res["each"] = [rc, L.gbls_last_error()]
    res["each_failing"] = [i for i in range(n) if v[i] != G.SUCCESS]
    res["each_verdicts_other"] = sorted(set(v[i] for i in range(n)) - {G.SUCCESS, G.VERIFY_FAIL})
    res["each_key_status"] = [[i, kst[i]] for i in range(n) if kst[i]]
    res["each_sig_status"] = [[i, st[i]] for i in range(n) if st[i]]
    # two items of 1100 sets, whole items per engine
    m = 2200
    sig2 = bytearray(compress(L, F.sign(sums[:m], msgs[:32 * m])))
    sig2[96 * 1500:96 * 1501] = sig2[96 * 20:96 * 21]
    st, kst, v2 = G.i32_array(m), G.i32_array(m), G.i32_array(2)
    rc = L.gbls_verify_items_spans(*call_args(msgs[:32 * m], bytes(sig2), bases[:m], masks[:m], clean[:m]),
                                   u64(F.rands(m, 11)), m, G.u32_array([0, 1100, m]), 2, st, kst, v2, 0)
    res["items"] = [rc, L.gbls_last_error(), [v2[0], v2[1]]]
    res["items_status"] = [sum(1 for i in range(m) if st[i]), sum(1 for i in range(m) if kst[i])]
    print(json.dumps(res))


def threads():
    L = G.lib()
    sks = setup(L, b"each/child")
    T, CALLS, N = 8, 20, 9
    seg = [0, 3, 6, 9]
    jobs = []
    for t in range(T):
        rng = random.Random("each/threads/%d" % t)
        bases, masks, fields, sums, msgs = span_sets(sks, N, rng, b"each/thread/%d" % t, shift=t)  # its own committees
        sig = bytearray(compress(L, F.sign(sums, msgs)))
        want_v, want_st, want_kst = [G.SUCCESS] * 3, [0] * N, [0] * N
        if t == 3:
            sig[96 * 3:96 * 4], sig[96 * 4:96 * 5] = sig[96 * 4:96 * 5], sig[96 * 3:96 * 4]
            want_v[1] = G.VERIFY_FAIL
        if t == 5:
            fields[7] = fields[7][:-1]
            want_v[2], want_kst[7] = G.VERIFY_FAIL, G.BAD_ENCODING
        if t == 6:
            sig[0] &= 0x7F   # the compression flag
            want_v[0] = G.VERIFY_FAIL
        want_st = decode_statuses(L, bytes(sig))   # the yardstick: gbls_g2_decompress
        assert (want_st[0] != 0) == (t == 6) and not any(want_st[1:])
        jobs.append((call_args(msgs, bytes(sig), bases, masks, fields), u64(F.rands(N, 100 + t)), want_v, want_st, want_kst))
    barrier = threading.Barrier(T)
    exact = [0] * T
    errors = []

    def run(t):
        args, rands, want_v, want_st, want_kst = jobs[t]
        segs = G.u32_array(seg)
        barrier.wait()
        for _ in range(CALLS):
            st, kst, v = G.i32_array(N), G.i32_array(N), G.i32_array(3)
            rc = L.gbls_verify_items_spans(*args, rands, N, segs, 3, st, kst, v, 0)
            got = (rc, [v[s] for s in range(3)], [st[i] for i in range(N)], [kst[i] for i in range(N)])
            if got == (G.SUCCESS, want_v, want_st, want_kst):
                exact[t] += 1
            else:
                errors.append([t, got[0], got[1], got[2], got[3]])

    pool = [threading.Thread(target=run, args=(t,)) for t in range(T)]
    for th in pool:
        th.start()
    for th in pool:
        th.join()
    print(json.dumps({"threads": T, "calls": CALLS, "exact": exact, "errors": errors[:4]}))


if __name__ == "__main__":
    {"replicas": replicas, "threads": threads}[MODE]()
