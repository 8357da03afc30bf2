"""Subprocess of tests/test_gpu_msgcache.py: the message line cache on engines that need a fresh
process.  One mode per run, one JSON line out; expected verdicts from the C oracle.

  lane      GBLS_LANE_MIN=1090 (through GBLS_INIT_TUNING): 1100 distinct messages take the
            lane-per-pair radix-2^28 line generator; its lines serve small calls (which would have
            used the one-wave generator) and the other way round
  replicas  two engines on the one GPU (gbls_init flags low byte 2): a 2048-set batch is sharded over
            both, each engine warms its own table
  sliced    GBLS_LINE_BUDGET_MB=16: a 4096-set batch's lines are made in event slices, so the
            submission bypasses the cache
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODE = sys.argv[1]
if MODE == "lane":
    os.environ["GBLS_LANE_MIN"] = "1090"
if MODE == "sliced":
    os.environ["GBLS_LINE_BUDGET_MB"] = "16"

from grandine_amd import _lib as G  # noqa: E402
if MODE in ("lane", "sliced"):
    G.enable_tuning()  # the engine reads the knob set above
from grandine_amd import factory as F  # noqa: E402

STATS = ("lookups", "hits", "misses", "published", "evictions", "bypassed", "entries", "reserved")


def u64(v):
    return (ctypes.c_uint64 * len(v))(*v)


def stats(L):
    out = (ctypes.c_uint64 * 8)()
    assert L.gbls_msgcache_stats(out) == 0
    return dict(zip(STATS, out))


def delta(L, before):
    now = stats(L)
    return {k: now[k] - before[k] for k in STATS[:6]}


def sub(b, idx):
    msgs, sigs, pks, rands = b
    return (b"".join(msgs[32 * i:32 * i + 32] for i in idx), b"".join(sigs[192 * i:192 * i + 192] for i in idx),
            b"".join(pks[96 * i:96 * i + 96] for i in idx), [rands[i] for i in idx])


def swap(b, i, j):
    msgs, sigs, pks, rands = b
    s = bytearray(sigs)
    s[192 * i:192 * i + 192] = sigs[192 * j:192 * j + 192]
    s[192 * j:192 * j + 192] = sigs[192 * i:192 * i + 192]
    return msgs, bytes(s), pks, rands


def main():
    L = G.lib(0, 2) if MODE == "replicas" else G.lib()
    C = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libbls_ref_fast.so"))
    C.ref_multi_verify.argtypes = [ctypes.c_char_p] * 3 + [ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
                                                           ctypes.c_int]

    def ref(b):
        return bool(C.ref_multi_verify(b[0], b[1], b[2], u64(b[3]), len(b[3]), 16))

    def mv(b):
        return L.gbls_multi_verify(b[0], b[1], b[2], u64(b[3]), len(b[3])) == 0

    res = {}
    if MODE == "lane":
        n = 1100
        b = F.c2_batch(n, seed=51)  # distinct messages
        small = sub(b, [0, 7, 1024, 1099])
        bad = swap(small, 1, 2)
        res.update(n=n, ref=[ref(b), ref(small), ref(bad)])
        assert L.gbls_msgcache_configure(2048) == 0
        s0 = stats(L)
        res["cold"] = mv(b)  # k_lines_lane28 writes the 1100 slots
        res["stats_cold"] = delta(L, s0)
        s1 = stats(L)
        res["warm_small"] = [mv(small), mv(bad)]
        res["warm_all"] = mv(b)
        res["stats_warm"] = delta(L, s1)
        assert L.gbls_msgcache_clear() == 0
        assert mv(small)  # the one-wave generator writes 4 slots, consumed beside 1096 lane-form lines
        res["small_then_large"] = mv(b)
    elif MODE == "replicas":
        res["engines"] = L.gbls_device_count()
        # 2048 sets on 64 distinct messages (one segment: per-engine partials, one final exponentiation)
        um = F.messages(64, b"mc/replicas")
        msgs = b"".join(um[32 * (i % 64):32 * (i % 64) + 32] for i in range(2048))
        sks = F.seeded_sks(2048, b"mc/replicas")
        b = (msgs, F.sign(sks, msgs), F.public_keys(sks), F.rands(2048, 53))
        bad = swap(b, 100, 1500)
        res.update(distinct=64, ref=[ref(b), ref(bad)])
        assert L.gbls_msgcache_configure(256) == 0
        s0 = stats(L)
        res["cold"] = mv(b)
        d = delta(L, s0)
        # each engine's shard holds all 64 messages
        res["stats_cold"] = {k: v // 2 for k, v in d.items()}
        assert d["lookups"] == 128
        s1 = stats(L)
        res["warm"] = [mv(b), mv(bad)]
        d = delta(L, s1)
        res["stats_warm"] = {k: v // 2 for k, v in d.items()}
        # small calls alternate between the engines: each finds the messages in its own table
        res["small"] = [mv(sub(b, [k, k + 64, k + 1])) for k in range(4)]
        res["entries"] = stats(L)["entries"] // 2
    elif MODE == "sliced":
        n = 4096
        b = F.c2_batch(n, seed=41)
        bad = swap(b, 2100, 2101)
        res.update(n=n, ref=[ref(b), ref(bad)])
        names = [L.gbls_stage_name(k).decode() for k in range(32) if L.gbls_stage_name(k)]
        calls = (ctypes.c_uint32 * 32)()
        assert L.gbls_msgcache_configure(64) == 0
        L.gbls_profile(1)
        s0 = stats(L)
        res["got"] = [mv(b), mv(bad)]
        res["stats"] = delta(L, s0)
        L.gbls_profile_read(None, calls, 32)
        res["load_store_calls"] = [calls[names.index("k_linecache_load")], calls[names.index("k_linecache_store")]]
        L.gbls_profile(0)
    assert L.gbls_msgcache_configure(0) == 0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
