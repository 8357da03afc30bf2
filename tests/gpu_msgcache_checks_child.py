"""Subprocess of tests/test_gpu_msgcache_checks.py: prefetch and served per-check calls on engines
that need a fresh process.  One mode per run, one JSON line out; expected verdicts from the C oracle.

  replicas  two engines on the one GPU (gbls_init flags low byte 2): one prefetch enters its roots
            on both engines; gbls_verify calls, which alternate between the engines, hit on both
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODE = sys.argv[1]

from grandine_amd import _lib as G  # noqa: E402
from grandine_amd import factory as F  # noqa: E402

STATS = ("lookups", "hits", "misses", "published", "evictions", "bypassed", "entries", "reserved")


def stats(L):
    out = (ctypes.c_uint64 * 8)()
    assert L.gbls_msgcache_stats(out) == 0
    return dict(zip(STATS, out))


def delta(L, before):
    now = stats(L)
    return {k: now[k] - before[k] for k in STATS[:6]}


def main():
    assert MODE == "replicas"
    L = G.lib(0, 2)
    C = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libbls_ref.so"))
    C.ref_verify.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    n = 5
    msgs = F.messages(n, b"mcc/replicas")
    sks = F.seeded_sks(n, b"mcc/replicas")
    sigs, pks = F.sign(sks, msgs), F.public_keys(sks)

    def args(i, j):  # check i with check j's signature
        return sigs[192 * j:192 * j + 192], msgs[32 * i:32 * i + 32], 32, pks[96 * i:96 * i + 96]

    def prefetch():
        st = G.i32_array(n)
        for i in range(n):
            st[i] = 77
        assert L.gbls_msgcache_prefetch(msgs, n, st) == 0
        return [st[i] for i in range(n)]

    res = dict(engines=L.gbls_device_count(), distinct=n, ref=[bool(C.ref_verify(*args(0, 0))), bool(C.ref_verify(*args(0, 1)))])
    assert L.gbls_msgcache_configure(256) == 0 and L.gbls_msgcache_serve_checks(1) == 0
    s0 = stats(L)
    res["first"] = prefetch()
    res["stats_prefetch"] = delta(L, s0)
    res["entries"] = stats(L)["entries"]
    res["again"] = prefetch()
    s1 = stats(L)
    res["warm"] = [L.gbls_verify(*args(k % n, k % n if k % 2 == 0 else (k + 1) % n)) == 0 for k in range(8)]
    res["stats_warm"] = delta(L, s1)
    L.gbls_msgcache_serve_checks(0)
    assert L.gbls_msgcache_configure(0) == 0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
