"""Child process of tests/test_gpu_dedup.py (run with GBLS_TRACE_DEDUP=1): a 64-set batch of 3
distinct messages and a 64-set batch of distinct messages under GBLS_INIT_DEDUP, with profiling
on.  The parent reads the engine's trace lines from stderr and the k_g1s_msgsum launch counts
printed here."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from grandine_amd import _lib as G  # noqa: E402
from grandine_amd import factory as F  # noqa: E402


def main():
    L = G.lib()
    um = F.messages(3, b"dedup/trace")
    of = [i % 3 for i in range(64)]
    msgs = b"".join(um[32 * g:32 * g + 32] for g in of)
    sks = F.seeded_sks(64, b"dedup/trace")
    pks = F.public_keys(sks)
    grouped = (msgs, F.sign(sks, msgs), pks)
    dm = F.messages(64, b"dedup/trace/distinct")
    distinct = (dm, F.sign(sks, dm), pks)
    rands = (ctypes.c_uint64 * 64)(*F.rands(64, 5))
    stage = [L.gbls_stage_name(k).decode() for k in range(32) if L.gbls_stage_name(k)].index("k_g1s_msgsum")
    calls = (ctypes.c_uint32 * 32)()
    prev = L.gbls_set_policy(G.INIT_DEDUP)
    L.gbls_profile(1)
    ok = True
    try:
        for name, (m, s, p) in (("grouped", grouped), ("distinct", distinct)):
            L.gbls_profile_read(None, calls, 32)
            before = calls[stage]
            ok = L.gbls_multi_verify(m, s, p, rands, 64) == G.SUCCESS and ok
            L.gbls_profile_read(None, calls, 32)
            print("%s msgsum_calls=%d" % (name, calls[stage] - before))
    finally:
        L.gbls_profile(0)
        L.gbls_set_policy(prev)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
