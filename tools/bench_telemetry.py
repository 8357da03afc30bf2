#!/usr/bin/env python3
"""What the telemetry levels cost per call (include/grandine_bls_gpu_telemetry.h).

DESIGN §13's protocol: one process, the forms alternating, five runs of 5 warm-up calls and about
0.3 s of timed calls each; reported is the median of the run medians with min..max.  Shapes:
gbls_multi_verify of 64 sets and gbls_verify_each_spans of 64 single-key sets.  Forms: levels 0, 1
and 2 of this library.  With --yardstick PATH (another build of the library inside the package
directory, e.g. the parent commit's, built with `make LIB=libprev BUILD=build_prev`) a child process
runs the same shapes on that library and its figures are printed as the yardstick for level 0: a
library's level cannot be compared with another library's in one process.

Prints one JSON line per (shape, form).

  python tools/bench_telemetry.py [--yardstick grandine_amd/libprev/libgrandine_bls.so]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS, WARMUP, WINDOW = 5, 5, 0.3


def shapes(L, G, F):
    msgs, sigs, pks, rands = F.c2_batch(64, seed=64)
    r64 = (ctypes.c_uint64 * 64)(*rands)
    sks, comp = F.registry(64, seed=b"bench-telemetry")
    assert not F.load_registry(comp).any()
    m2 = F.messages(64, b"bench-telemetry")
    out = ctypes.create_string_buffer(96 * 64)
    G.check(L.gbls_g2_compress(F.sign(sks, m2), 64, out), "compress")
    com = G.u32_array([G.NO_COMMITTEE] * 64)
    cbits, bits, boff = G.buf(bytes(8 * 64)), G.buf(b""), G.u32_array([0] * 65)
    idx, off = G.u32_array(range(64)), G.u32_array(range(65))
    st, kst, v = G.i32_array(64), G.i32_array(64), G.i32_array(64)

    def multi():
        return L.gbls_multi_verify(msgs, sigs, pks, r64, 64)

    def each():
        rc = L.gbls_verify_each_spans(m2, out, com, cbits, bits, boff, idx, off, 64, st, kst, v)
        return rc if rc else max(v[i] for i in range(64))

    return [("gbls_multi_verify x64", multi), ("gbls_verify_each_spans x64", each)]


def one_run(fn):
    for _ in range(WARMUP):
        assert fn() == 0
    lat, end = [], time.perf_counter() + WINDOW
    while time.perf_counter() < end:
        t = time.perf_counter()
        fn()
        lat.append(time.perf_counter() - t)
    return statistics.median(lat) * 1e6


def measure(forms):
    """forms: [(label, setup)] alternating within every run, for every shape."""
    from grandine_amd import _lib as G
    from grandine_amd import factory as F
    L = G.lib()
    for name, fn in shapes(L, G, F):
        meds = {label: [] for label, _ in forms}
        for _ in range(RUNS):
            for label, setup in forms:
                setup(L)
                meds[label].append(one_run(fn))
        for label, _ in forms:
            m = meds[label]
            print(json.dumps({"shape": name, "form": label, "us_per_call_median_of_run_medians": round(statistics.median(m), 2),
                              "min": round(min(m), 2), "max": round(max(m), 2), "runs": RUNS}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--yardstick", help="another build of the library (inside grandine_amd/) as the yardstick for level 0")
    ap.add_argument("--as-yardstick", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.as_yardstick:      # the child: GBLS_LIB names the other library, which has no telemetry entries
        measure([("yardstick library", lambda L: None)])
        return
    if args.yardstick:
        env = dict(os.environ, GBLS_LIB=os.path.abspath(args.yardstick))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--as-yardstick"], env=env, check=True)
    measure([("level %d" % k, lambda L, k=k: (L.gbls_telemetry_enable(k), L.gbls_telemetry_reset())) for k in (0, 1, 2)])


if __name__ == "__main__":
    main()
