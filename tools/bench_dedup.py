#!/usr/bin/env python3
"""Message-grouped batch verification (GBLS_INIT_DEDUP): call times with the policy off and on.

Every shape goes through the host-pointer gbls_multi_verify_compressed_ex (96-byte signatures,
point keys, one key per set), one process, one calling thread.  The policy is passed as the
literal 0x800, so the same script runs on a build that predates the bit (gbls_set_policy ignores
it there, and both columns measure the plain path).  GBLS_LIB selects another build of the library
inside the package directory (grandine_amd/_lib.py).

Per shape and policy: RUNS runs, alternating off / on; a run is WARMUP calls, then CALLS timed
calls (a host clock around each call, which returns after its device synchronise), and its figure
is the median call time.  The result line gives the median of the runs' figures and their spread
(min .. max).  CALLS is chosen per shape so that a run's timed window is about --window seconds.

  python tools/bench_dedup.py                      # every shape, one JSON line each
  python tools/bench_dedup.py --plan-cost EXE      # also the host cost of building the plan, by
                                                   # tests/native/dedup_plan_main.cpp built -O2
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POLICY_DEDUP = 0x800  # GBLS_INIT_DEDUP, as a literal (see above)

# name, sets, distinct messages
SHAPES = [
    ("gossip64_m1", 64, 1),
    ("gossip64_m2", 64, 2),
    ("gossip64_m4", 64, 4),
    ("gossip64_m64", 64, 64),
    ("sync512_m1", 512, 1),
    ("block131_m131", 131, 131),
    ("batch4096_m64", 4096, 64),
]
# run only when named in --shapes: many small groups, for the k_g1s_msgsum launch-form switch-over
# (--tuning with GBLS_MSGSUM_WAVE_MIN in the environment)
EXTRA_SHAPES = [
    ("batch4096_m2048", 4096, 2048),
    ("batch4096_m512", 4096, 512),
]


def make_shape(G, F, L, n, distinct, seed):
    um = F.messages(distinct, seed)
    msgs = b"".join(um[32 * (i % distinct):32 * (i % distinct) + 32] for i in range(n))
    sks = F.seeded_sks(n, seed)
    sigs = F.sign(sks, msgs)
    comp = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, comp), "gbls_g2_compress")
    rands = (ctypes.c_uint64 * n)(*F.rands(n, n + distinct))
    return msgs, comp.raw, G.buf(F.public_keys(sks)), rands


def plan_cost(exe):
    rng = random.Random(1)
    out = {}
    for n, distinct in ((64, 2), (65536, 1000)):
        keys = [rng.randbytes(32) for _ in range(distinct)]
        msgs = [keys[i % distinct] for i in range(n)]
        rng.shuffle(msgs)
        with tempfile.NamedTemporaryFile(suffix=".bin") as fh:
            fh.write(struct.pack("<III", n, 1, 0) + struct.pack("<I", n) + b"".join(msgs))
            fh.flush()
            txt = subprocess.run([exe, fh.name, "--time", "50"], capture_output=True, text=True, timeout=300,
                                 check=True).stdout
        out["n%d_m%d_us" % (n, distinct)] = float(txt.strip().splitlines()[-1].split()[1])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed calls per run")
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--plan-cost", default="", metavar="EXE")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    ap.add_argument("--tuning", action="store_true", help="let the engine read its GBLS_* tuning variables")
    a = ap.parse_args()

    from grandine_amd import _lib as G
    from grandine_amd import factory as F
    if a.tuning:
        G.enable_tuning()
    L = G.lib()
    prev = L.gbls_set_policy(POLICY_DEDUP)
    honoured = (L.gbls_set_policy(prev) & POLICY_DEDUP) != 0
    lines = [{"library": os.path.relpath(G.LIB_PATH, ROOT), "version": L.gbls_version().decode(), "policy_bit_honoured": honoured,
              "wave_min": os.environ.get("GBLS_MSGSUM_WAVE_MIN", "") if a.tuning else ""}]
    if a.plan_cost:
        lines.append({"plan_build": plan_cost(a.plan_cost)})
    want = set(a.shapes.split(",")) if a.shapes else None
    try:
        for name, n, distinct in SHAPES + EXTRA_SHAPES:
            if (want and name not in want) or (not want and (name, n, distinct) in EXTRA_SHAPES):
                continue
            msgs, comp, pks, rands = make_shape(G, F, L, n, distinct, b"bench-dedup/" + name.encode())
            st = G.i32_array(n)

            def call():
                t0 = time.perf_counter()
                rc = L.gbls_multi_verify_compressed_ex(msgs, comp, pks, None, None, rands, n, st, 0)
                dt = time.perf_counter() - t0
                if rc != G.SUCCESS:
                    raise SystemExit("%s: rc=%d" % (name, rc))
                return dt

            figures = {"off": [], "on": []}
            calls = 0
            for run in range(a.runs):
                order = ("off", "on") if run % 2 == 0 else ("on", "off")
                for pol in order:
                    L.gbls_set_policy((prev & ~POLICY_DEDUP) | (POLICY_DEDUP if pol == "on" else 0))
                    warm = [call() for _ in range(a.warmup)]
                    if not calls:
                        calls = int(max(20, min(2000, a.window / max(statistics.median(warm), 1e-6))))
                    figures[pol].append(statistics.median(call() for _ in range(calls)) * 1e6)
            res = {"shape": name, "sets": n, "distinct": distinct, "calls_per_run": calls}
            for pol in ("off", "on"):
                f = figures[pol]
                res[pol] = {"median_us": round(statistics.median(f), 1), "min_us": round(min(f), 1),
                            "max_us": round(max(f), 1), "runs_us": [round(x, 1) for x in f],
                            "sets_per_s": round(n / statistics.median(f) * 1e6)}
            lines.append(res)
            print(json.dumps(res), flush=True)
    finally:
        L.gbls_set_policy(prev)
    print(json.dumps(lines[0]), flush=True)
    if a.plan_cost:
        print(json.dumps(lines[1]), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
