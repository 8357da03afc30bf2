#!/usr/bin/env python3
"""Message line cache (include/grandine_bls_gpu_msgcache.h): call times with the cache off, on and
cold, on and warm, against another build of the library.

Every shape goes through the host-pointer gbls_multi_verify_compressed_ex (96-byte signatures,
point keys, one key per set), one process, one calling thread.  GBLS_LIB selects another build of
the library inside the package directory (grandine_amd/_lib.py); a build without the cache's
entry points measures the "off" legs only.

Legs per shape:
  off         the cache off, GBLS_INIT_DEDUP off
  off+dedup   the cache off, GBLS_INIT_DEDUP on
  cold        the cache on and cleared before every timed call (outside the timed window): every
              call hashes, generates lines and stores them
  warm        the cache on, every message present: every call loads
(with the cache on a submission is always planned by message, so the policy bit has no cold or
warm leg of its own.)

Per leg: RUNS runs, the legs taking turns; a run is WARMUP calls, then CALLS timed calls (a host
clock around each call, which returns after its device synchronise), and its figure is the median
call time.  CALLS is chosen per shape so that a run's timed window is about --window seconds.

  python tools/bench_msgcache.py                       # this build, every shape, one JSON line each
  python tools/bench_msgcache.py --compare lib_x       # this build and grandine_amd/lib_x (another
        # commit's build: make BUILD=build_x LIB=lib_x) in alternating fresh processes, two per
        # library; the runs of a library's processes are pooled, and every figure is a median with
        # its min .. max
  python tools/bench_msgcache.py --stages              # per-stage device times of a cold and a warm
        # call (gbls_profile), and the bytes/s of the load and store kernels at 4096 messages
  python tools/bench_msgcache.py --plan-cost EXE       # the host cost of the plan, by
        # tests/native/msgcache_index_main.cpp built -O2
  python tools/bench_msgcache.py --checks              # per-check calls and prefetch
        # (include/grandine_bls_gpu_msgcache_checks.h), us per call: verify1 (gbls_verify), fav512
        # (one gbls_fast_aggregate_verify over 512 keys), each64x4 (gbls_verify_batch_compressed,
        # 64 checks on 4 roots, one bad), legs off (serving off, the cache on), cold and warm
        # (serving on); prefetch4 and prefetch64: the prefetch call's own time, and the first
        # 64-set gbls_multi_verify after it against the same call cold.  With --compare the other
        # library's "off" leg is the parent's figure; --stages adds the per-stage device times
Every child process runs under a time limit, and the first failure stops the tool.
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

POLICY_DEDUP = 0x800  # GBLS_INIT_DEDUP
SLOT_BYTES = 68 * 72 * 4

# name, sets, distinct messages
SHAPES = [
    ("gossip64_m1", 64, 1),
    ("gossip64_m4", 64, 4),
    ("gossip64_m64", 64, 64),
    ("block131_m131", 131, 131),
    ("sync512_m1", 512, 1),
    ("batch4096_m64", 4096, 64),
    ("batch4096_m2048", 4096, 2048),
]
STAGE_SHAPES = [("gossip64_m4", 64, 4), ("gossip64_m64", 64, 64), ("batch4096_m4096", 4096, 4096)]
CACHE_SLOTS = 8192


def make_shape(G, F, L, n, distinct, seed):
    um = F.messages(distinct, seed)
    msgs = b"".join(um[32 * (i % distinct):32 * (i % distinct) + 32] for i in range(n))
    sks = F.seeded_sks(n, seed)
    sigs = F.sign(sks, msgs)
    comp = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, comp), "gbls_g2_compress")
    rands = (ctypes.c_uint64 * n)(*F.rands(n, n + distinct))
    return msgs, comp.raw, G.buf(F.public_keys(sks)), rands


def summary(figs, n):
    return {"median_us": round(statistics.median(figs), 1), "min_us": round(min(figs), 1), "max_us": round(max(figs), 1),
            "runs_us": [round(x, 1) for x in figs], "sets_per_s": round(n / statistics.median(figs) * 1e6)}


def worker(a):
    from grandine_amd import _lib as G
    from grandine_amd import factory as F
    L = G.lib()
    has_cache = hasattr(L, "gbls_msgcache_configure")
    legs = ["off", "off+dedup"] + (["cold", "warm"] if has_cache else [])
    prev = L.gbls_set_policy(0)
    L.gbls_set_policy(prev)
    print(json.dumps({"library": os.path.relpath(G.LIB_PATH, ROOT), "version": L.gbls_version().decode(),
                      "cache": has_cache, "legs": legs}), flush=True)
    want = set(a.shapes.split(",")) if a.shapes else None

    def set_leg(leg):
        L.gbls_set_policy((prev & ~POLICY_DEDUP) | (POLICY_DEDUP if leg == "off+dedup" else 0))
        if has_cache:
            G.check(L.gbls_msgcache_configure(CACHE_SLOTS if leg in ("cold", "warm") else 0), "configure")

    try:
        if a.stages:
            return stages(a, G, F, L)
        for name, n, distinct in SHAPES:
            if want and name not in want:
                continue
            msgs, comp, pks, rands = make_shape(G, F, L, n, distinct, b"bench-msgcache/" + name.encode())
            st = G.i32_array(n)

            def call(clear=False):
                if clear:
                    L.gbls_msgcache_clear()
                t0 = time.perf_counter()
                rc = L.gbls_multi_verify_compressed_ex(msgs, comp, pks, None, None, rands, n, st, 0)
                dt = time.perf_counter() - t0
                if rc != G.SUCCESS:
                    raise SystemExit("%s: rc=%d" % (name, rc))
                return dt

            figures = {leg: [] for leg in legs}
            calls = 0
            for run in range(a.runs):
                for leg in (legs if run % 2 == 0 else legs[::-1]):
                    set_leg(leg)
                    warm = [call(leg == "cold") for _ in range(a.warmup)]
                    if not calls:
                        calls = int(max(20, min(2000, a.window / max(statistics.median(warm), 1e-6))))
                    figures[leg].append(statistics.median(call(leg == "cold") for _ in range(calls)) * 1e6)
            res = {"shape": name, "sets": n, "distinct": distinct, "calls_per_run": calls}
            for leg in legs:
                res[leg] = summary(figures[leg], n)
            print(json.dumps(res), flush=True)
    finally:
        L.gbls_set_policy(prev)
        if has_cache:
            L.gbls_msgcache_configure(0)


def stages(a, G, F, L):
    """Per-stage device times (events on each stage's stream) of cold and warm calls."""
    names = [L.gbls_stage_name(k).decode() for k in range(32) if L.gbls_stage_name(k)]
    ms = (ctypes.c_double * 32)()
    calls = (ctypes.c_uint32 * 32)()
    for name, n, distinct in STAGE_SHAPES:
        msgs, comp, pks, rands = make_shape(G, F, L, n, distinct, b"bench-msgcache/" + name.encode())
        st = G.i32_array(n)
        res = {"stages_of": name, "sets": n, "distinct": distinct}
        for leg in ("off", "cold", "warm"):
            G.check(L.gbls_msgcache_configure(0 if leg == "off" else CACHE_SLOTS), "configure")
            for _ in range(5):  # buffers, tables
                if leg == "cold":
                    L.gbls_msgcache_clear()
                assert L.gbls_multi_verify_compressed_ex(msgs, comp, pks, None, None, rands, n, st, 0) == 0
            L.gbls_profile(1)
            L.gbls_profile_reset()
            reps = 20
            for _ in range(reps):
                if leg == "cold":
                    L.gbls_msgcache_clear()
                assert L.gbls_multi_verify_compressed_ex(msgs, comp, pks, None, None, rands, n, st, 0) == 0
            L.gbls_profile_read(ms, calls, 32)
            L.gbls_profile(0)
            res[leg] = {nm: round(ms[k] / calls[k] * 1e3, 1) for k, nm in enumerate(names) if calls[k]}  # us per call
            for k, nm in enumerate(names):
                if nm.startswith("k_linecache") and calls[k]:
                    # bytes moved: each slot read once and written once
                    res[leg][nm + "_GBps"] = round(2 * distinct * SLOT_BYTES / (ms[k] / calls[k] * 1e-3) / 1e9, 1)
        print(json.dumps(res), flush=True)
    L.gbls_msgcache_configure(0)


CHECK_SHAPES = ["verify1", "fav512", "each64x4"]


def check_shape(G, F, L, name):
    """-> (call() -> rc, expected rc, checks)"""
    seed = b"bench-msgcache/" + name.encode()
    if name == "verify1":
        msgs, comp, pks, _ = make_shape(G, F, L, 1, 1, seed)
        sks = F.seeded_sks(1, seed)
        sig = G.buf(F.sign(sks, msgs))
        return (lambda: L.gbls_verify(sig, msgs, 32, pks)), 0, 1
    if name == "fav512":
        msg = F.messages(1, seed)
        sks = F.seeded_sks(512, seed)
        sig = G.buf(F.sign([sum(sks) % F.R_ORDER], msg))
        pks = G.buf(F.public_keys(sks))
        return (lambda: L.gbls_fast_aggregate_verify(sig, msg, 32, pks, 512)), 0, 1
    msgs, comp, pks, _ = make_shape(G, F, L, 64, 4, seed)
    comp = comp[:96 * 9] + comp[96 * 10:96 * 11] + comp[96 * 10:]  # check 9 carries check 10's signature
    st, v = G.i32_array(64), G.i32_array(64)
    return (lambda: L.gbls_verify_batch_compressed(msgs, comp, pks, None, 64, st, v)), 0, 64


def checks_worker(a):
    from grandine_amd import _lib as G
    from grandine_amd import factory as F
    L = G.lib()
    serves = hasattr(L, "gbls_msgcache_serve_checks")
    legs = ["off"] + (["cold", "warm"] if serves else [])
    print(json.dumps({"library": os.path.relpath(G.LIB_PATH, ROOT), "version": L.gbls_version().decode(),
                      "serves_checks": serves, "legs": legs}), flush=True)
    want = set(a.shapes.split(",")) if a.shapes else None
    names = [L.gbls_stage_name(k).decode() for k in range(32) if L.gbls_stage_name(k)]
    ms, ncalls = (ctypes.c_double * 32)(), (ctypes.c_uint32 * 32)()

    def set_leg(leg):
        if serves:
            L.gbls_msgcache_serve_checks(0 if leg == "off" else 1)

    def timed(fn, expect, clear):
        if clear:
            L.gbls_msgcache_clear()
        t0 = time.perf_counter()
        rc = fn()
        dt = time.perf_counter() - t0
        if rc != expect:
            raise SystemExit("rc=%d, expected %d" % (rc, expect))
        return dt

    def measure(legs_, fns, n):
        """fns: leg -> (fn, expected rc, clear before each call)."""
        figures = {leg: [] for leg in legs_}
        calls = 0
        for run in range(a.runs):
            for leg in (legs_ if run % 2 == 0 else legs_[::-1]):
                set_leg(leg)
                fn, expect, clear = fns[leg]
                warm = [timed(fn, expect, clear) for _ in range(a.warmup)]
                if not calls:
                    calls = int(max(20, min(2000, a.window / max(statistics.median(warm), 1e-6))))
                figures[leg].append(statistics.median(timed(fn, expect, clear) for _ in range(calls)) * 1e6)
        out = {"calls_per_run": calls}
        for leg in legs_:
            out[leg] = summary(figures[leg], n)
        return out

    def stage_times(fn, expect, clear):
        L.gbls_profile(1)
        L.gbls_profile_reset()
        for _ in range(20):
            timed(fn, expect, clear)
        L.gbls_profile_read(ms, ncalls, 32)
        L.gbls_profile(0)
        return {nm: round(ms[k] / 20 * 1e3, 1) for k, nm in enumerate(names) if ncalls[k]}  # us per call

    G.check(L.gbls_msgcache_configure(CACHE_SLOTS), "configure")
    try:
        for name in CHECK_SHAPES:
            if want and name not in want:
                continue
            fn, expect, n = check_shape(G, F, L, name)
            fns = {"off": (fn, expect, False), "cold": (fn, expect, True), "warm": (fn, expect, False)}
            res = {"shape": name, "sets": n}
            res.update(measure(legs, fns, n))
            if a.stages:
                for leg in legs:
                    set_leg(leg)
                    res["stages:" + leg] = stage_times(*fns[leg])
            print(json.dumps(res), flush=True)
        if serves:
            set_leg("off")
            for name, k in (("prefetch4", 4), ("prefetch64", 64)):
                if want and name not in want:
                    continue
                msgs, comp, pks, rands = make_shape(G, F, L, 64, k, b"bench-msgcache/" + name.encode())
                roots = msgs[:32 * k]
                st = G.i32_array(64)

                def verify():
                    return L.gbls_multi_verify_compressed_ex(msgs, comp, pks, None, None, rands, 64, st, 0)

                def after_prefetch():  # the clear and the prefetch are outside the timed window of `first`
                    L.gbls_msgcache_clear()
                    return L.gbls_msgcache_prefetch(roots, k, None)

                first_figs = {"prefetch": [], "first_after": [], "first_cold": []}
                for run in range(a.runs):
                    for _ in range(a.warmup):
                        after_prefetch()
                        verify()
                    pf, fa, fc = [], [], []
                    for _ in range(max(20, int(a.window / 2e-3))):
                        L.gbls_msgcache_clear()
                        pf.append(timed(lambda: L.gbls_msgcache_prefetch(roots, k, None), 0, False))
                        fa.append(timed(verify, 0, False))
                        fc.append(timed(verify, 0, True))
                    for key, v in (("prefetch", pf), ("first_after", fa), ("first_cold", fc)):
                        first_figs[key].append(statistics.median(v) * 1e6)
                res = {"shape": name, "sets": 64, "distinct": k}
                for key, v in first_figs.items():
                    res[key] = summary(v, 64)
                print(json.dumps(res), flush=True)
    finally:
        if serves:
            L.gbls_msgcache_serve_checks(0)
        L.gbls_msgcache_configure(0)


def plan_cost(exe):
    out = {}
    for n, distinct in ((64, 4), (65536, 1000)):
        txt = subprocess.run([exe, "--time", str(n), str(distinct), "50"], capture_output=True, text=True, timeout=300,
                             check=True).stdout
        out["n%d_m%d_us" % (n, distinct)] = float(txt.split()[1])
    return {"plan_build": out}


def compare(a):
    """Two processes per library, alternating; each under its own time limit; stop at the first failure."""
    libs = [("this", None), ("other", os.path.join(ROOT, "grandine_amd", a.compare, "libgrandine_bls.so"))]
    pooled = {}
    for rnd in range(2):
        for tag, path in (libs if rnd == 0 else libs[::-1]):
            env = dict(os.environ)
            env.pop("GBLS_LIB", None)
            if path:
                env["GBLS_LIB"] = path
            cmd = [sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--warmup", str(a.warmup),
                   "--window", str(a.window)] + (["--shapes", a.shapes] if a.shapes else []) + (
                       ["--checks"] if a.checks else [])
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
            if out.returncode != 0:
                raise SystemExit("%s process failed (rc %d):\n%s" % (tag, out.returncode, out.stderr[-2000:]))
            for ln in out.stdout.splitlines():
                r = json.loads(ln)
                if "shape" not in r:
                    continue
                slot = pooled.setdefault(r["shape"], {"shape": r["shape"], "sets": r["sets"],
                                                      "distinct": r.get("distinct")})
                for leg, v in r.items():
                    if isinstance(v, dict) and "runs_us" in v:
                        slot.setdefault(tag + ":" + leg, []).extend(v["runs_us"])
    for name, slot in pooled.items():
        res = {k: (summary(v, slot["sets"]) if isinstance(v, list) else v) for k, v in slot.items()}
        for k, v in res.items():
            if isinstance(v, dict):
                v.pop("runs_us")
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed calls per run")
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--compare", default="", metavar="LIBDIR", help="another build's directory under grandine_amd/")
    ap.add_argument("--child-timeout", type=float, default=280.0, help="seconds per child process of --compare")
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--checks", action="store_true", help="per-check calls and prefetch")
    ap.add_argument("--plan-cost", default="", metavar="EXE")
    a = ap.parse_args()
    if a.plan_cost:
        print(json.dumps(plan_cost(a.plan_cost)), flush=True)
        return
    if a.compare:
        return compare(a)
    if a.checks:
        return checks_worker(a)
    worker(a)


if __name__ == "__main__":
    main()
