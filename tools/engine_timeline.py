#!/usr/bin/env python3
"""A timeline of block imports under gossip load, from the engine's own telemetry (level 2).

Reproduces bench.py's C1 "block under gossip load" leg with the same inputs from grandine_amd.factory:
16 loader threads of 64-set gbls_multi_verify calls, and the mainnet-shaped block (131 sets, ~66 000
registry keys) through gbls_multi_verify_compressed_ex with and without GBLS_CALL_BLOCK.

Per block call it prints the call's phases, read off its shard record (include/
grandine_bls_gpu_telemetry.h) and the caller's own clock (time.monotonic_ns is the engine's steady
clock on Linux):

  total    entry to return, measured here
  queue    first arrival -> start of the submission (hold, window and queue together; the block
           class has no window and is never held)
  lease    start of the submission -> context obtained (the registry lock included)
  enqueue  context obtained -> last launch enqueued (staging waits included, given beside it)
  wait     last launch enqueued -> host wait over
  device   between the two timing events on the shard's main stream
  lag      (wait over - first event recorded) - device: start delay on the GPU + completion notice

and the normal-class shards whose [first event, synced] interval overlaps the block's.  Then, per
mode (with / without GBLS_CALL_BLOCK; fast / slow calls when the totals are bimodal: the largest gap
in the sorted totals, when it exceeds a quarter of the median and leaves a tenth of the calls on
either side) the medians of every phase.  The raw records go to --out as JSON.

  python tools/engine_timeline.py --calls 40 --out timeline.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("total", "queue", "lease", "enqueue", "staging", "wait", "device", "lag")


def phases_of(rec, t0, t1):
    return {"total": t1 - t0, "queue": rec["lead_ns"] - rec["first_arrival_ns"], "lease": rec["lease_ns"] - rec["lead_ns"],
            "enqueue": rec["enqueued_ns"] - rec["lease_ns"], "staging": rec["staging_wait_ns"],
            "wait": rec["synced_ns"] - rec["enqueued_ns"], "device": rec["device_ns"], "lag": rec["lag_ns"]}


def split_modes(calls):
    """[(label, calls)]: one mode, or fast and slow at the midpoint of the largest gap of the totals."""
    tot = sorted(c["phases"]["total"] for c in calls)
    if len(tot) < 10:
        return [("all", calls)]
    gaps = [(b - a, (a + b) // 2, i + 1) for i, (a, b) in enumerate(zip(tot, tot[1:]))]
    gap, mid, below = max(gaps)
    if gap * 4 < statistics.median(tot) or min(below, len(tot) - below) * 10 < len(tot):
        return [("all", calls)]
    return [("fast", [c for c in calls if c["phases"]["total"] <= mid]),
            ("slow", [c for c in calls if c["phases"]["total"] > mid])]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=40, help="block calls per mode")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--load-threads", type=int, default=16)
    ap.add_argument("--registry", type=int, default=1 << 20)
    ap.add_argument("--out", default="engine_timeline.json")
    ap.add_argument("--quiet", action="store_true", help="only the summary")
    args = ap.parse_args()

    import numpy as np
    from grandine_amd import _lib as G
    from grandine_amd import factory as F
    from grandine_amd import telemetry as T

    T.enable(2)
    L = G.lib()
    nreg = args.registry
    sks, comp = F.registry(nreg, seed=b"c1-registry")
    assert not F.load_registry(comp).any()
    rng = np.random.default_rng(1)
    sizes = [1, 1] + [512] * 128 + [512]
    idx = np.concatenate([rng.choice(nreg, size=s, replace=False) for s in sizes]).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = len(sizes)
    msgs = F.messages(n, b"c1")
    sigs, _ = F.committee_signatures(sks, idx, off, msgs)
    comp_sigs = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, comp_sigs), "compress")
    rands = (ctypes.c_uint64 * n)(*F.rands(n, 1))
    pidx, poff = idx.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p)
    gm, gs, gp, gr = F.c2_batch(64, seed=64)
    r64 = (ctypes.c_uint64 * 64)(*gr)

    stop, errs = threading.Event(), []

    def loader():
        while not stop.is_set():
            if L.gbls_multi_verify(gm, gs, gp, r64, 64) != G.SUCCESS:
                errs.append(1)

    def block(flags):
        st = G.i32_array(n)
        t0 = time.monotonic_ns()
        rc = L.gbls_multi_verify_compressed_ex(msgs, comp_sigs, None, pidx, poff, rands, n, st, flags)
        return rc, t0, time.monotonic_ns()

    ths = [threading.Thread(target=loader) for _ in range(args.load_threads)]
    for x in ths:
        x.start()
    time.sleep(0.05)
    result = {"load_threads": args.load_threads, "block_sets": n, "modes": {}}
    for label, flags in (("GBLS_CALL_BLOCK", G.CALL_BLOCK), ("no flag", 0)):
        cls = "block" if flags else "normal"
        for _ in range(args.warmup):
            assert block(flags)[0] == G.SUCCESS
        T.trace()
        calls, lost = [], 0
        for k in range(args.calls):
            rc, t0, t1 = block(flags)
            assert rc == G.SUCCESS
            recs, dropped = T.trace()
            lost += dropped
            mine = [r for r in recs if r["cls"] == cls and r["sets"] == n and t0 <= r["first_arrival_ns"] <= t1]
            if len(mine) != 1:
                continue                      # (its record was overwritten before the drain)
            rec = mine[0]
            beside = [r for r in recs if r is not rec and r["cls"] == "normal" and r["first_event_ns"] and
                      r["first_event_ns"] <= rec["synced_ns"] and r["synced_ns"] >= rec["first_arrival_ns"]]
            calls.append({"call": k, "entry_ns": t0, "return_ns": t1, "phases": phases_of(rec, t0, t1), "record": rec,
                          "beside": beside})
            if not args.quiet:
                p = calls[-1]["phases"]
                print("%-15s call %3d  " % (label, k) + "  ".join("%s %7.3f" % (f, p[f] / 1e6) for f in PHASES) + " ms")
                for r in beside:
                    print("    beside: submission %d  %d callers %4d sets  starts %+8.3f ms  device %7.3f  lag %7.3f  "
                          "ends %+8.3f ms" % (r["submission"], r["callers"], r["sets"],
                                              (r["first_event_ns"] - rec["first_arrival_ns"]) / 1e6, r["device_ns"] / 1e6,
                                              r["lag_ns"] / 1e6, (r["synced_ns"] - rec["first_arrival_ns"]) / 1e6))
        result["modes"][label] = {"calls": calls, "trace_records_lost": lost}
    stop.set()
    for x in ths:
        x.join()
    assert not errs
    result["snapshot"] = {k: v for k, v in T.read().items() if k != "cells"}
    result["memory"] = T.memory()
    summary = {}
    for label, mode in result["modes"].items():
        for part, calls in split_modes(mode["calls"]):
            med = {f: statistics.median(c["phases"][f] for c in calls) / 1e6 for f in PHASES} if calls else {}
            med["beside"] = statistics.median(len(c["beside"]) for c in calls) if calls else 0
            summary["%s / %s" % (label, part)] = {"calls": len(calls), "median_ms": med}
            print("summary %-24s n=%3d  " % ("%s / %s" % (label, part), len(calls)) +
                  "  ".join("%s %7.3f" % (f, med.get(f, 0)) for f in PHASES) + " ms  beside %s" % med["beside"])
    result["summary"] = summary
    with open(args.out, "w") as f:
        json.dump(result, f)
    print("raw records: %s" % args.out)


if __name__ == "__main__":
    main()
