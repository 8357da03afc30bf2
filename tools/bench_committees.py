#!/usr/bin/env python3
"""Cached committee key sums: call times against the participant-list path.

Two C4 shapes, each over a registry just large enough: a slot (64 sets x 512-key committees) and
an epoch (2048 x 512).  Per shape and absentee count the SAME sets (messages, signatures, scalars)
go through three host-pointer, compressed-signature calls, one process, one calling thread:

  parent        gbls_multi_verify_compressed_ex, full participant index lists (the path before
                the committee table existed: the yardstick)
  absentees     gbls_multi_verify_committees, committee slot + absentee list
  participants  gbls_multi_verify_committees, GBLS_NO_COMMITTEE + participant list

RUNS runs alternate the three; a run is WARMUP calls, then CALLS timed calls (a host clock around
each call, which returns after its device synchronise), and its figure is the median call time.
The result line gives the median of the runs' figures and their spread (min .. max).  Also timed:
gbls_committees_set for the shape's committees (the one-off cost per epoch), and with --keys the
key resolution alone (gbls_g1_aggregate_committees), which is what the launch-form switch
(GBLS_COMMITTEE_ROW_MIN, with --tuning) moves.

With --bits the table is loaded with gbls_committees_set_members and the same sets also go through
the aggregation-bit calls (include/grandine_bls_gpu_bits.h), a slot and an SSZ Bitlist per set:

  bits          gbls_multi_verify_bits
  keys_bits     gbls_g1_aggregate_bits (beside keys_absentees / keys_participants)

alternating with the two committees forms (the yardstick of that leg; `parent` is left out), and
each result carries the host bytes a call uploads for its key source (upload_bytes).

  python tools/bench_committees.py                       # both shapes, one JSON line per point
  python tools/bench_committees.py --bits                # ... the aggregation-bit leg
  GBLS_COMMITTEE_ROW_MIN=1 python tools/bench_committees.py --tuning --keys-only
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("slot64x512", 64, 512), ("epoch2048x512", 2048, 512)]
ABSENT = [0, 1, 5, 51, 256, 511]


def timed(fn, runs_of, warmup, window, runs):
    """figures[name] = per-run median call times (us), the names alternating within every run."""
    figures = {k: [] for k in runs_of}
    calls = {}
    names = list(runs_of)
    for run in range(runs):
        order = names[run % len(names):] + names[:run % len(names)]
        for k in order:
            warm = [fn(k) for _ in range(warmup)]
            if k not in calls:
                calls[k] = int(max(10, min(2000, window / max(statistics.median(warm), 1e-6))))
            figures[k].append(statistics.median(fn(k) for _ in range(calls[k])) * 1e6)
    return figures, calls


def summary(f):
    return {"median_us": round(statistics.median(f), 1), "min_us": round(min(f), 1), "max_us": round(max(f), 1)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of timed calls per run")
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: both)")
    ap.add_argument("--absent", default="", help="comma-separated absentee counts (default: %s)" % ABSENT)
    ap.add_argument("--keys", action="store_true", help="also time the key resolution alone")
    ap.add_argument("--keys-only", action="store_true", help="only the key resolution")
    ap.add_argument("--bits", action="store_true",
                    help="the aggregation-bit calls beside the two committees forms, full calls and keys alone")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    ap.add_argument("--tuning", action="store_true", help="let the engine read its GBLS_* tuning variables")
    a = ap.parse_args()

    from grandine_amd import _lib as G
    from grandine_amd import factory as F
    if a.tuning:
        G.enable_tuning()
    L = G.lib()
    lines = [{"library": os.path.relpath(G.LIB_PATH, ROOT), "version": L.gbls_version().decode(),
              "row_min": os.environ.get("GBLS_COMMITTEE_ROW_MIN", "") if a.tuning else ""}]
    want = set(a.shapes.split(",")) if a.shapes else None
    absent_counts = [int(x) for x in a.absent.split(",")] if a.absent else ABSENT

    def emit(res):
        lines.append(res)
        print(json.dumps(res), flush=True)

    for name, ncom, size in SHAPES:
        if want and name not in want:
            continue
        nreg = ncom * size
        seed = b"bench-committees/" + name.encode()
        sks, comp = F.registry(nreg, seed)
        if F.load_registry(comp).any():
            raise SystemExit("registry load failed")
        perm, off = F.committees(nreg, ncom, 7)
        perm_c = np.ascontiguousarray(perm, dtype=np.uint32)
        off_c = np.ascontiguousarray(off, dtype=np.uint32)
        st = G.i32_array(ncom)

        def set_table():
            t0 = time.perf_counter()
            load = L.gbls_committees_set_members if a.bits else L.gbls_committees_set
            rc = load(0, perm_c.ctypes.data_as(ctypes.c_void_p), off_c.ctypes.data_as(ctypes.c_void_p),
                                       ncom, st)
            dt = time.perf_counter() - t0
            if rc != G.SUCCESS or any(st[c] for c in range(ncom)):
                raise SystemExit("%s: %s rc=%d" % (name, "gbls_committees_set_members" if a.bits else "gbls_committees_set", rc))
            return dt

        f, calls = timed(lambda k: set_table(), ["set"], 2, a.window, a.runs)
        emit({"shape": name, "committees": ncom, "size": size, "registry": nreg, "committees_set": summary(f["set"]),
              "calls_per_run": calls["set"]})
        totals = [sum(sks[int(v)] for v in perm[off[c]:off[c + 1]]) % F.R_ORDER for c in range(ncom)]
        msgs = F.messages(ncom, seed)
        rands = (ctypes.c_uint64 * ncom)(*F.rands(ncom, ncom + size))
        sig_st = G.i32_array(ncom)
        for k in absent_counts:
            absent = [perm[off[c]:off[c] + k] for c in range(ncom)]
            part = [perm[off[c] + k:off[c + 1]] for c in range(ncom)]
            sums = [(totals[c] - sum(sks[int(v)] for v in absent[c])) % F.R_ORDER for c in range(ncom)]
            sigs = F.sign(sums, msgs)
            sig_c = ctypes.create_string_buffer(96 * ncom)
            G.check(L.gbls_g2_compress(sigs, ncom, sig_c), "gbls_g2_compress")

            def csr(lists):
                idx = np.ascontiguousarray(np.concatenate(lists) if len(lists) else [], dtype=np.uint32)
                if idx.size == 0:
                    idx = np.zeros(1, dtype=np.uint32)
                o = np.zeros(ncom + 1, dtype=np.uint32)
                o[1:] = np.cumsum([len(v) for v in lists])
                return idx, o

            a_idx, a_off = csr(absent)
            p_idx, p_off = csr(part)
            slots = np.arange(ncom, dtype=np.uint32)
            none = np.full(ncom, G.NO_COMMITTEE, dtype=np.uint32)
            ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
            keys_out = ctypes.create_string_buffer(96 * ncom)
            # an attestation's aggregation_bits per set: a Bitlist over the committee, the first k clear
            fields = []
            for c in range(ncom):
                m = int(off[c + 1] - off[c])
                bits = np.zeros(8 * (m // 8 + 1), dtype=np.uint8)
                bits[k:m] = 1
                bits[m] = 1  # the delimiter
                fields.append(np.packbits(bits, bitorder="little").tobytes())
            b_all = ctypes.create_string_buffer(b"".join(fields), sum(len(x) for x in fields))
            b_off = np.zeros(ncom + 1, dtype=np.uint32)
            b_off[1:] = np.cumsum([len(x) for x in fields])
            upload = {"absentees": 4 * ncom + 4 * (ncom + 1) + 4 * int(a_off[ncom]),
                      "participants": 4 * ncom + 4 * (ncom + 1) + 4 * int(p_off[ncom]),
                      "bits": 4 * ncom + 4 * (ncom + 1) + int(b_off[ncom])}

            def call(which):
                t0 = time.perf_counter()
                if which == "parent":
                    rc = L.gbls_multi_verify_compressed_ex(msgs, sig_c, None, ptr(p_idx), ptr(p_off), rands, ncom,
                                                           sig_st, 0)
                elif which == "absentees":
                    rc = L.gbls_multi_verify_committees(msgs, sig_c, ptr(slots), ptr(a_idx), ptr(a_off), rands, ncom,
                                                        sig_st, 0)
                elif which == "participants":
                    rc = L.gbls_multi_verify_committees(msgs, sig_c, ptr(none), ptr(p_idx), ptr(p_off), rands, ncom,
                                                        sig_st, 0)
                elif which == "bits":
                    rc = L.gbls_multi_verify_bits(msgs, sig_c, ptr(slots), b_all, ptr(b_off), None, None, rands, ncom,
                                                  sig_st, 0)
                elif which == "keys_bits":
                    rc = L.gbls_g1_aggregate_bits(ptr(slots), b_all, ptr(b_off), None, None, ncom, keys_out, sig_st)
                elif which == "keys_absentees":
                    rc = L.gbls_g1_aggregate_committees(ptr(slots), ptr(a_idx), ptr(a_off), ncom, keys_out, sig_st)
                else:
                    rc = L.gbls_g1_aggregate_committees(ptr(none), ptr(p_idx), ptr(p_off), ncom, keys_out, sig_st)
                dt = time.perf_counter() - t0
                if rc != G.SUCCESS:
                    raise SystemExit("%s absent=%d %s: rc=%d err=%d" % (name, k, which, rc, L.gbls_last_error()))
                return dt

            kinds = [] if a.keys_only else ["parent", "absentees", "participants"]
            if a.keys or a.keys_only:
                kinds += ["keys_absentees", "keys_participants"]
            if a.bits:
                kinds = ([] if a.keys_only else ["absentees", "participants", "bits"]) + [
                    "keys_absentees", "keys_participants", "keys_bits"]
            f, calls = timed(call, kinds, a.warmup, a.window, a.runs)
            res = {"shape": name, "sets": ncom, "absent": k, "calls_per_run": calls}
            if a.bits:
                res["upload_bytes"] = upload
            for kind in kinds:
                res[kind] = summary(f[kind])
                res[kind]["runs_us"] = [round(x, 1) for x in f[kind]]
            emit(res)
    print(json.dumps(lines[0]), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
