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

With --spans the shape is block8x64x512: a block's 8 attestations over all 64 committees of a slot
(include/grandine_bls_gpu_spans.h; 512 committees of 512 members, loaded with their members) and 4
plain single-key sets, the first k members of every committee absent, the forms alternating:

  spans         gbls_multi_verify_spans: base slot, committee_bits and one bit string per set
  lists         gbls_multi_verify_compressed_ex over the full participant index lists
  three         the same result without the spans call, as three submissions: gbls_g1_aggregate_bits
                over the 512 (set, committee) pieces, the host regroup, and
                gbls_multi_verify_compressed_ex over the points, 64 keys per set
  keys_spans    gbls_g1_aggregate_spans (the keys alone)

With --each the shape is gossip64x3, a failed gossip aggregate batch looked at set by set
(include/grandine_bls_gpu_each.h): 64 items of three sets, two plain single-key sets (selection
proof, aggregate-and-proof signature) and one span over 8 committees of 512 members (64 committees
loaded with their members, item i over committees 8 (i % 8) ..), the first k members of every
committee absent, one signature bad, the forms alternating:

  each          gbls_verify_each_spans: one verdict per set
  items         gbls_verify_items_spans: one verdict per item
  points        gbls_verify_batch_compressed over every participant's key point (what the per-set
                fallback did before the each call: yardstick a)
  two           gbls_g1_aggregate_spans, then gbls_verify_batch_compressed over the 192 resulting
                points: two submissions (yardstick b)

With --local the keys are local ones (include/grandine_bls_gpu_local.h: compressed keys with no
registry entry, decoded inside the submission), three parts:

  forms             gbls_g1_aggregate_local over 1, 16, 64, 256, 2048 and 8192 one-key local sets
                    (keys_local) against gbls_g1_decompress(validate = 1) on the same bytes
                    (decompress).  The decode kernel's form follows the table's size (kLocalWaveMax,
                    gbls_local.h); an experiment build (make EXTRA=-DGBLS_LOCAL_WAVE_MAX=...)
                    loaded through GBLS_LIB shows the other form at the same sizes.
  deposits16        16 one-key local sets, one with a bad signature: gbls_verify_each_local
                    (each_local) against gbls_g1_decompress, then gbls_verify_batch_compressed over
                    the points (two: two submissions).
  block8x64x512+16  the --spans block plus 16 one-key local sets: gbls_verify_items_local, one
                    item, GBLS_CALL_BLOCK (items_local) against gbls_g1_decompress, the spans call
                    for the block and gbls_multi_verify_compressed_ex over the 16 (three: three
                    submissions); block is the items call of grandine_bls_gpu_each.h over the block
                    alone, so that the 16 sets' cost shows.

With --fold the call is the verified fold (include/grandine_bls_gpu_fold.h), two shapes of plain
single-key sets with about 1 % bad signatures, the forms alternating:

  fold          gbls_verify_each_fold: the verdicts and, per group, the sum of the signatures that
                passed, one submission
  three         today's best on the same inputs: gbls_verify_each_spans, the host filter of the
                verdicts (vectorised; its share is reported as three_host_filter_us),
                gbls_g2_decompress of the passing signatures, each ONCE, their points copied into
                every segment that names them, gbls_g2_aggregate_segments (three submissions: the
                yardstick)
  each          gbls_verify_each_spans alone: what the fold adds to the tail is fold - each

  singles64     64 sets of one message, one group of all
  subnet2050    2050 sets over four messages (the grouped regime), one group per message and one of
                all

and after the timed runs one profiled pass of each shape gives the fold stage's device time per
call (fold_stage_us, the k_g2_fold line of --stages).

  python tools/bench_committees.py                       # both shapes, one JSON line per point
  python tools/bench_committees.py --bits                # ... the aggregation-bit leg
  python tools/bench_committees.py --spans               # the span-set leg (its own shape)
  python tools/bench_committees.py --each                # per-set and per-item verdicts (its own shape)
  python tools/bench_committees.py --local               # local key sets (--parts forms,deposits16,block)
  python tools/bench_committees.py --fold                # verified folds (its own shapes)
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


def spans_leg(a, G, F, L, emit, absent_counts):
    """block8x64x512: the spans call against the two forms available without it."""
    nset, per_set, size, nplain = 8, 64, 512, 4
    ncom, n = nset * per_set, nset + nplain
    nreg = ncom * size
    seed = b"bench-committees/block8x64x512"
    sks, comp = F.registry(nreg, seed)
    if F.load_registry(comp).any():
        raise SystemExit("registry load failed")
    perm, off = F.committees(nreg, ncom, 7)
    perm_c = np.ascontiguousarray(perm, dtype=np.uint32)
    off_c = np.ascontiguousarray(off, dtype=np.uint32)
    st = G.i32_array(ncom)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = L.gbls_committees_set_members(0, ptr(perm_c), ptr(off_c), ncom, st)
    if rc != G.SUCCESS or any(st[c] for c in range(ncom)):
        raise SystemExit("gbls_committees_set_members rc=%d" % rc)
    emit({"shape": "block8x64x512", "sets": n, "span_sets": nset, "committees_per_set": per_set, "size": size,
          "plain_sets": nplain, "registry": nreg})
    sk = np.array(sks, dtype=object)
    totals = [int(sum(sk[perm[off[c]:off[c + 1]]])) for c in range(ncom)]
    plain = [int(perm[off[7 * i + 3]]) for i in range(nplain)]
    msgs = F.messages(n, seed)
    rands = (ctypes.c_uint64 * n)(*F.rands(n, n + size))
    sig_st = G.i32_array(max(n, ncom + nplain))
    full = np.uint8(0xFF)
    for k in absent_counts:
        sums = []
        for i in range(nset):
            t = 0
            for c in range(per_set * i, per_set * (i + 1)):
                t += totals[c] - int(sum(sk[perm[off[c]:off[c] + k]]))
            sums.append(t % F.R_ORDER)
        sums += [sks[v] for v in plain]
        sigs = F.sign(sums, msgs)
        sig_c = ctypes.create_string_buffer(96 * n)
        G.check(L.gbls_g2_compress(sigs, n, sig_c), "gbls_g2_compress")
        # spans: per set the base slot, all 64 committee bits and one Bitlist over the 64 committees
        base = np.array([per_set * i for i in range(nset)] + [G.NO_COMMITTEE] * nplain, dtype=np.uint32)
        masks = np.zeros((n, 8), dtype=np.uint8)
        masks[:nset] = full
        fields = []
        for i in range(nset):
            bits = np.zeros(8 * (per_set * size // 8 + 1), dtype=np.uint8)
            for c in range(per_set):
                bits[c * size + k:(c + 1) * size] = 1
            bits[per_set * size] = 1  # the delimiter
            fields.append(np.packbits(bits, bitorder="little").tobytes())
        s_all = ctypes.create_string_buffer(b"".join(fields), sum(len(x) for x in fields))
        s_off = np.zeros(n + 1, dtype=np.uint32)
        s_off[1:nset + 1] = np.cumsum([len(x) for x in fields])
        s_off[nset + 1:] = s_off[nset]
        q_idx = np.array(plain, dtype=np.uint32)
        q_off = np.zeros(n + 1, dtype=np.uint32)
        q_off[nset + 1:] = np.arange(1, nplain + 1)
        # lists: every participant's index
        lists = [np.concatenate([perm[off[c] + k:off[c + 1]] for c in range(per_set * i, per_set * (i + 1))])
                 for i in range(nset)] + [np.array([v]) for v in plain]
        l_idx = np.ascontiguousarray(np.concatenate(lists), dtype=np.uint32)
        l_off = np.zeros(n + 1, dtype=np.uint32)
        l_off[1:] = np.cumsum([len(v) for v in lists])
        # three: one single-committee Bitlist per (set, committee) piece, then the plain sets
        npc = ncom + nplain
        p_slots = np.array(list(range(ncom)) + [G.NO_COMMITTEE] * nplain, dtype=np.uint32)
        one = np.zeros(8 * (size // 8 + 1), dtype=np.uint8)
        one[k:size] = 1
        one[size] = 1
        piece = np.packbits(one, bitorder="little").tobytes()
        p_all = ctypes.create_string_buffer(piece * ncom, len(piece) * ncom)
        p_off = np.zeros(npc + 1, dtype=np.uint32)
        p_off[1:ncom + 1] = len(piece) * np.arange(1, ncom + 1)
        p_off[ncom + 1:] = p_off[ncom]
        pq_off = np.zeros(npc + 1, dtype=np.uint32)
        pq_off[ncom + 1:] = np.arange(1, nplain + 1)
        points = ctypes.create_string_buffer(96 * npc)
        g_off = np.zeros(n + 1, dtype=np.uint32)
        keys_out = ctypes.create_string_buffer(96 * n)
        upload = {"spans": 4 * n + 8 * n + 4 * (n + 1) + int(s_off[n]) + 4 * nplain + 4 * (n + 1),
                  "lists": 4 * (n + 1) + 4 * int(l_off[n]),
                  "three": 4 * npc + 4 * (npc + 1) + int(p_off[npc]) + 4 * nplain + 4 * (npc + 1) + 96 * npc + 4 * (n + 1)}

        def call(which):
            t0 = time.perf_counter()
            if which == "spans":
                rc = L.gbls_multi_verify_spans(msgs, sig_c, ptr(base), ptr(masks), s_all, ptr(s_off), ptr(q_idx),
                                               ptr(q_off), rands, n, sig_st, 0)
            elif which == "lists":
                rc = L.gbls_multi_verify_compressed_ex(msgs, sig_c, None, ptr(l_idx), ptr(l_off), rands, n, sig_st, 0)
            elif which == "three":
                rc = L.gbls_g1_aggregate_bits(ptr(p_slots), p_all, ptr(p_off), ptr(q_idx), ptr(pq_off), npc, points,
                                              sig_st)
                if rc == G.SUCCESS:  # the regroup: the pieces are in set order, so it is the offsets
                    g_off[1:nset + 1] = per_set * np.arange(1, nset + 1)
                    g_off[nset + 1:] = ncom + np.arange(1, nplain + 1)
                    rc = L.gbls_multi_verify_compressed_ex(msgs, sig_c, points, None, ptr(g_off), rands, n, sig_st, 0)
            else:
                rc = L.gbls_g1_aggregate_spans(ptr(base), ptr(masks), s_all, ptr(s_off), ptr(q_idx), ptr(q_off), n,
                                               keys_out, sig_st)
            dt = time.perf_counter() - t0
            if rc != G.SUCCESS:
                raise SystemExit("block8x64x512 absent=%d %s: rc=%d err=%d" % (k, which, rc, L.gbls_last_error()))
            return dt

        kinds = (["keys_spans"] if a.keys_only else ["spans", "lists", "three", "keys_spans"])
        f, calls = timed(call, kinds, a.warmup, a.window, a.runs)
        res = {"shape": "block8x64x512", "sets": n, "absent": k, "calls_per_run": calls, "upload_bytes": upload}
        for kind in kinds:
            res[kind] = summary(f[kind])
            res[kind]["runs_us"] = [round(x, 1) for x in f[kind]]
        emit(res)


def each_leg(a, G, F, L, emit, absent_counts):
    """gossip64x3: the per-set and per-item calls against the two forms available without them."""
    nitem, per_set, size, ncom = 64, 8, 512, 64
    n, nreg = 3 * nitem, ncom * size
    seed = b"bench-committees/gossip64x3"
    sks, comp = F.registry(nreg, seed)
    if F.load_registry(comp).any():
        raise SystemExit("registry load failed")
    perm, off = F.committees(nreg, ncom, 7)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    perm_c = np.ascontiguousarray(perm, dtype=np.uint32)
    off_c = np.ascontiguousarray(off, dtype=np.uint32)
    st = G.i32_array(ncom)
    rc = L.gbls_committees_set_members(0, ptr(perm_c), ptr(off_c), ncom, st)
    if rc != G.SUCCESS or any(st[c] for c in range(ncom)):
        raise SystemExit("gbls_committees_set_members rc=%d" % rc)
    emit({"shape": "gossip64x3", "sets": n, "items": nitem, "committees_per_span": per_set, "size": size,
          "registry": nreg})
    raw = F.public_keys(sks)
    pk = np.frombuffer(raw, dtype=np.uint8).reshape(nreg, 96)
    sk = np.array(sks, dtype=object)
    totals = [int(sum(sk[perm[off[c]:off[c + 1]]])) for c in range(ncom)]
    msgs = F.messages(n, seed)
    rands = (ctypes.c_uint64 * n)(*F.rands(n, n + size))
    seg = np.arange(0, n + 1, 3, dtype=np.uint32)
    bad_item = 17
    for k in absent_counts:
        # set 3 i, 3 i + 1: a single key; set 3 i + 2: the span over committees 8 (i % 8) .. + 7
        singles = [int(perm[off[(5 * j) % ncom] + k + j % 7]) for j in range(2 * nitem)]
        sums, lists = [], []
        for i in range(nitem):
            first = per_set * (i % 8)
            t = sum(totals[c] - int(sum(sk[perm[off[c]:off[c] + k]])) for c in range(first, first + per_set))
            sums += [sks[singles[2 * i]], sks[singles[2 * i + 1]], t % F.R_ORDER]
            lists += [np.array([singles[2 * i]]), np.array([singles[2 * i + 1]]),
                      np.concatenate([perm[off[c] + k:off[c + 1]] for c in range(first, first + per_set)])]
        sigs = F.sign(sums, msgs)
        sig_c = ctypes.create_string_buffer(96 * n)
        G.check(L.gbls_g2_compress(sigs, n, sig_c), "gbls_g2_compress")
        b = 96 * (3 * bad_item + 2)  # one bad signature: a valid signature of another set
        sig_c[b:b + 96] = sig_c.raw[96 * 2:96 * 3]
        base = np.full(n, G.NO_COMMITTEE, dtype=np.uint32)
        base[2::3] = [per_set * (i % 8) for i in range(nitem)]
        masks = np.zeros((n, 8), dtype=np.uint8)
        masks[2::3, 0] = 0xFF
        bits = np.zeros(8 * (per_set * size // 8 + 1), dtype=np.uint8)
        for c in range(per_set):
            bits[c * size + k:(c + 1) * size] = 1
        bits[per_set * size] = 1  # the delimiter
        field = np.packbits(bits, bitorder="little").tobytes()
        s_all = ctypes.create_string_buffer(field * nitem, len(field) * nitem)
        s_off = np.zeros(n + 1, dtype=np.uint32)
        s_off[1:] = len(field) * ((np.arange(1, n + 1)) // 3)
        q_idx = np.ascontiguousarray(singles, dtype=np.uint32)
        q_off = np.zeros(n + 1, dtype=np.uint32)
        q_off[1:] = [2 * (j // 3) + min(j % 3, 2) for j in range(1, n + 1)]
        l_idx = np.concatenate(lists)
        l_off = np.zeros(n + 1, dtype=np.uint32)
        l_off[1:] = np.cumsum([len(v) for v in lists])
        l_pts = np.ascontiguousarray(pk[l_idx])
        keys_out = ctypes.create_string_buffer(96 * n)
        sst, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
        span_args = 4 * n + 8 * n + 4 * (n + 1) + int(s_off[n]) + 4 * len(singles) + 4 * (n + 1)
        upload = {"each": span_args, "items": span_args + 8 * n + 4 * (nitem + 1),
                  "points": 4 * (n + 1) + 96 * int(l_off[n]), "two": span_args + 96 * n}
        want = [int(j != 3 * bad_item + 2) for j in range(n)]

        def call(which):
            t0 = time.perf_counter()
            if which == "each":
                rc = L.gbls_verify_each_spans(msgs, sig_c, ptr(base), ptr(masks), s_all, ptr(s_off), ptr(q_idx),
                                              ptr(q_off), n, sst, kst, v)
            elif which == "items":
                rc = L.gbls_verify_items_spans(msgs, sig_c, ptr(base), ptr(masks), s_all, ptr(s_off), ptr(q_idx),
                                               ptr(q_off), rands, n, ptr(seg), nitem, sst, kst, v, 0)
            elif which == "points":
                rc = L.gbls_verify_batch_compressed(msgs, sig_c, ptr(l_pts), ptr(l_off), n, sst, v)
            else:
                rc = L.gbls_g1_aggregate_spans(ptr(base), ptr(masks), s_all, ptr(s_off), ptr(q_idx), ptr(q_off), n,
                                               keys_out, kst)
                if rc == G.SUCCESS:
                    rc = L.gbls_verify_batch_compressed(msgs, sig_c, keys_out, None, n, sst, v)
            dt = time.perf_counter() - t0
            m = nitem if which == "items" else n
            good = [int(v[j] == G.SUCCESS) for j in range(m)]
            if rc != G.SUCCESS or good != ([int(i != bad_item) for i in range(nitem)] if which == "items" else want):
                raise SystemExit("gossip64x3 absent=%d %s: rc=%d err=%d failing=%s" % (
                    k, which, rc, L.gbls_last_error(), [j for j in range(m) if not good[j]]))
            return dt

        kinds = ["each", "items", "points", "two"]
        f, calls = timed(call, kinds, a.warmup, a.window, a.runs)
        res = {"shape": "gossip64x3", "sets": n, "absent": k, "calls_per_run": calls, "upload_bytes": upload}
        for kind in kinds:
            res[kind] = summary(f[kind])
            res[kind]["runs_us"] = [round(x, 1) for x in f[kind]]
        emit(res)


def fold_leg(a, G, F, L, emit):
    """singles64 and subnet2050: the fold call against the three submissions it replaces and against
    the each-call alone."""
    nreg = 4096
    seed = b"bench-committees/fold"
    sks, comp = F.registry(nreg, seed)
    if F.load_registry(comp).any():
        raise SystemExit("registry load failed")
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    names = [L.gbls_stage_name(k).decode() for k in range(32) if L.gbls_stage_name(k)]
    stage = names.index("k_g2_fold")
    for name, n, nmsg in (("singles64", 64, 1), ("subnet2050", 2050, 4)):
        um = F.messages(nmsg, seed + name.encode())
        msgs = b"".join(um[32 * (i % nmsg):32 * (i % nmsg) + 32] for i in range(n))
        idx = np.ascontiguousarray([(7 * i + 3) % nreg for i in range(n)], dtype=np.uint32)
        sigs = F.sign([sks[int(v)] for v in idx], msgs)
        sig_c = ctypes.create_string_buffer(96 * n)
        G.check(L.gbls_g2_compress(sigs, n, sig_c), "gbls_g2_compress")
        bad = sorted({(97 * j + 5) % n for j in range(max(1, n // 100))})
        for i in bad:  # a valid signature of another set
            j = (i + nmsg) % n
            sig_c[96 * i:96 * i + 96] = sig_c.raw[96 * j:96 * j + 96]
        base = np.full(n, G.NO_COMMITTEE, dtype=np.uint32)
        masks = np.zeros((n, 8), dtype=np.uint8)
        boff = np.zeros(n + 1, dtype=np.uint32)
        off = np.arange(n + 1, dtype=np.uint32)
        groups = ([list(range(n))] if nmsg == 1 else
                  [list(range(m, n, nmsg)) for m in range(nmsg)] + [list(range(n))])
        nfold = len(groups)
        fset = np.ascontiguousarray(np.concatenate(groups), dtype=np.uint32)
        foff = np.zeros(nfold + 1, dtype=np.uint32)
        foff[1:] = np.cumsum([len(g) for g in groups])
        sst, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
        out = ctypes.create_string_buffer(192 * nfold)
        out3 = ctypes.create_string_buffer(192 * nfold)
        fb = ctypes.create_string_buffer(96 * nfold)
        cnt = (ctypes.c_uint32 * nfold)()
        dec = ctypes.create_string_buffer(192 * n)
        dst, ast = G.i32_array(n), G.i32_array(nfold)
        want = [int(i not in bad) for i in range(n)]
        # the host side of the three submissions, vectorised: views on the call's own buffers
        v_np = np.frombuffer(v, dtype=np.int32, count=n)
        sig_np = np.frombuffer(sig_c, dtype=np.uint8, count=96 * n).reshape(n, 96)
        dec_np = np.frombuffer(dec, dtype=np.uint8, count=192 * n).reshape(n, 192)
        filter_s = []

        def each():
            return L.gbls_verify_each_spans(msgs, sig_c, ptr(base), ptr(masks), None, ptr(boff), ptr(idx), ptr(off), n,
                                            sst, kst, v)

        def call(which):
            t0 = time.perf_counter()
            if which == "fold":
                rc = L.gbls_verify_each_fold(msgs, sig_c, ptr(base), ptr(masks), None, ptr(boff), ptr(idx), ptr(off), n,
                                             ptr(fset), ptr(foff), nfold, sst, kst, v, out, fb, cnt)
            elif which == "each":
                rc = each()
            else:
                rc = each()
                if rc == G.SUCCESS:
                    # the host filter: every passing signature is decoded ONCE, its point then copied
                    # into every segment that names it
                    t1 = time.perf_counter()
                    ok = v_np == G.SUCCESS
                    passing = np.ascontiguousarray(sig_np[ok])
                    t2 = time.perf_counter()
                    rc = L.gbls_g2_decompress(ptr(passing), len(passing), dec, dst)
                    if rc == G.SUCCESS:
                        t3 = time.perf_counter()
                        where = np.cumsum(ok) - 1            # a passing set's place among the decoded points
                        keep = ok[fset]
                        pts = np.ascontiguousarray(dec_np[where[fset[keep]]])
                        o3 = np.concatenate(([0], np.cumsum(keep)))[foff].astype(np.uint32)
                        t4 = time.perf_counter()
                        filter_s.append((t2 - t1) + (t4 - t3))
                        rc = L.gbls_g2_aggregate_segments(ptr(pts), ptr(o3), nfold, out3, ast)
            dt = time.perf_counter() - t0
            if rc != G.SUCCESS or [int(v[i] == G.SUCCESS) for i in range(n)] != want:
                raise SystemExit("%s %s: rc=%d err=%d" % (name, which, rc, L.gbls_last_error()))
            return dt

        call("fold"), call("three")
        if out.raw != out3.raw or [cnt[g] for g in range(nfold)] != [sum(want[s] for s in g) for g in groups]:
            raise SystemExit("%s: the fold and the three submissions disagree" % name)
        kinds = ["fold", "three", "each"]
        f, calls = timed(call, kinds, a.warmup, a.window, a.runs)
        res = {"shape": name, "sets": n, "groups": nfold, "bad": len(bad), "calls_per_run": calls}
        for kind in kinds:
            res[kind] = summary(f[kind])
            res[kind]["runs_us"] = [round(x, 1) for x in f[kind]]
        res["fold_below_three_range"] = res["fold"]["max_us"] < res["three"]["min_us"]
        res["added_us"] = round(res["fold"]["median_us"] - res["each"]["median_us"], 1)
        # the host filter's share of `three` (numpy on views of the call's buffers), inside its timed window
        res["three_host_filter_us"] = round(statistics.median(filter_s) * 1e6, 1)
        # the fold stage's device time, one profiled pass
        ms, ncalls = (ctypes.c_double * 32)(), (ctypes.c_uint32 * 32)()
        L.gbls_profile(1)
        L.gbls_profile_reset()
        for _ in range(20):
            call("fold")
        L.gbls_profile_read(ms, ncalls, 32)
        L.gbls_profile(0)
        res["fold_stage_us"] = round(1e3 * ms[stage] / max(1, ncalls[stage]), 1)
        res["fold_stage_calls"] = ncalls[stage]
        emit(res)


def local_leg(a, G, F, L, emit, absent_counts):
    """Local key sets: the decode forms, deposits16 and block8x64x512+16."""
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    parts = set(a.parts.split(",")) if a.parts else {"forms", "deposits16", "block"}

    def report(shape, extra, call, kinds):
        f, calls = timed(call, kinds, a.warmup, a.window, a.runs)
        res = dict({"shape": shape, "calls_per_run": calls}, **extra)
        for kind in kinds:
            res[kind] = summary(f[kind])
            res[kind]["runs_us"] = [round(x, 1) for x in f[kind]]
        emit(res)

    def local_sets(nl, first=0):
        """nl one-key local sets behind `first` other sets: com, cbits, bits_off, pk_idx, pk_off tails."""
        return (np.full(nl, G.LOCAL_KEYS, dtype=np.uint32), np.arange(nl, dtype=np.uint32),
                np.arange(first, first + nl + 1, dtype=np.uint32))

    lsks, lcomp = F.registry(8192, b"bench-committees/local")
    if "forms" in parts:
        for nk in (1, 16, 64, 256, 2048, 8192):
            table = ctypes.create_string_buffer(lcomp[:48 * nk], 48 * nk)
            com, idx, off = local_sets(nk)
            masks, boff = np.zeros((nk, 8), dtype=np.uint8), np.zeros(nk + 1, dtype=np.uint32)
            out, st, pst = ctypes.create_string_buffer(96 * nk), G.i32_array(nk), G.i32_array(nk)

            def call(which):
                t0 = time.perf_counter()
                if which == "keys_local":
                    rc = L.gbls_g1_aggregate_local(ptr(com), ptr(masks), None, ptr(boff), ptr(idx), ptr(off), table, nk,
                                                   nk, out, st, pst)
                else:
                    rc = L.gbls_g1_decompress(table, nk, 1, out, st)
                dt = time.perf_counter() - t0
                if rc != G.SUCCESS or any(st[i] for i in range(nk)):
                    raise SystemExit("forms %d %s: rc=%d err=%d" % (nk, which, rc, L.gbls_last_error()))
                return dt

            report("local_forms", {"keys": nk}, call, ["keys_local", "decompress"])
    if "deposits16" in parts:
        nl = 16
        table = ctypes.create_string_buffer(lcomp[:48 * nl], 48 * nl)
        msgs = F.messages(nl, b"bench-committees/deposits16")
        sigs = bytearray(F.sign(lsks[:nl], msgs))
        sigs[192 * 5:192 * 6] = sigs[192 * 6:192 * 7]  # one deposit with another's signature
        sig_c = ctypes.create_string_buffer(96 * nl)
        G.check(L.gbls_g2_compress(bytes(sigs), nl, sig_c), "gbls_g2_compress")
        com, idx, off = local_sets(nl)
        masks, boff = np.zeros((nl, 8), dtype=np.uint8), np.zeros(nl + 1, dtype=np.uint32)
        pts, st, kst, v, pst = ctypes.create_string_buffer(96 * nl), G.i32_array(nl), G.i32_array(nl), G.i32_array(nl), G.i32_array(nl)

        def call(which):
            t0 = time.perf_counter()
            if which == "each_local":
                rc = L.gbls_verify_each_local(msgs, sig_c, ptr(com), ptr(masks), None, ptr(boff), ptr(idx), ptr(off), table,
                                              nl, nl, st, kst, v, pst)
            else:
                rc = L.gbls_g1_decompress(table, nl, 1, pts, pst)
                if rc == G.SUCCESS:
                    rc = L.gbls_verify_batch_compressed(msgs, sig_c, pts, ptr(off), nl, st, v)
            dt = time.perf_counter() - t0
            if rc != G.SUCCESS or [i for i in range(nl) if v[i] != G.SUCCESS] != [5]:
                raise SystemExit("deposits16 %s: rc=%d err=%d" % (which, rc, L.gbls_last_error()))
            return dt

        report("deposits16", {"sets": nl}, call, ["each_local", "two"])
    if "block" not in parts:
        return
    # the --spans block (8 span sets over 64 committees of 512, 4 plain sets) plus 16 local sets
    nset, per_set, size, nplain, nl = 8, 64, 512, 4, 16
    ncom, nb = nset * per_set, nset + nplain
    n, nreg = nb + nl, ncom * size
    seed = b"bench-committees/block8x64x512"
    sks, comp = F.registry(nreg, seed)
    if F.load_registry(comp).any():
        raise SystemExit("registry load failed")
    perm, coff = F.committees(nreg, ncom, 7)
    perm_c, coff_c = np.ascontiguousarray(perm, dtype=np.uint32), np.ascontiguousarray(coff, dtype=np.uint32)
    cst = G.i32_array(ncom)
    rc = L.gbls_committees_set_members(0, ptr(perm_c), ptr(coff_c), ncom, cst)
    if rc != G.SUCCESS or any(cst[c] for c in range(ncom)):
        raise SystemExit("gbls_committees_set_members rc=%d" % rc)
    sk = np.array(sks, dtype=object)
    totals = [int(sum(sk[perm[coff[c]:coff[c + 1]]])) for c in range(ncom)]
    plain = [int(perm[coff[7 * i + 3]]) for i in range(nplain)]
    msgs = F.messages(n, seed + b"+16")
    rands = (ctypes.c_uint64 * n)(*F.rands(n, n + size))
    table = ctypes.create_string_buffer(lcomp[:48 * nl], 48 * nl)
    for k in absent_counts:
        sums = []
        for i in range(nset):
            t = 0
            for c in range(per_set * i, per_set * (i + 1)):
                t += totals[c] - int(sum(sk[perm[coff[c]:coff[c] + k]]))
            sums.append(t % F.R_ORDER)
        sums += [sks[v] for v in plain] + lsks[:nl]
        sig_c = ctypes.create_string_buffer(96 * n)
        G.check(L.gbls_g2_compress(F.sign(sums, msgs), n, sig_c), "gbls_g2_compress")
        lcom, lidx, _ = local_sets(nl)
        base = np.concatenate([np.array([per_set * i for i in range(nset)] + [G.NO_COMMITTEE] * nplain, dtype=np.uint32), lcom])
        masks = np.zeros((n, 8), dtype=np.uint8)
        masks[:nset] = np.uint8(0xFF)
        fields = []
        for i in range(nset):
            bits = np.zeros(8 * (per_set * size // 8 + 1), dtype=np.uint8)
            for c in range(per_set):
                bits[c * size + k:(c + 1) * size] = 1
            bits[per_set * size] = 1  # the delimiter
            fields.append(np.packbits(bits, bitorder="little").tobytes())
        s_all = ctypes.create_string_buffer(b"".join(fields), sum(len(x) for x in fields))
        s_off = np.zeros(n + 1, dtype=np.uint32)
        s_off[1:nset + 1] = np.cumsum([len(x) for x in fields])
        s_off[nset + 1:] = s_off[nset]
        q_idx = np.concatenate([np.array(plain, dtype=np.uint32), lidx])
        q_off = np.zeros(n + 1, dtype=np.uint32)
        q_off[nset + 1:] = np.arange(1, nplain + nl + 1)
        seg_all, seg_block = np.array([0, n], dtype=np.uint32), np.array([0, nb], dtype=np.uint32)
        l_off = np.arange(nl + 1, dtype=np.uint32)
        l_msgs = ctypes.create_string_buffer(msgs[32 * nb:], 32 * nl)
        l_sig = ctypes.create_string_buffer(sig_c.raw[96 * nb:], 96 * nl)
        l_rands = (ctypes.c_uint64 * nl)(*[rands[nb + i] for i in range(nl)])
        pts, st, kst, v, pst = ctypes.create_string_buffer(96 * nl), G.i32_array(n), G.i32_array(n), G.i32_array(1), G.i32_array(nl)

        def call(which):
            t0 = time.perf_counter()
            if which == "items_local":
                rc = L.gbls_verify_items_local(msgs, sig_c, ptr(base), ptr(masks), s_all, ptr(s_off), ptr(q_idx), ptr(q_off),
                                               table, nl, rands, n, ptr(seg_all), 1, st, kst, v, pst, G.CALL_BLOCK)
                rc = rc or v[0]
            elif which == "block":
                rc = L.gbls_verify_items_spans(msgs, sig_c, ptr(base), ptr(masks), s_all, ptr(s_off), ptr(q_idx), ptr(q_off),
                                               rands, nb, ptr(seg_block), 1, st, kst, v, G.CALL_BLOCK)
                rc = rc or v[0]
            else:
                rc = L.gbls_g1_decompress(table, nl, 1, pts, pst)
                if rc == G.SUCCESS:
                    rc = L.gbls_multi_verify_spans(msgs, sig_c, ptr(base), ptr(masks), s_all, ptr(s_off), ptr(q_idx),
                                                   ptr(q_off), rands, nb, st, G.CALL_BLOCK)
                if rc == G.SUCCESS:
                    rc = L.gbls_multi_verify_compressed_ex(l_msgs, l_sig, pts, None, ptr(l_off), l_rands, nl, st,
                                                           G.CALL_BLOCK)
            dt = time.perf_counter() - t0
            if rc != G.SUCCESS:
                raise SystemExit("block8x64x512+16 absent=%d %s: rc=%d err=%d" % (k, which, rc, L.gbls_last_error()))
            return dt

        report("block8x64x512+16", {"sets": n, "local_sets": nl, "absent": k}, call, ["items_local", "three", "block"])


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
    ap.add_argument("--spans", action="store_true",
                    help="the span-set leg: block8x64x512 through the spans call and the two forms without it")
    ap.add_argument("--each", action="store_true",
                    help="the per-set / per-item leg: gossip64x3 through the each and items calls and the two forms "
                         "without them")
    ap.add_argument("--local", action="store_true",
                    help="the local key set leg: the decode forms, deposits16 and block8x64x512+16")
    ap.add_argument("--fold", action="store_true",
                    help="the verified-fold leg: singles64 and subnet2050 through the fold call, the three submissions "
                         "it replaces and the each-call alone")
    ap.add_argument("--parts", default="", help="with --local: comma-separated parts (forms, deposits16, block)")
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

    if a.spans:
        spans_leg(a, G, F, L, emit, [int(x) for x in a.absent.split(",")] if a.absent else [0, 5, 51, 256])
    if a.each:
        each_leg(a, G, F, L, emit, [int(x) for x in a.absent.split(",")] if a.absent else [0, 5, 51])
    if a.local:
        local_leg(a, G, F, L, emit, [int(x) for x in a.absent.split(",")] if a.absent else [5])
    if a.fold:
        fold_leg(a, G, F, L, emit)
    for name, ncom, size in SHAPES:
        if a.spans or a.each or a.local or a.fold or (want and name not in want):
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
