"""Subprocess of tests/test_gpu_telemetry.py: the telemetry level is process-wide and sticky, so every
case runs in a process of its own.  argv: MODE [LEVEL].  Prints one JSON line.

sequence  the fixed call sequence at LEVEL (0, 1 or 2), single-threaded: 4 x gbls_multi_verify of 3
          sets, 2 x gbls_verify_batch_compressed of 5 checks (check 2 of them carries another check's
          signature), one gbls_multi_verify_compressed_ex with GBLS_CALL_BLOCK of 1 set, one
          gbls_verify_each_spans of 3, one gbls_g1_decompress of 2, one gbls_verify_batch_compressed with
          a NULL message pointer.  Reports the verdicts, the snapshot and the drained trace; at level 2
          then 1030 gbls_g1_compress calls of one point and the trace after them.
merge / nomerge
          8 threads x 20 gbls_multi_verify calls of 3 sets at level 1, with the coalescer or with
          GBLS_INIT_NO_COALESCE.
memory    the gauges before gbls_init, after loading the 600-key registry, with the message line cache
          configured to 256 slots and after one served call, after configure(0) and another call, and
          around a small and a larger verification.
device    one gbls_multi_verify_segments_device call on torch tensors at level 1 (and a corrupted one).
replicas  two engines on the one GPU at level 1: a 2100-check gbls_verify_each_spans call is sharded
          over both."""
import ctypes
import json
import os
import random
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
MODE = sys.argv[1]
LEVEL = int(sys.argv[2]) if len(sys.argv) > 2 else 1
sys.argv[1] = "none"   # (the each child reads its mode on import)

import gpu_each_child as C  # noqa: E402
from grandine_amd import _lib as G  # noqa: E402
from grandine_amd import factory as F  # noqa: E402
from grandine_amd import telemetry as T  # noqa: E402


def nonzero_cells(snap):
    """The cells with anything in them, histograms reduced to what the tests compare."""
    out = {}
    for a, row in snap["cells"].items():
        for k, c in row.items():
            if any(c[n] for n in T.COUNTERS) or any(h["count"] for h in c["phases"].values()):
                out["%s/%s" % (a, k)] = c
    return out


def batch(n, seed):
    msgs, sigs, pks, rands = F.c2_batch(n, seed)
    return msgs, sigs, pks, C.u64(rands)


def sequence():
    T.enable(LEVEL)
    L = G.lib()
    sks = C.setup(L, b"telemetry/child")
    m3, s3, p3, r3 = batch(3, 31)
    m5, s5, p5, _ = batch(5, 32)
    c5 = bytearray(C.compress(L, s5))
    c5[96 * 2:96 * 3] = c5[96 * 3:96 * 4]           # check 2: a valid signature of another check
    c5 = bytes(c5)
    m1, s1, p1, r1 = batch(1, 33)
    c1 = C.compress(L, s1)
    bases, masks, fields, sums, sm = C.span_sets(sks, 3, random.Random("telemetry/spans"), b"telemetry/spans")
    sargs = C.call_args(sm, C.compress(L, F.sign(sums, sm)), bases, masks, fields)
    keys48 = F.compress_g1(p3[:192])
    point = p3[:96]
    T.reset()
    res = {"level": LEVEL, "verdicts": []}
    for _ in range(4):
        res["verdicts"].append(L.gbls_multi_verify(m3, s3, p3, r3, 3))
    for _ in range(2):
        st, v = G.i32_array(5), G.i32_array(5)
        rc = L.gbls_verify_batch_compressed(m5, c5, p5, None, 5, st, v)
        res["verdicts"].append([rc, [st[i] for i in range(5)], [v[i] for i in range(5)]])
    st = G.i32_array(1)
    res["verdicts"].append(L.gbls_multi_verify_compressed_ex(m1, c1, p1, None, None, r1, 1, st, G.CALL_BLOCK))
    st, kst, v = G.i32_array(3), G.i32_array(3), G.i32_array(3)
    rc = L.gbls_verify_each_spans(*sargs, 3, st, kst, v)
    res["verdicts"].append([rc, [v[i] for i in range(3)]])
    out, st = ctypes.create_string_buffer(96 * 2), G.i32_array(2)
    res["verdicts"].append([L.gbls_g1_decompress(keys48, 2, 1, out, st), [st[0], st[1]], out.raw == p3[:192]])
    st, v = G.i32_array(5), G.i32_array(5)
    res["rejected"] = [L.gbls_verify_batch_compressed(None, c5, p5, None, 5, st, v), L.gbls_last_error()]
    res["cells"] = nonzero_cells(T.read())
    res["trace"], res["dropped"] = T.trace()
    if LEVEL == 2:
        buf = ctypes.create_string_buffer(48)
        for _ in range(1030):
            assert L.gbls_g1_compress(point, 1, buf) == 0
        recs, dropped = T.trace()
        snap = T.read()
        res["flood"] = {"n": len(recs), "dropped": dropped, "ids": [recs[0]["id"], recs[-1]["id"]],
                        "consecutive": all(b["id"] == a["id"] + 1 for a, b in zip(recs, recs[1:])),
                        "kinds": sorted(set(r["kind"] for r in recs)), "written": snap["trace_written"],
                        "snapshot_dropped": snap["trace_dropped"]}
    print(json.dumps(res))


def merging(flags):
    T.enable(1)
    L = G.lib(0, flags)
    THREADS, CALLS = 8, 20
    jobs = [batch(3, 40 + t) for t in range(THREADS)]
    T.reset()
    barrier = threading.Barrier(THREADS)
    good = [0] * THREADS

    def run(t):
        m, s, p, r = jobs[t]
        barrier.wait()
        for _ in range(CALLS):
            good[t] += L.gbls_multi_verify(m, s, p, r, 3) == G.SUCCESS

    pool = [threading.Thread(target=run, args=(t,)) for t in range(THREADS)]
    for th in pool:
        th.start()
    for th in pool:
        th.join()
    print(json.dumps({"good": good, "cells": nonzero_cells(T.read())}))


def memory():
    res = {"before_init": T.memory()}
    raw = G.TelemetryMemoryInfo()
    G.load_library().gbls_telemetry_memory(ctypes.byref(raw), ctypes.sizeof(raw))
    res["before_init_zero"] = not any(bytes(raw)[8:]) and raw.engines == 0
    L = G.lib()
    C.setup(L, b"telemetry/child")
    res["registry"] = T.memory()
    m3, s3, p3, r3 = batch(3, 31)
    m64, s64, p64, r64 = batch(64, 34)
    assert L.gbls_msgcache_configure(256) == 0
    res["configured"] = T.memory()
    assert L.gbls_multi_verify(m3, s3, p3, r3, 3) == G.SUCCESS
    res["served"] = T.memory()
    assert L.gbls_msgcache_configure(0) == 0
    assert L.gbls_multi_verify(m3, s3, p3, r3, 3) == G.SUCCESS
    res["unconfigured"] = T.memory()
    assert L.gbls_multi_verify(m64, s64, p64, r64, 64) == G.SUCCESS
    res["larger"] = T.memory()
    print(json.dumps(res))


def device():
    import torch
    T.enable(LEVEL)
    L = G.lib()
    dev = torch.device("cuda", 0)
    m3, s3, p3, r3 = F.c2_batch(3, 31)
    bad = bytearray(m3)
    bad[40] ^= 1

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    dm, db, ds, dp = up(m3), up(bytes(bad)), up(s3), up(p3)
    dr = torch.tensor([x - (1 << 64) if x >= 1 << 63 else x for x in r3], dtype=torch.int64, device=dev)
    seg = G.u32_array([0, 3])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    T.reset()
    v = torch.full((1,), -1, dtype=torch.int32, device=dev)
    rc = L.gbls_multi_verify_segments_device(dm.data_ptr(), ds.data_ptr(), dp.data_ptr(), dr.data_ptr(), 3, seg, 1,
                                             v.data_ptr(), st)
    snap = nonzero_cells(T.read())          # before the caller's own synchronisation
    torch.cuda.synchronize()
    res = {"rc": rc, "verdict": int(v.item()), "cells": snap, "trace": T.trace()[0]}
    v2 = torch.full((1,), -1, dtype=torch.int32, device=dev)
    rc2 = L.gbls_multi_verify_segments_device(db.data_ptr(), ds.data_ptr(), dp.data_ptr(), dr.data_ptr(), 3, seg, 1,
                                              v2.data_ptr(), st)
    torch.cuda.synchronize()
    res["corrupted"] = [rc2, int(v2.item())]
    print(json.dumps(res))


def replicas():
    T.enable(1)
    L = G.lib(0, 2)
    res = {"engines": L.gbls_device_count()}
    sks = C.setup(L, b"telemetry/child")
    n = 2100
    bases, masks, fields, sums, msgs = C.span_sets(sks, n, random.Random("telemetry/replicas"), b"telemetry/big")
    args = C.call_args(msgs, C.compress(L, F.sign(sums, msgs)), bases, masks, fields)
    T.reset()
    st, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
    rc = L.gbls_verify_each_spans(*args, n, st, kst, v)
    res["rc"] = [rc, L.gbls_last_error(), sum(1 for i in range(n) if v[i] != G.SUCCESS)]
    res["cells"] = nonzero_cells(T.read())
    res["trace"] = T.trace()[0]
    res["memory"] = T.memory()
    print(json.dumps(res))


if __name__ == "__main__":
    {"sequence": sequence, "merge": lambda: merging(0), "nomerge": lambda: merging(G.INIT_NO_COALESCE),
     "memory": memory, "device": device, "replicas": replicas}[MODE]()
