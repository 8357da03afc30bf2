"""Subprocess of tests/test_gpu_local.py, with an engine of its own.

replicas: two engines on the one GPU (gbls_init flags = 2).  4200 independent checks through
gbls_verify_each_local, two-committee spans with every fifth set a local one over a table of 12
keys (one of them not on the curve): whole segments per engine, each shard decoding the whole
table, the table's statuses copied back once.  A bad signature at 3000 (a local set), sets naming
the invalid key at 100 and 4000.  Then gbls_verify_items_local over two 1100-set items, one per
engine, the second holding a bad signature.

threads: eight threads, started together behind a barrier, each making 20 items calls of its own
9-set, 3-item batch with its OWN key table (t + 1 keys, thread 2's empty, positions that only its
own table makes right); thread 3's second item holds a swapped signature, thread 5's set 7 names an
invalid key of its table, thread 6's set 0 a position past its table (inside a merged one).  Counts
the calls whose verdicts and statuses are exactly the caller's own: a merged submission rebases the
positions on the device's table.  (Whether calls were merged is the business of
tests/test_local_sched.py.)

Prints one JSON line."""
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
sys.argv[1] = "none"   # (the each child reads its mode on import)

import gpu_each_child as C  # noqa: E402
from grandine_amd import _lib as G  # noqa: E402
from grandine_amd import factory as F  # noqa: E402

LOCAL = G.LOCAL_KEYS
NOT_ON_CURVE = next(bytes.fromhex(c["in"]) for c in json.load(open(os.path.join(
    ROOT, "tests", "golden", "g1_decode.json")))["cases"] if c["validate_status"] == 2)


def local_args(msgs, sigs, bases, masks, fields, lists, table):
    _, boff = C.flat(fields)
    idx, off = C.flat(lists)
    return (msgs, sigs, G.u32_array(bases), G.buf(b"".join(masks)), G.buf(b"".join(fields)), G.u32_array(boff),
            G.u32_array(idx or [0]), G.u32_array(off), G.buf(b"".join(table)) if table else None, len(table))


def with_local(sks, lsks, n, rng, tag, every, pick, shift=0):
    """n sets, two-committee spans with set i local when i % every == every - 1: its positions are
    pick(i) into the table of lsks."""
    bases, masks, fields, sums, msgs = C.span_sets(sks, n, rng, tag, shift=shift)
    lists = [[] for _ in range(n)]
    for i in range(every - 1, n, every):
        lists[i] = pick(i)
        bases[i], masks[i], fields[i] = LOCAL, bytes(8), b""
        sums[i] = sum(lsks[p] for p in lists[i]) % F.R_ORDER
    return bases, masks, fields, lists, sums, msgs


def replicas():
    L = G.lib(0, 2)
    res = {"engines": L.gbls_device_count()}
    sks = C.setup(L, b"local/child")
    lsks, lcomp = F.registry(11, seed=b"local/child/keys")
    table = [lcomp[48 * j:48 * j + 48] for j in range(11)] + [NOT_ON_CURVE]
    rng = random.Random("local/replicas")
    n = 4200
    bases, masks, fields, lists, sums, msgs = with_local(sks, lsks, n, rng, b"local/big", 5,
                                                         lambda i: [i % 11] if i % 2 else [i % 11, (i + 3) % 11])
    assert bases[3004] == LOCAL
    sig = bytearray(C.compress(L, F.sign(sums, msgs)))
    sig[96 * 3004:96 * 3005] = sig[96 * 9:96 * 10]    # a valid signature of another local set, in the second shard
    clean = [list(v) for v in lists]
    for i in (104, 4004):                              # one set per shard names the invalid key
        assert bases[i] == LOCAL
        lists[i] = lists[i] + [11]
    st, kst, v, pst = G.i32_array(n), G.i32_array(n), G.i32_array(n), G.i32_array(12)
    rc = L.gbls_verify_each_local(*local_args(msgs, bytes(sig), bases, masks, fields, lists, table), n, st, kst, v, pst)
    res["rc"] = [rc, L.gbls_last_error()]
    res["failing"] = [i for i in range(n) if v[i] != G.SUCCESS]
    res["want_failing"] = [104, 3004, 4004]
    res["key_status"] = [[i, kst[i]] for i in range(n) if kst[i]]
    res["want_key_status"] = [[104, G.BAD_ENCODING], [4004, G.BAD_ENCODING]]
    res["pkb_status"] = [pst[j] for j in range(12)]
    res["want_pkb_status"] = [0] * 11 + [2]
    m = 2200
    sig2 = bytearray(C.compress(L, F.sign(sums[:m], msgs[:32 * m])))
    sig2[96 * 1504:96 * 1505] = sig2[96 * 24:96 * 25]
    st, kst, v2, pst = G.i32_array(m), G.i32_array(m), G.i32_array(2), G.i32_array(12)
    rc = L.gbls_verify_items_local(*local_args(msgs[:32 * m], bytes(sig2), bases[:m], masks[:m], fields[:m], clean[:m],
                                               table), C.u64(F.rands(m, 11)), m, G.u32_array([0, 1100, m]), 2, st, kst,
                                   v2, pst, 0)
    assert rc == 0 and not any(st[i] or kst[i] for i in range(m)) and [pst[j] for j in range(12)] == [0] * 11 + [2]
    res["items"] = [v2[0], v2[1]]
    print(json.dumps(res))


def threads():
    L = G.lib()
    sks = C.setup(L, b"local/child")
    T, CALLS, N = 8, 20, 9
    seg = [0, 3, 6, 9]
    jobs = []
    for t in range(T):
        rng = random.Random("local/threads/%d" % t)
        nk = 0 if t == 2 else t + 1
        lsks, lcomp = F.registry(max(nk, 1), seed=b"local/thread/%d" % t)   # every thread its own keys
        table = [lcomp[48 * j:48 * j + 48] for j in range(nk)]
        every = 10 if nk == 0 else 2                                         # thread 2: no local set either
        bases, masks, fields, lists, sums, msgs = with_local(
            sks, lsks, N, rng, b"local/thread/%d" % t, every, lambda i: [(i + k) % nk for k in range(1 + i % 3)], shift=t)
        want_v, want_kst, want_pst = [G.SUCCESS] * 3, [0] * N, [0] * nk
        if t == 5:
            table.append(NOT_ON_CURVE)   # a seventh key, named by set 7 alone
            want_pst.append(2)
            assert bases[7] == LOCAL
            lists[7] = lists[7] + [nk]
            want_v[2], want_kst[7] = G.VERIFY_FAIL, G.BAD_ENCODING
        if t == 6:
            assert bases[1] == LOCAL
            lists[1] = [len(table)]   # past its own table: inside a merged one, another caller's key
            want_v[0], want_kst[1] = G.VERIFY_FAIL, G.BAD_ENCODING
        sig = bytearray(C.compress(L, F.sign(sums, msgs)))
        if t == 3:
            sig[96 * 3:96 * 4], sig[96 * 5:96 * 6] = sig[96 * 5:96 * 6], sig[96 * 3:96 * 4]
            want_v[1] = G.VERIFY_FAIL
        jobs.append((local_args(msgs, bytes(sig), bases, masks, fields, lists, table), C.u64(F.rands(N, 100 + t)), want_v,
                     want_kst, want_pst))
    assert [len(j[4]) for j in jobs] == [1, 2, 0, 4, 5, 7, 7, 8]
    barrier = threading.Barrier(T)
    exact = [0] * T
    errors = []

    def run(t):
        args, rands, want_v, want_kst, want_pst = jobs[t]
        segs, nk = G.u32_array(seg), len(want_pst)
        barrier.wait()
        for _ in range(CALLS):
            st, kst, v, pst = G.i32_array(N), G.i32_array(N), G.i32_array(3), G.i32_array(nk)
            rc = L.gbls_verify_items_local(*args, rands, N, segs, 3, st, kst, v, pst, 0)
            got = (rc, [v[s] for s in range(3)], [st[i] for i in range(N)], [kst[i] for i in range(N)],
                   [pst[j] for j in range(nk)])
            if got == (G.SUCCESS, want_v, [0] * N, want_kst, want_pst):
                exact[t] += 1
            else:
                errors.append([t] + list(got))

    pool = [threading.Thread(target=run, args=(t,)) for t in range(T)]
    for th in pool:
        th.start()
    for th in pool:
        th.join()
    print(json.dumps({"threads": T, "calls": CALLS, "exact": exact, "errors": errors[:4]}))


if __name__ == "__main__":
    {"replicas": replicas, "threads": threads}[MODE]()
