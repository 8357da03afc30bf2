"""Subprocess of tests/test_gpu_fold.py, with an engine of its own.

single / replicas: one engine, or two engines on the one GPU (gbls_init flags = 2).  2100
independent checks over two-committee spans through gbls_verify_each_fold, with five groups that
name sets all over the call (every fourth set from 0, 1, 2 and 3, and all sets; set 7 twice): a
submission that carries groups stays on one engine, so both modes must give the same verdicts,
counts, sums and bytes.  A bad signature at 3 and at 1500, a malformed string at 100 and at 2000.
The sums are also formed by gbls_g2_decompress + gbls_g2_aggregate_segments over the host-filtered
list, in the same process.

threads: eight threads, each with its OWN 9 sets and its own groups (thread 2 none at all, thread 4
an empty group and a set named twice); thread 3 holds a swapped signature, thread 5 a malformed
string, thread 6 a signature that does not decode.  Every thread first runs its call alone (its
sums checked against gbls_g2_aggregate_segments over the sets that passed), then all start together
behind a barrier and make 20 calls each.  Counts the calls whose outputs are exactly the caller's
solo run: a merged submission rebases the groups on the merged sets.  (Whether calls were merged is
the business of tests/test_fold_sched.py.)

Prints one JSON line."""
import ctypes
import hashlib
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


def fold_call(L, args, n, groups):
    nfold = len(groups)
    fset, foff = C.flat(groups)
    st, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
    out = ctypes.create_string_buffer(192 * max(nfold, 1))
    fb = ctypes.create_string_buffer(96 * max(nfold, 1))
    cnt = G.u32_array([0xEEEEEEEE] * nfold)
    rc = L.gbls_verify_each_fold(*args, n, G.u32_array(fset or [0]), G.u32_array(foff), nfold, st, kst, v, out, fb, cnt)
    return (rc, L.gbls_last_error(), [st[i] for i in range(n)], [kst[i] for i in range(n)], [v[i] for i in range(n)],
            out.raw[:192 * nfold], [cnt[g] for g in range(nfold)], fb.raw[:96 * nfold])


def three_submissions(L, comp, verdicts, groups):
    """gbls_g2_decompress of the passing signatures, then gbls_g2_aggregate_segments (no empty segment)."""
    lists = [[s for s in g if verdicts[s] == G.SUCCESS] for g in groups]
    sent = [k for k, l in enumerate(lists) if l]
    flat = [s for k in sent for s in lists[k]]
    sums = [bytes(192)] * len(groups)
    if not flat:
        return sums
    dec, st = ctypes.create_string_buffer(192 * len(flat)), G.i32_array(len(flat))
    G.check(L.gbls_g2_decompress(b"".join(comp[96 * s:96 * s + 96] for s in flat), len(flat), dec, st), "decompress")
    off = [0]
    for k in sent:
        off.append(off[-1] + len(lists[k]))
    out, ast = ctypes.create_string_buffer(192 * len(sent)), G.i32_array(len(sent))
    G.check(L.gbls_g2_aggregate_segments(dec, G.u32_array(off), len(sent), out, ast), "aggregate")
    for j, k in enumerate(sent):
        sums[k] = out.raw[192 * j:192 * j + 192]
    return sums


def engines(flags):
    L = G.lib(0, flags)
    res = {"engines": L.gbls_device_count()}
    sks = C.setup(L, b"fold/child")
    rng = random.Random("fold/replicas")
    n = 2100
    bases, masks, fields, sums, msgs = C.span_sets(sks, n, rng, b"fold/big")
    sig = bytearray(C.compress(L, F.sign(sums, msgs)))
    for i in (3, 1500):                                 # a valid signature of another set
        sig[96 * i:96 * i + 96] = sig[96 * (i + 10):96 * (i + 11)]
    for i in (100, 2000):                               # a malformed string: its last byte dropped
        fields[i] = fields[i][:-1]
    groups = [list(range(r, n, 4)) for r in range(4)] + [list(range(n)) + [7]]
    rc, err, st, kst, v, out, cnt, fb = fold_call(L, C.call_args(msgs, bytes(sig), bases, masks, fields), n, groups)
    res["rc"] = [rc, err]
    res["failing"] = [i for i in range(n) if v[i] != G.SUCCESS]
    res["want_failing"] = [3, 100, 1500, 2000]
    res["counts"] = cnt
    res["want_counts"] = [len(g) - sum(1 for s in g if s in (3, 100, 1500, 2000)) for g in groups]
    res["sums"] = hashlib.sha256(out).hexdigest()
    res["bytes"] = hashlib.sha256(fb).hexdigest()
    res["three_submissions"] = hashlib.sha256(b"".join(three_submissions(L, bytes(sig), v, groups))).hexdigest()
    print(json.dumps(res))


def threads():
    L = G.lib()
    sks = C.setup(L, b"fold/child")
    T, CALLS, N = 8, 20, 9
    jobs, solo_ok = [], []
    for t in range(T):
        rng = random.Random("fold/threads/%d" % t)
        bases, masks, fields, sums, msgs = C.span_sets(sks, N, rng, b"fold/thread/%d" % t, shift=t)
        sig = bytearray(C.compress(L, F.sign(sums, msgs)))
        bad = set()
        if t == 3:
            sig[96 * 3:96 * 4], sig[96 * 4:96 * 5] = sig[96 * 4:96 * 5], sig[96 * 3:96 * 4]
            bad = {3, 4}
        if t == 5:
            fields[7] = fields[7][:-1]
            bad = {7}
        if t == 6:
            sig[0] &= 0x7F
            bad = {0}
        groups = [[(t + k + 3 * j) % N for j in range(1 + (t + k) % 5)] for k in range(1 + t % 3)] + [list(range(N))]
        if t == 2:
            groups = []
        if t == 4:
            groups = [[], [8, 8, 1], list(range(N))]
        args = C.call_args(msgs, bytes(sig), bases, masks, fields)
        want = fold_call(L, args, N, groups)              # the solo run
        ok = want[0] == G.SUCCESS and {i for i in range(N) if want[4][i] != G.SUCCESS} == bad
        ok = ok and want[5] == b"".join(three_submissions(L, bytes(sig), want[4], groups))
        ok = ok and want[6] == [sum(1 for s in g if s not in bad) for g in groups]
        solo_ok.append(bool(ok))
        jobs.append((args, groups, want))
    barrier = threading.Barrier(T)
    exact = [0] * T
    errors = []

    def run(t):
        args, groups, want = jobs[t]
        barrier.wait()
        for _ in range(CALLS):
            got = fold_call(L, args, N, groups)
            if got == want:
                exact[t] += 1
            else:
                errors.append([t, got[0], got[1], got[4], got[6]])

    pool = [threading.Thread(target=run, args=(t,)) for t in range(T)]
    for th in pool:
        th.start()
    for th in pool:
        th.join()
    print(json.dumps({"threads": T, "calls": CALLS, "exact": exact, "solo_ok": solo_ok, "errors": errors[:4]}))


if __name__ == "__main__":
    {"single": lambda: engines(0), "replicas": lambda: engines(2), "threads": threads}[MODE]()
