"""Subprocess of tests/test_gpu_committees.py, with an engine of its own.

replicas: two engines on the one GPU (gbls_init flags = 2): the committee table is replicated, a
4200-set one-segment batch takes the sharded-partials path of verify_host, and four threads verify
while a fifth rewrites another slot range with gbls_committees_set.

switch NAME=VALUE: the list-length switch of k_g1_committee_keys forced through
GBLS_COMMITTEE_ROW_MIN (GBLS_INIT_TUNING): the keys of 150 sets against gbls_g1_aggregate_indexed.

Prints one JSON line."""
import ctypes
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODE = sys.argv[1]
for kv in sys.argv[2:]:
    k, v = kv.split("=", 1)
    assert k.startswith("GBLS_"), kv
    os.environ[k] = v

from grandine_amd import _lib as G  # noqa: E402
if MODE == "switch":
    G.enable_tuning()  # the engine reads the knob set above
from grandine_amd import factory as F  # noqa: E402

NREG = 600


def u64(v):
    return (ctypes.c_uint64 * len(v))(*v)


def flat(lists):
    off = [0]
    for v in lists:
        off.append(off[-1] + len(v))
    return [i for v in lists for i in v], off


def committees_set(L, first, coms):
    idx, off = flat(coms)
    st = G.i32_array(len(coms))
    rc = L.gbls_committees_set(first, G.u32_array(idx), G.u32_array(off), len(coms), st)
    assert rc == 0 and not any(st[c] for c in range(len(coms))), (rc, L.gbls_last_error())


def compress(L, sigs):
    n = len(sigs) // 192
    out = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, out), "compress")
    return out.raw


def signed_sets(L, sks, coms, n, seed):
    """n sets: set i names slot i % len(coms) with i % 3 absentees, signed by the participants."""
    slots, absent, sums = [], [], []
    for i in range(n):
        m = coms[i % len(coms)]
        a = [m[(i + j) % len(m)] for j in range(i % 3)]
        slots.append(i % len(coms))
        absent.append(a)
        sums.append(sum(sks[v] for v in m if v not in a) % F.R_ORDER)
    msgs = F.messages(n, seed)
    return dict(n=n, slots=slots, absent=absent, msgs=msgs, sigs=F.sign(sums, msgs), rands=F.rands(n, 7 + n))


def verify(L, b, sigs_c):
    idx, off = flat(b["absent"])
    st = G.i32_array(b["n"])
    rc = L.gbls_multi_verify_committees(b["msgs"], sigs_c, G.u32_array(b["slots"]), G.u32_array(idx), G.u32_array(off),
                                        u64(b["rands"]), b["n"], st, 0)
    return rc, L.gbls_last_error()


def replicas():
    L = G.lib(0, 2)
    res = {"engines": L.gbls_device_count()}
    sks, comp = F.registry(NREG, seed=b"committees/child")
    assert not F.load_registry(comp).any()
    coms = [[(64 * c + j) % NREG for j in range(64)] for c in range(8)]
    committees_set(L, 0, coms)
    committees_set(L, 8, coms)  # slots 8..15: the range the fifth thread rewrites
    res["table"] = L.gbls_committees_size()
    big = signed_sets(L, sks, coms, 4200, b"committees/big")
    good = compress(L, big["sigs"])
    bad = bytearray(good)
    bad[96 * 3000:96 * 3001] = good[96 * 10:96 * 11]  # a set of the second shard
    out = [verify(L, big, good), verify(L, big, bytes(bad))]
    res["big"], res["big_err"] = [o[0] for o in out], [o[1] for o in out]
    # four verifiers and a writer
    small = signed_sets(L, sks, coms, 64, b"committees/small")
    sg = compress(L, small["sigs"])
    sb = bytearray(sg)
    sb[96 * 5:96 * 6] = sg[96 * 6:96 * 7]
    stats = {"wrong": 0, "errors": 0, "verified": 0, "rewrites": 0}
    lock = threading.Lock()
    stop = threading.Event()
    gate = threading.Barrier(5)

    def verifier(t):
        gate.wait()
        for k in range(6):
            want_ok = (k + t) % 2 == 0
            rc, err = verify(L, small, sg if want_ok else bytes(sb))
            with lock:
                stats["verified"] += 1
                stats["wrong"] += rc != (0 if want_ok else 5)
                stats["errors"] += err != 0

    def writer():
        gate.wait()
        k = 0
        while True:
            committees_set(L, 8, coms[k % 8:] + coms[:k % 8])
            with lock:
                stats["rewrites"] += 1
            k += 1
            if stop.is_set():
                break

    th = [threading.Thread(target=verifier, args=(t,)) for t in range(4)]
    w = threading.Thread(target=writer)
    for x in th + [w]:
        x.start()
    for x in th:
        x.join()
    stop.set()
    w.join()
    stats["errors"] += L.gbls_committees_size() != 16
    res["threads"] = stats
    print(json.dumps(res))


def switch():
    L = G.lib()
    sks, comp = F.registry(NREG, seed=b"committees/child")
    assert not F.load_registry(comp).any()
    sizes = [1, 2, 15, 16, 17, 64, 257]
    coms = [[(37 * c + 11 * j) % NREG for j in range(sizes[c % 7])] for c in range(14)]
    committees_set(L, 0, coms)
    n = 150
    slots, lists, parts = [], [], []
    for i in range(n):
        m = coms[i % 14]
        k = [0, 1, 2, 15, 16, 17, len(m) - 1, len(m)][i % 8]
        a = [m[(i + j) % len(m)] for j in range(min(k, len(m)))]
        p = [v for v in m if v not in a]
        no_com = i % 4 == 3 and p
        slots.append(G.NO_COMMITTEE if no_com else i % 14)
        lists.append(p if no_com else a)
        parts.append(p)
    idx, off = flat(lists)
    got, ref = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(96 * n)
    st, st2 = G.i32_array(n), G.i32_array(n)
    G.check(L.gbls_g1_aggregate_committees(G.u32_array(slots), G.u32_array(idx), G.u32_array(off), n, got, st), "keys")
    idx2, off2 = flat(parts)
    G.check(L.gbls_g1_aggregate_indexed(G.u32_array(idx2), G.u32_array(off2), n, ref, st2), "indexed")
    equal = sum(st[i] == 0 and got.raw[96 * i:96 * i + 96] == ref.raw[96 * i:96 * i + 96] for i in range(n))
    print(json.dumps({"sets": n, "equal": equal, "longest": max(len(v) for v in lists)}))


if __name__ == "__main__":
    {"replicas": replicas, "switch": switch}[MODE]()
