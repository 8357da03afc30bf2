"""Subprocess of tests/test_gpu_bits.py, with an engine of its own.

replicas: two engines on the one GPU (gbls_init flags = 2): the member blocks are replicated, a
4200-set one-segment batch takes the sharded-partials path of verify_host (each shard uploads its
slice of the bits), and four threads verify sets of slots 8..15 while a fifth keeps rewriting slots
8..23 with gbls_committees_set_members: slots 8..15 alternate between a committee and the same
committee reversed, under bits that clear the first and the last member, so the key is the same
whichever order a verification reads; slots 16..23 change their sizes with every rewrite.

switch NAME=VALUE: the launch form of k_g1_bits_keys forced through GBLS_COMMITTEE_ROW_MIN
(GBLS_INIT_TUNING): the keys of every size, pattern and encoding, with plain sets between them,
against gbls_g1_aggregate_indexed, and a digest of their bytes.

Prints one JSON line."""
import ctypes
import hashlib
import json
import os
import random
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
SIZES = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 512, 2048]
PATTERNS = ["all", "none", "one-set", "one-clear", "alternating", "half", "half+1", "random-a", "random-b"]


def u64(v):
    return (ctypes.c_uint64 * len(v))(*v)


def flat(lists):
    off = [0]
    for v in lists:
        off.append(off[-1] + len(v))
    return [i for v in lists for i in v], off


def set_members(L, first, coms):
    idx, off = flat(coms)
    st = G.i32_array(len(coms))
    rc = L.gbls_committees_set_members(first, G.u32_array(idx), G.u32_array(off), len(coms), st)
    assert rc == 0 and not any(st[c] for c in range(len(coms))), (rc, L.gbls_last_error())


def encode(bits, bitlist):
    m = len(bits)
    out = bytearray(m // 8 + 1 if bitlist else (m + 7) // 8)
    for j, b in enumerate(bits):
        out[j >> 3] |= b << (j & 7)
    if bitlist:
        out[m >> 3] |= 1 << (m & 7)
    return bytes(out)


def pattern_bits(m, name):
    rng = random.Random("%d/%s" % (m, name))
    if name == "all":
        return [1] * m
    if name == "none":
        return [0] * m
    if name == "one-set":
        return [int(j == (2 * m) // 3) for j in range(m)]
    if name == "one-clear":
        return [int(j != m // 3) for j in range(m)]
    if name == "alternating":
        return [j & 1 for j in range(m)]
    if name in ("half", "half+1"):
        chosen = set(rng.sample(range(m), min(m, m // 2 + (name == "half+1"))))
        return [int(j in chosen) for j in range(m)]
    return [int(rng.random() < (0.9 if name == "random-a" else 0.3)) for j in range(m)]


def compress(L, sigs):
    n = len(sigs) // 192
    out = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, out), "compress")
    return out.raw


def signed_sets(L, sks, coms, first, n, seed, bits_of):
    """n sets: set i names slot first + i % len(coms) with the bits bits_of(i, m), signed by the
    participants."""
    slots, fields, sums = [], [], []
    for i in range(n):
        m = coms[i % len(coms)]
        bits = bits_of(i, len(m))
        slots.append(first + i % len(coms))
        fields.append(encode(bits, i % 2 == 0))
        sums.append(sum(sks[v] for v, b in zip(m, bits) if b) % F.R_ORDER)
    msgs = F.messages(n, seed)
    return dict(n=n, slots=slots, fields=fields, msgs=msgs, sigs=F.sign(sums, msgs), rands=F.rands(n, 7 + n))


def verify(L, b, sigs_c):
    _, boff = flat(b["fields"])
    st = G.i32_array(b["n"])
    rc = L.gbls_multi_verify_bits(b["msgs"], sigs_c, G.u32_array(b["slots"]), G.buf(b"".join(b["fields"])),
                                  G.u32_array(boff), None, None, u64(b["rands"]), b["n"], st, 0)
    return rc, L.gbls_last_error()


def replicas():
    L = G.lib(0, 2)
    res = {"engines": L.gbls_device_count()}
    sks, comp = F.registry(NREG, seed=b"bits/child")
    assert not F.load_registry(comp).any()
    coms = [[(64 * c + j) % NREG for j in range(64)] for c in range(8)]

    def rewrite(k):
        """slots 8..15: coms in order (k even) or reversed (k odd); slots 16..23: sizes that change"""
        a = [m if k % 2 == 0 else m[::-1] for m in coms]
        b = [[(5 * c + 3 * j + k) % NREG for j in range(1 + (7 * k + 13 * c) % 90)] for c in range(8)]
        set_members(L, 8, a + b)

    set_members(L, 0, coms)
    rewrite(0)
    res["table"] = L.gbls_committees_size()
    big = signed_sets(L, sks, coms, 0, 4200, b"bits/big",
                      lambda i, m: [int(j not in ((i + 1) % m, (3 * i) % m)[:i % 3]) for j in range(m)])
    good = compress(L, big["sigs"])
    bad = bytearray(good)
    bad[96 * 3000:96 * 3001] = good[96 * 10:96 * 11]  # a set of the second shard
    out = [verify(L, big, good), verify(L, big, bytes(bad))]
    res["big"], res["big_err"] = [o[0] for o in out], [o[1] for o in out]
    # four verifiers and a writer: the first and the last member absent, the same key in both orders
    small = signed_sets(L, sks, coms, 8, 64, b"bits/small", lambda i, m: [0] + [1] * (m - 2) + [0])
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
        k = 1
        while True:
            rewrite(k)
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
    stats["errors"] += L.gbls_committees_size() != 24
    stats["errors"] += [L.gbls_committees_members(s) for s in range(16)] != [64] * 16
    res["threads"] = stats
    print(json.dumps(res))


def switch():
    L = G.lib()
    sks, comp = F.registry(NREG, seed=b"bits/child")
    assert not F.load_registry(comp).any()
    coms = [[(37 * c + 11 * j) % NREG for j in range(SIZES[c])] for c in range(len(SIZES))]
    set_members(L, 0, coms)
    slots, fields, lists, parts, longest, i = [], [], [], [], 0, 0
    for c, m in enumerate(SIZES):
        for name in PATTERNS:
            bits = pattern_bits(m, name)
            for bitlist in (False, True):
                slots.append(c)
                fields.append(encode(bits, bitlist))
                lists.append([])
                parts.append([v for v, b in zip(coms[c], bits) if b])
                p = sum(bits)
                longest = max(longest, m - p if m - p < p else p)
                if i % 9 == 4:
                    plain = [(300 + i + 11 * j) % NREG for j in range(1 + i % 20)]
                    slots.append(G.NO_COMMITTEE)
                    fields.append(b"")
                    lists.append(plain)
                    parts.append(plain)
                i += 1
    n = len(slots)
    idx, off = flat(lists)
    _, boff = flat(fields)
    got, ref = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(96 * n)
    st, st2 = G.i32_array(n), G.i32_array(n)
    G.check(L.gbls_g1_aggregate_bits(G.u32_array(slots), G.buf(b"".join(fields)), G.u32_array(boff), G.u32_array(idx),
                                     G.u32_array(off), n, got, st), "keys")
    idx2, off2 = flat(parts)
    G.check(L.gbls_g1_aggregate_indexed(G.u32_array(idx2), G.u32_array(off2), n, ref, st2), "indexed")
    # (a set without participants: the indexed sum reports its empty list, the bytes agree: all-zero)
    equal = sum(st[k] == 0 and st2[k] == (0 if parts[k] else G.AGGR_TYPE_MISMATCH) and
                got.raw[96 * k:96 * k + 96] == ref.raw[96 * k:96 * k + 96] for k in range(n))
    print(json.dumps({"sets": n, "equal": equal, "longest": longest, "digest": hashlib.sha256(got.raw).hexdigest()}))


if __name__ == "__main__":
    {"replicas": replicas, "switch": switch}[MODE]()
