"""Subprocess of tests/test_gpu_spans.py, with an engine of its own.

replicas: two engines on the one GPU (gbls_init flags = 2): the member blocks are replicated and a
4200-set one-segment batch takes the sharded-partials path of verify_host, each shard uploading its
slice of the masks and the bits.  Every set spans two committees of at most 9 members, so that
signing stays cheap.  Verdicts clean and with one corrupted set of the second shard.

switch NAME=VALUE: the launch form of k_g1_span_pieces forced through GBLS_COMMITTEE_ROW_MIN
(GBLS_INIT_TUNING): span sets of one to 64 committees in every direction and both encodings, with
plain sets between them, against gbls_g1_aggregate_indexed, and a digest of their bytes.

Prints one JSON line."""
import ctypes
import hashlib
import json
import os
import random
import sys

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
SIZES = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]
KINDS = ["full", "one-clear", "one-set", "half", "most", "few"]


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


def mask_bytes(named):
    out = bytearray(8)
    for c in named:
        out[c >> 3] |= 1 << (c & 7)
    return bytes(out)


def committee_bits(m, kind, rng):
    if kind == "full":
        return [1] * m
    if kind == "one-clear":
        return [int(j != m // 3 or m == 1) for j in range(m)]
    if kind == "one-set":
        return [int(j == (2 * m) // 3) for j in range(m)]
    if kind == "half":
        chosen = set(rng.sample(range(m), max(1, m // 2)))
        return [int(j in chosen) for j in range(m)]
    bits = [int(rng.random() < (0.9 if kind == "most" else 0.25)) for _ in range(m)]
    bits[rng.randrange(m)] = 1
    return bits


def compress(L, sigs):
    n = len(sigs) // 192
    out = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, out), "compress")
    return out.raw


def replicas():
    L = G.lib(0, 2)
    res = {"engines": L.gbls_device_count()}
    sks, comp = F.registry(NREG, seed=b"spans/child")
    assert not F.load_registry(comp).any()
    coms = [[(9 * c + j) % NREG for j in range(3 + c % 7)] for c in range(16)]   # 3..9 members
    set_members(L, 0, coms)
    rng = random.Random("spans/replicas")
    n = 4200
    bases, masks, fields, sums = [], [], [], []
    for i in range(n):
        base, second = i % 13, 1 + i % 3
        per = [committee_bits(len(coms[base + c]), KINDS[(i + c) % len(KINDS)], rng) for c in (0, second)]
        bases.append(base)
        masks.append(mask_bytes([0, second]))
        fields.append(encode(per[0] + per[1], i % 2 == 0))
        sums.append(sum(sks[v] for c, b in zip((0, second), per) for v, x in zip(coms[base + c], b) if x) % F.R_ORDER)
    msgs = F.messages(n, b"spans/big")
    good = compress(L, F.sign(sums, msgs))
    bad = bytearray(good)
    bad[96 * 3000:96 * 3001] = good[96 * 10:96 * 11]  # a set of the second shard
    _, boff = flat(fields)
    rands = u64(F.rands(n, 7 + n))
    out = []
    for sig in (good, bytes(bad)):
        st = G.i32_array(n)
        rc = L.gbls_multi_verify_spans(msgs, sig, G.u32_array(bases), G.buf(b"".join(masks)), G.buf(b"".join(fields)),
                                       G.u32_array(boff), None, None, rands, n, st, 0)
        out.append((rc, L.gbls_last_error()))
    res["big"], res["big_err"] = [o[0] for o in out], [o[1] for o in out]
    print(json.dumps(res))


def switch():
    L = G.lib()
    sks, comp = F.registry(NREG, seed=b"spans/child")
    assert not F.load_registry(comp).any()
    coms = [[(37 * c + 11 * j) % NREG for j in range(SIZES[c % len(SIZES)])] for c in range(64)]
    coms += [[(37 * (200 + c) + 11 * j) % NREG for j in range(512)] for c in range(8)]
    set_members(L, 0, coms)
    rng = random.Random("spans/switch")
    shapes = [(0, [c]) for c in (0, 1, 31, 32, 63)] + [(0, [0, 2, 5]), (3, [0, 2, 5])]
    shapes += [(0, [c, c + 1]) for c in (0, 6, 7, 12, 30, 31, 32, 62)]
    shapes += [(0, list(range(64))), (64, list(range(8))), (60, list(range(12))), (8, list(range(56)))]
    bases, masks, fields, lists, parts, longest = [], [], [], [], [], 0
    for i in range(4 * len(shapes)):
        base, named = shapes[i % len(shapes)]
        per = [committee_bits(len(coms[base + c]), KINDS[(i // len(shapes) + k) % len(KINDS)], rng)
               for k, c in enumerate(named)]
        bases.append(base)
        masks.append(mask_bytes(named))
        fields.append(encode([x for b in per for x in b], i % 2 == 0))
        lists.append([])
        parts.append([v for c, b in zip(named, per) for v, x in zip(coms[base + c], b) if x])
        longest = max([longest] + [min(sum(b), len(b) - sum(b)) for b in per])
        if i % 5 == 2:
            plain = [(300 + i + 11 * j) % NREG for j in range(1 + i % 20)]
            bases.append(G.NO_COMMITTEE)
            masks.append(bytes(8))
            fields.append(b"")
            lists.append(plain)
            parts.append(plain)
    n = len(bases)
    idx, off = flat(lists)
    _, boff = flat(fields)
    got, ref = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(96 * n)
    st, st2 = G.i32_array(n), G.i32_array(n)
    G.check(L.gbls_g1_aggregate_spans(G.u32_array(bases), G.buf(b"".join(masks)), G.buf(b"".join(fields)),
                                      G.u32_array(boff), G.u32_array(idx), G.u32_array(off), n, got, st), "keys")
    idx2, off2 = flat(parts)
    G.check(L.gbls_g1_aggregate_indexed(G.u32_array(idx2), G.u32_array(off2), n, ref, st2), "indexed")
    equal = sum(st[k] == 0 and st2[k] == 0 and got.raw[96 * k:96 * k + 96] == ref.raw[96 * k:96 * k + 96] != bytes(96)
                for k in range(n))
    print(json.dumps({"sets": n, "equal": equal, "longest": longest, "digest": hashlib.sha256(got.raw).hexdigest()}))


if __name__ == "__main__":
    {"replicas": replicas, "switch": switch}[MODE]()
