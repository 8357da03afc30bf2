"""CPU: the message-group path (GBLS_INIT_DEDUP) on the engine's own arithmetic compiled for the
host (tests/native/dedup_harness.cpp): the complete g1s addition of both arithmetic layers against
the oracle's affine addition, and the grouped pipeline against the C oracle's multi_verify."""
import ctypes
import json
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SO = os.path.join(ROOT, "tests", "native", "_build", "libdedup_harness.so")
MONT = 1 << 384
RINV = pow(MONT, -1, O.P)
LAYERS = [0, 1]  # bls_pairing.h g1s_add; bls_curve28.h g1h28_add


@pytest.fixture(scope="module")
def H():
    src = os.path.join(ROOT, "tests", "native", "dedup_harness.cpp")
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                           "-DGBLS_R28_CHECK", "-I/opt/rocm/include", "-o", SO, src])
    L = ctypes.CDLL(SO)
    L.h_multi_verify_dedup.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                       ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32,
                                       ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_int,
                                       ctypes.POINTER(ctypes.c_int32)]
    L.h_g1s_add.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    L.h_g1s_sum28.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    return L


@pytest.fixture(scope="module")
def C():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libbls_ref.so"))
    L.ref_multi_verify.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                   ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_int]
    L.ref_sign.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    L.ref_sk_to_pk.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return L


def fp_b(x):
    return (x * MONT % O.P).to_bytes(48, "little")


def g1_b(p):
    return bytes(96) if p is None else fp_b(p[0]) + fp_b(p[1])


def g2_b(p):
    return bytes(192) if p is None else fp_b(p[0][0]) + fp_b(p[0][1]) + fp_b(p[1][0]) + fp_b(p[1][1])


# ---------------------------------------------------------------- the g1s addition
def g1s_b(p, scale=1):
    """Affine point (or None) as a line-evaluation point (x c, y c, c), c = scale; infinity all-zero."""
    if p is None:
        return bytes(144)
    return fp_b(p[0] * scale % O.P) + fp_b(p[1] * scale % O.P) + fp_b(scale % O.P)


def g1s_affine(b):
    x, y, c = (int.from_bytes(b[48 * k:48 * k + 48], "little") * RINV % O.P for k in range(3))
    if c == 0:
        assert x == 0 and y == 0, "an infinite sum is all-zero"
        return None
    ci = pow(c, -1, O.P)
    return (x * ci % O.P, y * ci % O.P)


def g1s_add(H, a, b, layer):
    out = ctypes.create_string_buffer(144)
    H.h_g1s_add(a, b, out, layer)
    return out.raw


G1 = O.sk_to_pk(1)


@pytest.mark.parametrize("layer", LAYERS)
def test_g1s_add_against_oracle(H, layer):
    rng = random.Random(11 + layer)
    pts = [O.g1_mul(G1, rng.randrange(1, 1 << 64)) for _ in range(12)]
    sc = lambda: rng.randrange(1, O.P)  # a random projective scaling
    for i, p in enumerate(pts):
        q = pts[(i + 5) % len(pts)]
        for sa, sb in ((1, 1), (sc(), 1), (1, sc()), (sc(), sc())):
            assert g1s_affine(g1s_add(H, g1s_b(p, sa), g1s_b(q, sb), layer)) == O.g1_add(p, q)  # random points
            assert g1s_affine(g1s_add(H, g1s_b(p, sa), g1s_b(p, sb), layer)) == O.g1_add(p, p)  # P + P
            assert g1s_affine(g1s_add(H, g1s_b(p, sa), g1s_b(O.g1_neg(p), sb), layer)) is None  # P + (-P)
            assert g1s_affine(g1s_add(H, g1s_b(None), g1s_b(p, sb), layer)) == p  # O + P
            assert g1s_affine(g1s_add(H, g1s_b(p, sa), g1s_b(None), layer)) == p  # P + O
    assert g1s_affine(g1s_add(H, g1s_b(None), g1s_b(None), layer)) is None  # O + O
    assert g1s_add(H, g1s_b(None), g1s_b(None), layer) == bytes(144)
    # the result of P + (-P) is all-zero bytes (what line_eval_s and ml_pc_inf test)
    assert g1s_add(H, g1s_b(pts[0], sc()), g1s_b(O.g1_neg(pts[0]), sc()), layer) == bytes(144)


def test_g1s_chain_in_radix28(H):
    """The kernel's accumulator never leaves the radix-2^28 form between additions: sums of 1 .. 65
    points with doublings, cancellations and infinities inside."""
    rng = random.Random(13)
    base = [O.g1_mul(G1, rng.randrange(1, 1 << 64)) for _ in range(9)]
    for n in (1, 2, 3, 8, 65):
        pts = [base[rng.randrange(len(base))] for _ in range(n)]
        if n >= 8:
            pts[1] = pts[0]  # doubling
            pts[3] = O.g1_neg(pts[2])  # cancellation
            pts[5] = None  # infinity inside
        want = None
        for p in pts:
            want = O.g1_add(want, p)
        out = ctypes.create_string_buffer(144)
        H.h_g1s_sum28(b"".join(g1s_b(p, rng.randrange(1, O.P)) for p in pts), n, out)
        assert g1s_affine(out.raw) == want
    out = ctypes.create_string_buffer(144)
    p = base[0]
    H.h_g1s_sum28(g1s_b(p, 5) + g1s_b(O.g1_neg(p), 7) + g1s_b(p, 9) + g1s_b(O.g1_neg(p), 1), 4, out)
    assert out.raw == bytes(144)


# ---------------------------------------------------------------- the grouped pipeline
def gold(name):
    with open(os.path.join(GOLD, name + ".json")) as fh:
        return json.load(fh)


def case_bytes(c):
    sigs = [g2_b(O.g2_decompress(bytes.fromhex(h))[1]) for h in c["sigs"]]
    pks = [g1_b(O.g1_decompress(bytes.fromhex(h))[1]) for h in c["pks"]]
    msgs = [bytes.fromhex(h) for h in c["msgs"]]
    return msgs, sigs, pks, [int(r) for r in c["rands"]]


def run_dedup(H, msgs, sigs, pks, rands, seg_off, layer):
    n, nseg = len(msgs), len(seg_off) - 1
    v = (ctypes.c_int32 * max(nseg, 1))()
    groups = H.h_multi_verify_dedup(b"".join(msgs), b"".join(sigs), b"".join(pks), (ctypes.c_uint64 * max(n, 1))(*rands),
                                    n, (ctypes.c_uint32 * (nseg + 1))(*seg_off), nseg, layer, v)
    return groups, [v[s] == 0 for s in range(nseg)]


def ref(C, msgs, sigs, pks, rands):
    n = len(msgs)
    return bool(C.ref_multi_verify(b"".join(msgs), b"".join(sigs), b"".join(pks), (ctypes.c_uint64 * n)(*rands), n, 2))


@pytest.mark.parametrize("layer", LAYERS)
def test_golden_multi_verify_cases(H, C, layer):
    for c in gold("multi_verify")["cases"]:
        msgs, sigs, pks, rands = case_bytes(c)
        groups, v = run_dedup(H, msgs, sigs, pks, rands, [0, len(msgs)], layer)
        assert groups == len(set(msgs))
        assert v == [c["expect"]], c["note"]
        assert v == [ref(C, msgs, sigs, pks, rands)], c["note"]


@pytest.mark.parametrize("layer", LAYERS)
def test_golden_cases_doubled(H, C, layer):
    """Every golden case followed by itself under fresh scalars: each message at least twice."""
    rng = random.Random(17)
    for c in gold("multi_verify")["cases"]:
        msgs, sigs, pks, rands = case_bytes(c)
        n = len(msgs)
        r2 = rands + [rng.randrange(1, 1 << 64) for _ in range(n)]
        groups, v = run_dedup(H, msgs * 2, sigs * 2, pks * 2, r2, [0, 2 * n], layer)
        assert groups == len(set(msgs)) < 2 * n
        assert v == [ref(C, msgs * 2, sigs * 2, pks * 2, r2)], c["note"]
        # ... and as two segments of one submission: no grouping across them, per-segment verdicts
        groups, v = run_dedup(H, msgs * 2, sigs * 2, pks * 2, r2, [0, n, 2 * n], layer)
        assert groups == 2 * len(set(msgs))
        assert v == [ref(C, msgs, sigs, pks, r2[:n]), ref(C, msgs, sigs, pks, r2[n:])], c["note"]


def signed_sets(C, rng, nkeys, msgs):
    sks = [rng.randrange(1, O.R).to_bytes(32, "big") for _ in range(nkeys)]
    pks, sigs = [], []
    for sk, m in zip(sks, msgs):
        pk, sig = ctypes.create_string_buffer(96), ctypes.create_string_buffer(192)
        C.ref_sk_to_pk(sk, pk)
        C.ref_sign(sk, m, 32, sig)
        pks.append(pk.raw)
        sigs.append(sig.raw)
    return pks, sigs


@pytest.mark.parametrize("layer", LAYERS)
def test_built_duplicate_cases(H, C, layer):
    rng = random.Random(19)
    a, b = rng.randbytes(32), rng.randbytes(32)
    msgs = [a, a, b, a, a, b, a]
    pks, sigs = signed_sets(C, rng, len(msgs), msgs)
    rands = [rng.randrange(1, 1 << 64) for _ in msgs]
    seg = [0, len(msgs)]
    assert ref(C, msgs, sigs, pks, rands)
    assert run_dedup(H, msgs, sigs, pks, rands, seg, layer) == (2, [True])
    # one corrupted signature inside the group of a, and one in the group of b
    for bad in (3, 2):
        s2 = list(sigs)
        s2[bad] = sigs[(bad + 1) % len(sigs)]
        assert not ref(C, msgs, s2, pks, rands)
        assert run_dedup(H, msgs, s2, pks, rands, seg, layer) == (2, [False])
    # signatures swapped inside one group: fails under distinct scalars, and under equal scalars
    # gives what the oracle gives (the sums coincide)
    s2 = list(sigs)
    s2[0], s2[1] = sigs[1], sigs[0]
    assert not ref(C, msgs, s2, pks, rands)
    assert run_dedup(H, msgs, s2, pks, rands, seg, layer) == (2, [False])
    r2 = list(rands)
    r2[1] = r2[0]
    assert run_dedup(H, msgs, s2, pks, r2, seg, layer) == (2, [ref(C, msgs, s2, pks, r2)])
    # the same set twice under equal scalars (the doubling case of the group sum)
    m3, s3, p3, r3 = msgs + [msgs[0]], sigs + [sigs[0]], pks + [pks[0]], rands + [rands[0]]
    assert ref(C, m3, s3, p3, r3)
    assert run_dedup(H, m3, s3, p3, r3, [0, len(m3)], layer) == (2, [True])
    # an infinite key inside a group, a zero scalar inside a group: both fail
    p4 = list(pks)
    p4[1] = bytes(96)
    assert run_dedup(H, msgs, sigs, p4, rands, seg, layer) == (2, [False])
    r4 = list(rands)
    r4[3] = 0
    assert run_dedup(H, msgs, sigs, pks, r4, seg, layer) == (2, [False])
