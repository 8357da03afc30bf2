"""CPU: the claims of tests/golden/small_order.json and decode_edges.json re-derived from the
Python oracle (orders, on-curve, statuses, both roots, the class counts), the launch layouts of
tests/edges_cases.py, and the C oracle against the Python oracle for hash_to_G2 at the message and
DST lengths tests/test_gpu_edges.py hashes."""
import ctypes
import os
import subprocess

import pytest

from oracle import bls12_381 as O

import edges_cases as E

H1 = (O.X - 1) ** 2 // 3
H2 = (O.X ** 8 - 4 * O.X ** 7 + 5 * O.X ** 6 - 4 * O.X ** 4 + 6 * O.X ** 3 - 4 * O.X ** 2 - 4 * O.X + 13) // 9


def test_small_order_points():
    s = E.gold("small_order")
    assert [c["order"] for c in s["e2"]] == [13, 23, 2713, 11953]
    assert [c["order"] for c in s["e1"]] == [11, 10177, 859267]
    for c in s["e2"]:
        q = c["order"]
        assert H2 % q == 0 and O.R % q != 0
        t, nt, tg = (E.g2_of_rec(c[k]) for k in ("T", "negT", "T_plus_gen"))
        assert O.g2_on_curve(t) and O.g2_mul(t, q) is None  # q is prime and T is finite: exact order q
        assert nt == O.g2_neg(t) and tg == O.g2_add(t, O.G2_GEN)
        for k, pt in (("T", t), ("negT", nt), ("T_plus_gen", tg)):
            assert O.g2_on_curve(pt) and not O.g2_in_group(pt), (q, k)
            enc = bytes.fromhex(c[k]["enc"])
            assert enc == O.g2_compress(pt) and O.g2_decompress(enc) == (O.SUCCESS, pt)
    for c in s["e1"]:
        q = c["order"]
        assert H1 % q == 0 and O.R % q != 0
        t, tg = E.g1_of_rec(c["T"]), E.g1_of_rec(c["T_plus_gen"])
        assert O.g1_on_curve(t) and O.g1_mul(t, q) is None and tg == O.g1_add(t, O.G1_GEN)
        for k, pt in (("T", t), ("T_plus_gen", tg)):
            assert not O.g1_in_group(pt), (q, k)
            enc = bytes.fromhex(c[k]["enc"])
            assert enc == O.g1_compress(pt) and O.g1_decompress(enc) == (O.SUCCESS, pt)
            assert O.public_key_from_bytes(enc)[0] == O.POINT_NOT_IN_GROUP


def test_which_special_cases_the_membership_chain_can_meet():
    """psi(P) == [x]P runs [|x|]P as 63 doublings and a mixed addition of P at bits 62, 60, 57, 48
    and 16.  Before the addition at bit i the accumulator is [(|x| >> i) - 1]P, so it equals -P
    (the sum is infinity) iff ord(P) divides |x| >> i, and +P (the addition is a doubling) iff
    ord(P) divides (|x| >> i) - 2.  ord(P) divides h2 r: only order 13 at bit 60 meets the first,
    nothing meets the second, and [|x|]P is never infinity for a finite P."""
    from math import gcd
    n = H2 * O.R
    adds = [i for i in range(62, -1, -1) if (O.X_ABS >> i) & 1]
    assert adds == [62, 60, 57, 48, 16] and O.X_ABS >> 63 == 1
    assert {i: gcd(O.X_ABS >> i, n) for i in adds} == {62: 1, 60: 13, 57: 1, 48: 1, 16: 1}
    assert all(gcd((O.X_ABS >> i) - 2, n) == 1 for i in adds) and gcd(O.X_ABS, n) == 1
    t = E.g2_of_rec(E.gold("small_order")["e2"][0]["T"])
    assert O.g2_mul(t, (O.X_ABS >> 60) - 1) == O.g2_neg(t)


def test_g2_roots_in_fp_and_u_fp():
    cases = E.gold("decode_edges")["g2_roots"]
    kinds = {"real": 0, "imag": 0, "re0": 0}
    by_x = {}
    for c in cases:
        x, y = E.g2_of_rec(c)
        a = O.f2_add(O.f2_mul(O.f2_sqr(x), x), O.B2)
        assert O.f2_sqr(y) == a and O.g2_on_curve((x, y))
        if c["class"] == "real":  # y^2 in Fp and a residue: y in Fp, decided by fp2_lex_largest's c1 == 0 branch
            assert a[1] == 0 and O.fp_is_square(a[0]) and y[1] == 0 and y[0] != 0
        elif c["class"] == "imag":  # y^2 in Fp and a non-residue: the delta == 0 fallback of the square root
            assert a[1] == 0 and not O.fp_is_square(a[0]) and y[0] == 0 and y[1] != 0
        else:
            assert c["class"] == "re0" and a[0] == 0 and a[1] != 0 and y[0] != 0 and y[1] != 0
        kinds[c["class"]] += 1
        enc = bytes.fromhex(c["in"])
        assert O.g2_decompress(enc) == (c["status"], (x, y)) == (O.SUCCESS, (x, y)) and O.g2_compress((x, y)) == enc
        assert c["in_group"] == O.g2_in_group((x, y))
        by_x.setdefault(x, []).append((enc[0] & 0x20, y))
    # every point with both sign bits: (x, y) for one, (x, -y) for the other
    for x, lst in by_x.items():
        assert len(lst) == 2 and lst[0][0] != lst[1][0] and lst[0][1] == O.f2_neg(lst[1][1])
    assert kinds["real"] >= 8 and kinds["imag"] >= 8 and kinds["re0"] >= 4  # >= 4, 4 and 2 points, two signs each
    assert not any(c["in_group"] for c in cases)


def test_flag_and_range_edges():
    e = E.gold("decode_edges")
    seen = {}
    for c in e["g2_flags"]:
        enc = bytes.fromhex(c["in"])
        st, pt = O.g2_decompress(enc)
        assert st == c["status"], c["note"]
        seen[c["note"]] = st
        if st == O.SUCCESS and pt is not None:
            assert E.g2_of_rec(c) == pt and c["in_group"] == O.g2_in_group(pt) and O.g2_compress(pt) == enc
    p = O.P
    c1 = lambda b: int.from_bytes(bytes([b[0] & 0x1F]) + b[1:48], "big")  # noqa: E731
    c0 = lambda b: int.from_bytes(b[48:], "big")  # noqa: E731
    enc = {c["note"]: bytes.fromhex(c["in"]) for c in e["g2_flags"]}
    assert seen["0xe0 then zeros"] == seen["all 0xff"] == O.BAD_ENCODING
    assert seen["infinity, non-zero byte in the second half"] == O.BAD_ENCODING
    assert seen["compression bit clear on a valid point"] == O.BAD_ENCODING and seen["valid point"] == O.SUCCESS
    assert c1(enc["x.c1 = p-1, on the curve"]) == p - 1 and seen["x.c1 = p-1, on the curve"] == O.SUCCESS
    assert c0(enc["x.c0 = p-1, on the curve"]) == p - 1 and seen["x.c0 = p-1, on the curve"] == O.SUCCESS
    assert c0(enc["x.c0 = p, valid c1"]) == p and seen["x.c0 = p, valid c1"] == O.BAD_ENCODING
    assert c0(enc["x.c0 = p+1, valid c1"]) == p + 1 and seen["x.c0 = p+1, valid c1"] == O.BAD_ENCODING
    for note in ("x.c1 >= p in its top bits only: 0x1b then zeros",
                 "x.c1 >= p in its top bits only: valid c1 with its five top bits set"):
        v = c1(enc[note])
        assert v >= p > v % (1 << 376) and seen[note] == O.BAD_ENCODING
    assert c1(enc["x = 0"]) == c0(enc["x = 0"]) == 0 and seen["x = 0"] in (O.SUCCESS, O.POINT_NOT_ON_CURVE)
    g1 = {c["note"]: c for c in e["g1_flags"]}
    for c in e["g1_flags"]:
        b = bytes.fromhex(c["in"])
        st, pt = O.g1_decompress(b)
        assert st == c["status"] and O.public_key_from_bytes(b)[0] == c["validate_status"], c["note"]
        if st == O.SUCCESS and pt is not None:
            assert E.g1_of_rec(c) == pt
    assert g1["x = p"]["status"] == g1["x = p, sign bit"]["status"] == g1["x = p+1"]["status"] == O.BAD_ENCODING
    assert g1["0xa0 then zeros"]["status"] == O.POINT_NOT_IN_GROUP and g1["0xe0 then zeros"]["status"] == O.BAD_ENCODING
    assert g1["largest x on the curve"]["status"] == O.SUCCESS
    assert int.from_bytes(bytes.fromhex(g1["x = p-1"]["in"]), "big") & ((1 << 381) - 1) == p - 1


def test_launch_layouts():
    """The lane launch is longer than the row form takes, its last wave is partly filled, and the
    edge cases sit in the first wave, across a 64-lane boundary and in the last wave."""
    edges = E.g2_edge_encodings()
    lane = E.g2_lane_launch()
    assert len(edges) <= E.ROW_MAX < len(lane) == E.LANE_N <= 2200
    where = [i for i, (lab, _) in enumerate(lane) if not lab.startswith("valid #")]
    assert len(where) == 2 * len(edges)
    assert where[0] < 64 <= where[len(edges) - 1] and where[-1] == E.LANE_N - 1 and where[len(edges)] < E.LANE_N - 38
    statuses = {O.g2_decompress(enc)[0] for _, enc in edges}
    assert statuses == {O.SUCCESS, O.BAD_ENCODING, O.POINT_NOT_ON_CURVE}
    g1, known = E.g1_ragged_launch()
    assert len(g1) == E.G1_RAGGED_N and len(known) == E.G1_RAGGED_N - len(E.g1_edge_encodings())
    assert all(O.g1_decompress(g1[i][1]) == (O.SUCCESS, p) for i, p in list(known.items())[:5])
    mem = E.g2_membership_cases()
    assert {st for _, _, st in mem} == {O.SUCCESS, O.POINT_NOT_IN_GROUP}
    assert sum(1 for _, p, _ in mem if p is None) >= 4


def test_message_and_dst_lengths_cross_the_block_boundaries():
    assert E.b0_blocks(8, 43) + 1 == E.b0_blocks(9, 43) and E.b0_blocks(72, 43) + 1 == E.b0_blocks(73, 43)
    assert E.b0_blocks(136, 43) + 1 == E.b0_blocks(137, 43)
    for lo, hi in ((21, 22), (85, 86), (149, 150), (213, 214)):
        assert E.bi_blocks(lo) + 1 == E.bi_blocks(hi) and lo in E.DST_LENGTHS and hi in E.DST_LENGTHS
    data, off = E.pack(E.mixed_messages())
    assert sorted(b - a for a, b in zip(off, off[1:])) == sorted(E.MIXED_LENGTHS)
    assert sum(1 for o in off[:-1] if o % 2) >= 8 and sum(1 for o in off[:-1] if o % 4) >= 12
    assert len(E.padded_messages()) == E.PAD_TO
    assert [len(d) for d, _ in E.dst_cases()] == E.DST_LENGTHS


@pytest.fixture(scope="module")
def C():
    subprocess.check_call(["make", "-C", os.path.join(E.ROOT, "oracle"), "-s"])
    L = ctypes.CDLL(os.path.join(E.ROOT, "oracle", "_build", "libbls_ref.so"))
    L.ref_hash_to_g2.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    return L


def c_hash(C, msg, dst):
    out = ctypes.create_string_buffer(192)
    C.ref_hash_to_g2(msg, len(msg), dst, len(dst), out)
    return out.raw


def test_c_oracle_equals_python_oracle_at_these_lengths(C):
    """A sample on the Python side (0.3 s per hash): the messages on b_0's block boundaries under
    the POP DST, the longest message, and the shortest, longest and boundary DSTs."""
    msgs = {len(m): m for m in E.mixed_messages()}
    sample = [(msgs[n], O.DST_POP) for n in (0, 8, 9, 73, 137, 1000)]
    for dst, ms in E.dst_cases():
        if len(dst) in (0, 22, 150, 255):
            sample.append((ms[2], dst))
    for m, d in sample:
        assert c_hash(C, m, d) == E.g2_b(O.hash_to_g2(m, d)), (len(m), len(d))
