"""The layer an untrusted peer reaches, bit by bit on the GPU: point decoding in both kernel forms,
the subgroup checks on points that force their exceptional branches, and hash_to_G2 at the message
and DST lengths where expand_message_xmd changes its block counts.

Expected values come from oracle/bls12_381.py (Python integers) and, for hash_to_G2 points, from
the C oracle (oracle/bls_ref.c); never from the engine.  Everything is exact: statuses, verdicts
and every output byte.  Each test asserts how many cases it compared.

Inputs: tests/golden/small_order.json (points of order 13, 23, 2713, 11953 on E2 and 11, 10177,
859267 on E1), tests/golden/decode_edges.json (roots of y^2 that lie in Fp or in u Fp, flag and
range edges), laid out as launches by tests/edges_cases.py.  The non-default kernel forms run in
a child process (tests/gpu_edges_child.py) that sets their knobs."""
import ctypes
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

from oracle import bls12_381 as O

import edges_cases as E
import gpu_edges_child as CH

pytestmark = pytest.mark.gpu
ROOT = E.ROOT


@pytest.fixture(scope="module")
def G():
    from grandine_amd import _lib as G
    return G


@pytest.fixture(scope="module")
def L(G):
    return G.lib()


@pytest.fixture(scope="module")
def C():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
    return CH.ref_lib()


def child(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_edges_child.py"), *args],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def ints(a, n):
    return [a[i] for i in range(n)]


# ------------------------------------------------------------------ decoding
def g2_decompress(G, L, encs):
    n = len(encs)
    out = ctypes.create_string_buffer(b"\xee" * (192 * n), 192 * n)
    st = G.i32_array(n)
    for i in range(n):
        st[i] = 77
    G.check(L.gbls_g2_decompress(G.buf(b"".join(encs)), n, out, st), "g2 decompress")
    return ints(st, n), [out.raw[192 * i:192 * i + 192] for i in range(n)]


def compare_decoded(labels, got_st, got_pts, want):
    bad = [(lab, s, w[0]) for lab, s, p, w in zip(labels, got_st, got_pts, want) if (s, p) != w]
    assert not bad, "%d of %d differ from the oracle, first %s" % (len(bad), len(want), bad[:6])
    assert all(p == bytes(len(p)) for s, p in zip(got_st, got_pts) if s != O.SUCCESS)  # failed: all-zero
    return len(want)


def test_g2_decompress_row_and_lane_forms(G, L):
    """The same special and invalid encodings through k_g2_decompress_row (one short launch) and
    through k_g2_decompress (scattered among valid signatures in a launch of 2150: first wave,
    across 64-lane boundaries, the partly filled last wave): status and all 192 bytes equal the
    oracle's, failed cases all-zero, the two forms byte for byte the same, and gbls_g2_compress of
    every decoded point returns its input."""
    edges = E.g2_edge_encodings()
    ne = len(edges)
    assert ne <= E.ROW_MAX
    want_e = [E.g2_expect(enc) for _, enc in edges]
    row_st, row_pts = g2_decompress(G, L, [enc for _, enc in edges])
    assert compare_decoded([lab for lab, _ in edges], row_st, row_pts, want_e) == ne
    lane = E.g2_lane_launch()
    assert len(lane) == E.LANE_N > E.ROW_MAX
    cache = dict(zip((enc for _, enc in edges), want_e))
    want_l = [cache[enc] if enc in cache else E.g2_expect(enc) for _, enc in lane]
    lane_st, lane_pts = g2_decompress(G, L, [enc for _, enc in lane])
    assert compare_decoded([lab for lab, _ in lane], lane_st, lane_pts, want_l) == E.LANE_N
    # the two forms on the same encoding, wherever it sits in the long launch
    by_enc = {enc: (row_st[i], row_pts[i]) for i, (_, enc) in enumerate(edges)}
    seen = 0
    for i, (lab, enc) in enumerate(lane):
        if enc in by_enc and not lab.startswith("valid #"):
            assert (lane_st[i], lane_pts[i]) == by_enc[enc], (i, lab)
            seen += 1
    assert seen == 2 * ne
    classes = {s: sum(1 for x in row_st if x == s) for s in set(row_st)}
    assert set(classes) == {O.SUCCESS, O.BAD_ENCODING, O.POINT_NOT_ON_CURVE}
    # re-compression
    ok = [i for i in range(E.LANE_N) if lane_st[i] == O.SUCCESS]
    enc = ctypes.create_string_buffer(96 * len(ok))
    G.check(L.gbls_g2_compress(G.buf(b"".join(lane_pts[i] for i in ok)), len(ok), enc), "g2 compress")
    back = [enc.raw[96 * j:96 * j + 96] for j in range(len(ok))]
    assert back == [lane[i][1] for i in ok] and len(ok) >= E.LANE_N - 2 * ne


def g1_decompress(G, L, encs, validate):
    n = len(encs)
    out = ctypes.create_string_buffer(b"\xee" * (96 * n), 96 * n)
    st = G.i32_array(n)
    for i in range(n):
        st[i] = 77
    G.check(L.gbls_g1_decompress(G.buf(b"".join(encs)), n, validate, out, st), "g1 decompress")
    return ints(st, n), [out.raw[96 * i:96 * i + 96] for i in range(n)]


@pytest.fixture(scope="module")
def g1_want():
    """{validate: {encoding: (status, bytes)}} of the G1 edge encodings (textbook [r]P: once)."""
    return {v: {enc: E.g1_expect(enc, v) for _, enc in E.g1_edge_encodings()} for v in (0, 1)}


@pytest.mark.parametrize("validate", [0, 1])
def test_g1_decompress_edges(G, L, g1_want, validate):
    """gbls_g1_decompress (one form) on a short launch of the range and flag edges and the points
    of order 11, 10177 and 859267 (NOT_IN_GROUP under validate), and on a launch with a ragged last
    block; gbls_g1_compress of the decoded points returns the inputs."""
    edges = E.g1_edge_encodings()
    want = [g1_want[validate][enc] for _, enc in edges]
    st, pts = g1_decompress(G, L, [enc for _, enc in edges], validate)
    assert compare_decoded([lab for lab, _ in edges], st, pts, want) == len(edges)
    if validate:
        small = [i for i, (lab, _) in enumerate(edges) if lab.startswith("order ")]
        assert len(small) == 6 and all(st[i] == O.POINT_NOT_IN_GROUP for i in small)
    launch, known = E.g1_ragged_launch()
    want = [(O.SUCCESS, E.g1_b(known[i])) if i in known else g1_want[validate][enc]
            for i, (_, enc) in enumerate(launch)]
    st, pts = g1_decompress(G, L, [enc for _, enc in launch], validate)
    assert compare_decoded([lab for lab, _ in launch], st, pts, want) == E.G1_RAGGED_N
    ok = [i for i in range(len(launch)) if st[i] == O.SUCCESS]
    enc = ctypes.create_string_buffer(48 * len(ok))
    G.check(L.gbls_g1_compress(G.buf(b"".join(pts[i] for i in ok)), len(ok), enc), "g1 compress")
    assert [enc.raw[48 * j:48 * j + 48] for j in range(len(ok))] == [launch[i][1] for i in ok]
    assert len(ok) >= len(known)


def test_small_order_key_in_a_local_key_table(G, L, C):
    """gbls_verify_each_local with a point of order 11 as the middle key of its local table: that
    key's status is NOT_IN_GROUP and its set fails; its neighbours verify."""
    t = bytes.fromhex(E.gold("small_order")["e1"][0]["T"]["enc"])
    sks = [(0x51 + i).to_bytes(32, "big") for i in range(3)]
    msgs = [bytes([0xA0 + i]) * 32 for i in range(3)]
    table = [O.g1_compress(E.g1_of(CH.ref_pk(C, sk))) for sk in sks]
    table[1] = t
    sigs = [O.g2_compress(E.g2_of(CH.ref_sign(C, sk, m))) for sk, m in zip(sks, msgs)]
    n = 3
    st, kst, v, pst = (G.i32_array(n) for _ in range(4))
    for a in (st, kst, v, pst):
        for i in range(n):
            a[i] = 77
    rc = L.gbls_verify_each_local(G.buf(b"".join(msgs)), G.buf(b"".join(sigs)), G.u32_array([G.LOCAL_KEYS] * n),
                                  G.buf(bytes(8 * n)), G.buf(b""), G.u32_array([0] * (n + 1)), G.u32_array([0, 1, 2]),
                                  G.u32_array([0, 1, 2, 3]), G.buf(b"".join(table)), n, n, st, kst, v, pst)
    assert rc == 0 and L.gbls_last_error() == 0
    assert ints(pst, n) == [O.SUCCESS, O.POINT_NOT_IN_GROUP, O.SUCCESS]
    assert ints(st, n) == [O.SUCCESS] * 3
    assert ints(kst, n) == [O.SUCCESS, O.BAD_ENCODING, O.SUCCESS]
    assert [x == O.SUCCESS for x in ints(v, n)] == [True, False, True]


# ------------------------------------------------------------------ membership and verdicts
@pytest.mark.parametrize("knob", ["GBLS_LANE_R28=1", "GBLS_LANE_R28=0"])
def test_membership_and_verdicts(C, knob):
    """gbls_g2_validate through k_g2_check28 (radix 2^28, the default) and k_g2_check (engine form)
    on every small-order E2 point, its negation and its sum with the generator (for order 13 the
    accumulator of the [|x|] chain is the base's negation at the addition of bit 60, |x| >> 60 = 13:
    the sum is infinity and the chain restarts from the base), the decode_edges points, infinity and
    valid signatures; then Signature.verify and fast_aggregate_verify, which decode and check inside
    one submission, on small-order signatures and on signature + T.

    No point of E2(Fp2) reaches the other special cases of this chain: its group order h2 r is
    coprime to (|x| >> i) - 2 at every addition (bits 62, 60, 57, 48, 16: the accumulator never
    equals the base), to |x| >> i except for 13 at bit 60, and to |x| (the result is never infinity);
    tests/test_edges_fixtures.py holds that arithmetic."""
    cases = E.g2_membership_cases()
    res = child(knob, "member", "verdicts")
    assert res["knobs"] == [knob]
    got = res["member"]
    assert len(got) == len(cases)
    bad = [(lab, g, w) for (lab, _, w), g in zip(cases, got) if g != w]
    assert not bad, bad[:8]
    small = [g for (lab, _, _), g in zip(cases, got) if lab.startswith("order ")]
    assert small == [O.POINT_NOT_IN_GROUP] * 12
    assert sum(1 for _, p, _ in cases if p is None) >= 4 and sum(1 for g in got if g == O.SUCCESS) >= len(cases) // 2
    want = CH.verdict_cases(C)
    assert len(want) == 9 and [w[3] for w in want] == [True] + [False] * 8
    assert res["verdicts"] == [[lab, exp, exp] for lab, _, _, exp in want]


# ------------------------------------------------------------------ hash_to_G2
def c_hashes(C, msgs, dst):
    def one(m):
        out = ctypes.create_string_buffer(192)
        C.ref_hash_to_g2(m, len(m), dst, len(dst), out)
        return out.raw
    with ThreadPoolExecutor(8) as ex:  # ctypes releases the GIL
        return list(ex.map(one, msgs))


def gpu_hashes(G, L, msgs, dst, dst_len=None, expect_rc=0):
    data, off = E.pack(msgs)
    n = len(msgs)
    out = ctypes.create_string_buffer(b"\xee" * (192 * n), 192 * n)
    rc = L.gbls_hash_to_g2(G.buf(data), G.u32_array(off), n, None if dst is None else G.buf(dst),
                           len(dst or b"") if dst_len is None else dst_len, out)
    assert rc == expect_rc, (rc, L.gbls_last_error())
    return [out.raw[192 * i:192 * i + 192] for i in range(n)]


def test_hash_to_g2_mixed_lengths_one_launch(G, L, C):
    """22 messages of lengths 0 to 1000 packed back to back (odd offsets, an empty message between
    two others, neighbouring lanes in different block counts) in ONE launch under the POP DST:
    every point equals the C oracle's, a sample the Python oracle's."""
    msgs = E.mixed_messages()
    got = gpu_hashes(G, L, msgs, O.DST_POP)
    want = c_hashes(C, msgs, O.DST_POP)
    bad = [len(m) for m, g, w in zip(msgs, got, want) if g != w]
    assert not bad and len(got) == len(E.MIXED_LENGTHS) == 22, bad
    for n in (9, 137):
        i = [len(m) for m in msgs].index(n)
        assert got[i] == E.g2_b(O.hash_to_g2(msgs[i]))


def test_hash_to_g2_dst_lengths(G, L, C):
    """One call per DST length 0 ... 255 (21/22, 85/86, 149/150, 213/214: the b_i block
    boundaries), messages on either side of b_0's boundary for that DST; 256 is an argument error."""
    compared = 0
    for dst, msgs in E.dst_cases():
        got = gpu_hashes(G, L, msgs, dst)
        want = c_hashes(C, msgs, dst)
        bad = [(len(dst), len(m)) for m, g, w in zip(msgs, got, want) if g != w]
        assert not bad, bad
        compared += len(msgs)
        if len(dst) in (0, 255):
            assert got[2] == E.g2_b(O.hash_to_g2(msgs[2], dst))
    assert compared == sum(len(m) for _, m in E.dst_cases()) >= 4 * len(E.DST_LENGTHS)
    out = gpu_hashes(G, L, [b"abc"], bytes(256), expect_rc=O.VERIFY_FAIL)
    assert L.gbls_last_error() == 102 and out == [b"\xee" * 192]  # GBLS_ERR_ARG, nothing written


def test_hash_to_g2_padded_launch_in_both_clearing_forms(G, L, C, tmp_path):
    """The mixed-length messages padded with 32-byte ones to 1100: row clearing under the defaults,
    the radix-2^28 lane chains with GBLS_LANE_MIN=1025 (child process); identical to each other
    and to the C oracle."""
    msgs = E.padded_messages()
    want = c_hashes(C, msgs, O.DST_POP)
    got = gpu_hashes(G, L, msgs, None)  # dst == NULL: the scheme's own DST
    bad = [i for i in range(len(msgs)) if got[i] != want[i]]
    assert not bad and len(got) == E.PAD_TO, bad[:8]
    path = str(tmp_path / "h2c.bin")
    res = child("GBLS_LANE_MIN=1025", "h2c=" + path)
    raw = open(path, "rb").read()
    assert res["h2c"] == E.PAD_TO and len(raw) == 192 * E.PAD_TO
    lane = [raw[192 * i:192 * i + 192] for i in range(E.PAD_TO)]
    bad = [i for i in range(E.PAD_TO) if lane[i] != want[i]]
    assert not bad and lane == got, bad[:8]
