"""Inputs and expected outputs shared by tests/test_edges_fixtures.py (CPU), tests/test_gpu_edges.py
and its child tests/gpu_edges_child.py: the encodings an untrusted peer can send (tests/golden/
small_order.json, decode_edges.json, and the older g1_decode.json / g2_decode.json), laid out as
launches, and the message / DST lengths at which expand_message_xmd changes its block counts.

Every expected value here comes from oracle/bls12_381.py (Python integers).  Nothing imports the
engine."""
import hashlib
import json
import os

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MONT = 1 << 384
RINV = pow(MONT, -1, O.P)
ROW_MAX = 2048  # launch_g2_decompress: up to this many signatures take the 16-lane row kernel


def gold(name):
    with open(os.path.join(GOLD, name + ".json")) as fh:
        return json.load(fh)


# ---------------------------------------------------------------- the engine's point bytes
def fp_b(x):
    return (x * MONT % O.P).to_bytes(48, "little")


def g1_b(p):
    return bytes(96) if p is None else fp_b(p[0]) + fp_b(p[1])


def g2_b(p):
    return bytes(192) if p is None else fp_b(p[0][0]) + fp_b(p[0][1]) + fp_b(p[1][0]) + fp_b(p[1][1])


def g2_of(b):
    v = [int.from_bytes(b[48 * k:48 * k + 48], "little") * RINV % O.P for k in range(4)]
    return None if not any(b) else ((v[0], v[1]), (v[2], v[3]))


def g1_of(b):
    v = [int.from_bytes(b[48 * k:48 * k + 48], "little") * RINV % O.P for k in range(2)]
    return None if not any(b) else (v[0], v[1])


def f2_of_hex(h):
    return (int(h[0], 16), int(h[1], 16))


def g2_of_rec(rec):
    return (f2_of_hex(rec["x"]), f2_of_hex(rec["y"]))


def g1_of_rec(rec):
    return (int(rec["x"], 16), int(rec["y"], 16))


# ---------------------------------------------------------------- G2 decoding
def g2_edge_encodings():
    """[(label, 96 bytes)]: every special or invalid G2 encoding of the fixtures."""
    e = gold("decode_edges")
    out = [("root %s #%d" % (c["class"], i), bytes.fromhex(c["in"])) for i, c in enumerate(e["g2_roots"])]
    out += [("flag: " + c["note"], bytes.fromhex(c["in"])) for c in e["g2_flags"]]
    for c in gold("small_order")["e2"]:
        for k in ("T", "negT", "T_plus_gen"):
            out.append(("order %d %s" % (c["order"], k), bytes.fromhex(c[k]["enc"])))
    out += [("g2_decode.json #%d" % i, bytes.fromhex(c["in"])) for i, c in enumerate(gold("g2_decode")["cases"])]
    return out


def g2_expect(enc):
    """(status, the 192 output bytes): a failed case and infinity are all-zero."""
    st, pt = O.g2_decompress(enc)
    return st, g2_b(pt if st == O.SUCCESS else None)


def g2_chain(n, k=0x5EED1234):
    """n points of G2, P_i = [k]G + [i]G: valid signatures as far as decoding and membership go."""
    p = O.g2_mul(O.G2_GEN, k)
    out = []
    for _ in range(n):
        out.append(p)
        p = O.g2_add(p, O.G2_GEN)
    return out


LANE_N = 2150  # 33 full waves and one of 38 lanes; > ROW_MAX, so the one-lane-per-point kernel


def g2_lane_launch():
    """[(label, enc)] of LANE_N signatures: valid ones, with every edge case once from lane 30 on
    (the first wave and across its 64-lane boundary, further boundaries behind it) and once more
    at the very end (the partly filled last wave and the full one before it)."""
    edges = g2_edge_encodings()
    ne = len(edges)
    assert 64 - 30 < ne < 38 + 64 and 30 + ne < LANE_N - ne
    fill = [("valid #%d" % i, O.g2_compress(p)) for i, p in enumerate(g2_chain(LANE_N - 2 * ne))]
    out = fill[:30] + edges + fill[30:] + edges
    assert len(out) == LANE_N and LANE_N % 64 == 38 and LANE_N > ROW_MAX
    return out


# ---------------------------------------------------------------- G1 decoding
def g1_edge_encodings():
    e = gold("decode_edges")
    out = [("flag: " + c["note"], bytes.fromhex(c["in"])) for c in e["g1_flags"]]
    for c in gold("small_order")["e1"]:
        for k in ("T", "T_plus_gen"):
            out.append(("order %d %s" % (c["order"], k), bytes.fromhex(c[k]["enc"])))
    out += [("g1_decode.json #%d" % i, bytes.fromhex(c["in"])) for i, c in enumerate(gold("g1_decode")["cases"])]
    return out


def g1_expect(enc, validate):
    """(status, the 96 output bytes) of gbls_g1_decompress: PublicKey::try_from with validate."""
    st, pt = O.public_key_from_bytes(enc) if validate else O.g1_decompress(enc)
    return st, g1_b(pt if st == O.SUCCESS else None)


G1_RAGGED_N = 64 * 3 + 29


def g1_ragged_launch():
    """([(label, enc)], {index: point} of the valid fillers): G1_RAGGED_N keys, the edge cases
    split over the first wave's end and the partly filled last block.  The fillers are [k + i]G,
    in G1 by construction, so the caller need not run the textbook [r]P on them."""
    edges = g1_edge_encodings()
    ne = len(edges)
    half = ne // 2
    pts, p = [], O.g1_mul(O.G1_GEN, 0xC0FFEE)
    for _ in range(G1_RAGGED_N - ne):
        pts.append(p)
        p = O.g1_add(p, O.G1_GEN)
    fill = [("valid #%d" % i, O.g1_compress(q)) for i, q in enumerate(pts)]
    cut = 64 - half // 2
    out = fill[:cut] + edges[:half] + fill[cut:] + edges[half:]
    assert len(out) == G1_RAGGED_N and G1_RAGGED_N % 64 == 29 and ne - half > 3
    known = {i: pts[int(lab.split("#")[1])] for i, (lab, _) in enumerate(out) if lab.startswith("valid #")}
    return out, known


# ---------------------------------------------------------------- G2 membership
def g2_membership_cases():
    """[(label, point or None, expected status of gbls_g2_validate)]: every small-order E2 point,
    its negation and its sum with the generator, the decode_edges points (on the curve, outside
    G2), infinity and valid signatures, interleaved so that each wave mixes verdicts."""
    bad = []
    for c in gold("small_order")["e2"]:
        for k in ("T", "negT", "T_plus_gen"):
            bad.append(("order %d %s" % (c["order"], k), g2_of_rec(c[k]), O.POINT_NOT_IN_GROUP))
    e = gold("decode_edges")
    for i, c in enumerate(e["g2_roots"]):
        bad.append(("root %s #%d" % (c["class"], i), g2_of_rec(c),
                    O.SUCCESS if c["in_group"] else O.POINT_NOT_IN_GROUP))
    for c in e["g2_flags"]:
        if c["status"] == O.SUCCESS and c["x"] is not None:
            bad.append(("flag: " + c["note"], g2_of_rec(c), O.SUCCESS if c["in_group"] else O.POINT_NOT_IN_GROUP))
    good = [("valid #%d" % i, p, O.SUCCESS) for i, p in enumerate(g2_chain(len(bad) + 8, k=0xABCDEF))]
    out = []
    for i, g in enumerate(good):
        out.append(g)
        if i < len(bad):
            out.append(bad[i])
        if i % 9 == 4:
            out.append(("infinity", None, O.SUCCESS))
    assert len(out) > 64
    return out


# ---------------------------------------------------------------- hash_to_G2 lengths
MIXED_LENGTHS = [0, 1, 7, 8, 9, 31, 32, 33, 55, 56, 63, 64, 65, 71, 72, 73, 119, 120, 136, 137, 200, 1000]
DST_LENGTHS = [0, 1, 21, 22, 43, 85, 86, 149, 150, 213, 214, 254, 255]
PAD_TO = 1100  # > kW4Max = 1024: row clearing by default, the lane chains with GBLS_LANE_MIN=1025


def b0_blocks(mlen, dlen):
    """SHA-256 blocks of b_0's input after Z_pad: msg || 2 || 1 || DST || 1, then 0x80 and 8 bytes."""
    return (mlen + dlen + 4 + 9 + 63) // 64


def bi_blocks(dlen):
    return (34 + dlen + 9 + 63) // 64


def stream(tag, n):
    out = b""
    i = 0
    while len(out) < n:
        out += hashlib.sha256(b"%s/%d" % (tag, i)).digest()
        i += 1
    return out[:n]


def mixed_messages():
    """The MIXED_LENGTHS messages in an order in which neighbouring lanes differ in b_0's block
    count, the empty message between two others."""
    lens = sorted(MIXED_LENGTHS, key=lambda m: (b0_blocks(m, 43), m))
    lo, hi = lens[:len(lens) // 2], lens[len(lens) // 2:]
    order = [x for pair in zip(hi, lo) for x in pair]
    assert sorted(order) == sorted(MIXED_LENGTHS) and 0 < order.index(0) < len(order) - 1
    assert all(b0_blocks(a, 43) != b0_blocks(b, 43) for a, b in zip(order, order[1:]))
    return [stream(b"mixed%d" % m, m) for m in order]


def padded_messages():
    msgs = mixed_messages()
    return msgs + [hashlib.sha256(b"pad%d" % i).digest() for i in range(PAD_TO - len(msgs))]


def pack(msgs):
    """(data, offsets): messages back to back, as gbls_hash_to_g2 takes them."""
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    return b"".join(msgs), off


def dst_cases():
    """[(dst, [messages])]: per DST length a few messages, among them the two lengths on either
    side of b_0's first block boundary for that DST."""
    out = []
    for d in DST_LENGTHS:
        dst = stream(b"dst%d" % d, d)
        edge = next(64 * k - 13 - d for k in range(1, 8) if 64 * k - 13 - d >= 0)
        lens = sorted({0, 32, edge, edge + 1, edge + 64, edge + 65})
        assert b0_blocks(edge, d) + 1 == b0_blocks(edge + 1, d)
        out.append((dst, [stream(b"d%dm%d" % (d, m), m) for m in lens]))
    return out
