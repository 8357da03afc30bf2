"""CPU: the per-piece and per-set steps of the span-set keys (grandine_amd/csrc/gbls_spans.h, the
text k_g1_span_pieces and k_g1_span_keys compile for gfx950) built for the host
(tests/native/spans_harness.cpp) and checked against the pure-Python oracle: committee_bits to
pieces, the window of a bit row at every bit residue, both SSZ encodings and every malformed string
over M, the direction per committee, and pieces and fold in lane order and in row order.  The
oracle's key of a set is (sum of the participants' scalars) G.  The same harness runs once as a
stand-alone program under AddressSanitizer and UBSan."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "spans_harness.cpp")
SO = os.path.join(ROOT, "tests", "native", "_build", "libspans_harness.so")
MONT = 1 << 384
SUCCESS, BAD_ENCODING, AGGR_TYPE_MISMATCH = 0, 1, 4
SP_BAD_INDEX, SP_BAD_SLOT, SP_EMPTY = 1, 2, 4
FORMS = [(1, 1), (1, 16), (16, 1), (16, 16)]  # lanes per piece, lanes per set's fold
SIZES = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]
NTAB = 2 * len(SIZES)  # slot s holds SIZES[s % 13] members
G1 = O.sk_to_pk(1)
BASE = 0x1234567  # the member at global position g has scalar BASE + g


@pytest.fixture(scope="module")
def H():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    u32, vp, cp = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p
    L.h_span_window.argtypes = [vp, u32, u32, u32]
    L.h_span_window.restype = u32
    L.h_span_pieces.argtypes = [u32, cp, u32, vp, vp, vp]
    L.h_span_pieces.restype = u32
    L.h_span_key.argtypes = [u32, cp, u32, cp, vp, cp, cp, vp, u32, u32, u32, cp, vp]
    L.h_span_plain.argtypes = [cp, u32, cp]
    return L


def fp_b(x):
    return (x * MONT % O.P).to_bytes(48, "little")


def g1_b(p):
    return bytes(96) if p is None else fp_b(p[0]) + fp_b(p[1])


def scalar_key(gs):
    gs = list(gs)
    return g1_b(O.g1_mul(G1, sum(BASE + g for g in gs) % O.R)) if gs else bytes(96)


class Table:
    """NTAB slots over consecutive members; the cached sums and the keys as the harness's bytes."""

    def __init__(self):
        self.off = [0]
        for s in range(NTAB):
            self.off.append(self.off[-1] + SIZES[s % len(SIZES)])
        keys, p = [], O.g1_mul(G1, BASE)
        for _ in range(self.off[-1]):
            keys.append(g1_b(p))
            p = O.g1_add(p, G1)
        self.keys = b"".join(keys)
        self.C = b"".join(scalar_key(range(self.off[s], self.off[s + 1])) for s in range(NTAB))
        self.keeps = bytes([1]) * NTAB

    def members(self, s):
        return list(range(self.off[s], self.off[s + 1]))


@pytest.fixture(scope="module")
def T():
    return Table()


def mask_bytes(named):
    out = bytearray(8)
    for c in named:
        out[c >> 3] |= 1 << (c & 7)
    return bytes(out)


def encode(bits, bitlist):
    m = len(bits)
    out = bytearray(m // 8 + 1 if bitlist else (m + 7) // 8)
    for j, b in enumerate(bits):
        out[j >> 3] |= b << (j & 7)
    if bitlist:
        out[m >> 3] |= 1 << (m & 7)
    return bytes(out)


def committee_bits(m, kind, rng):
    """One committee's bits in one of the three directions (and their edges); never empty."""
    if kind == "full":  # the cached sum unchanged
        return [1] * m
    if kind == "one-clear":  # subtracts its absentee (m = 1: nobody to spare, full)
        return [int(j != m // 3 or m == 1) for j in range(m)]
    if kind == "one-set":  # sums its participant
        return [int(j == (2 * m) // 3) for j in range(m)]
    if kind == "half":  # the tie: participants
        chosen = set(rng.sample(range(m), max(1, m // 2)))
        return [int(j in chosen) for j in range(m)]
    bits = [int(rng.random() < (0.85 if kind == "most" else 0.25)) for _ in range(m)]
    bits[rng.randrange(m)] = 1
    return bits


KINDS = ["full", "one-clear", "one-set", "half", "most", "few"]


def run(H, T, com, named, field, forms=(1, 1), offset=0, table=None):
    """The string placed at byte `offset` of a buffer that ends with it."""
    buf = ctypes.create_string_buffer(bytes(offset) + field, offset + len(field) or 1)
    out = ctypes.create_string_buffer(96)
    info = (ctypes.c_uint32 * (2 + 4 * 64))()
    C, keeps, keys = table or (T.C, T.keeps, T.keys)
    off = (ctypes.c_uint32 * (NTAB + 1))(*T.off)
    st = H.h_span_key(com, mask_bytes(named) if not isinstance(named, bytes) else named, NTAB, C, off, keeps, keys,
                      ctypes.addressof(buf) + offset, len(field), forms[0], forms[1], out, info)
    k = info[0]
    return st, out.raw, (k, info[1], [tuple(info[2 + 4 * q:6 + 4 * q]) for q in range(k)])


def residue_masks():
    """For each bit residue r of a row word, the first ascending choice of committees (base 0) whose
    member counts sum to r mod 32, followed by one more committee: its window starts at residue r."""
    found = {}
    for k in range(1, 6):
        for sub in itertools.combinations(range(NTAB - 1), k):
            r = sum(SIZES[c % len(SIZES)] for c in sub) % 32
            found.setdefault(r, list(sub) + [sub[-1] + 1])
        if len(found) == 32:
            break
    return found


def test_window_extraction_at_every_bit_residue(H, T):
    """Windows over the concatenated committees: every word of every committee's window equals the
    bits of the string at that offset, zero past the string's end; the windows tested start at
    every one of the 32 bit residues, in both encodings."""
    rng = random.Random("windows")
    masks = residue_masks()
    assert sorted(masks) == list(range(32))
    residues = set()
    for r, named in sorted(masks.items()):
        bits = [rng.getrandbits(1) for c in named for _ in T.members(c)]
        for bitlist in (False, True):
            field = encode(bits, bitlist)
            value = int.from_bytes(field, "little")
            at = 0
            for c in named:
                m = len(T.members(c))
                for offset in (0, 1, 3):
                    buf = ctypes.create_string_buffer(bytes(offset) + field, offset + len(field))
                    for w in range((m + 31) // 32 + 1):  # one word further: past the string reads zero
                        got = H.h_span_window(ctypes.addressof(buf) + offset, len(field), at, w)
                        assert got == (value >> (at + 32 * w)) & 0xFFFFFFFF, (named, bitlist, c, w)
                residues.add(at % 32)
                at += m
        assert at % 32 == (r + len(T.members(named[-1]))) % 32
    assert residues == set(range(32))  # the coverage the test claims
    # far past the string: zero, whatever the offset
    assert H.h_span_window(ctypes.c_char_p(b"\xff" * 5), 5, 40, 0) == 0
    assert H.h_span_window(ctypes.c_char_p(b"\xff" * 5), 5, 33, 0) == 0x7F
    assert H.h_span_window(ctypes.c_char_p(b"\xff" * 5), 5, 4096, 3) == 0


@pytest.mark.parametrize("forms", FORMS)
def test_keys_directions_and_counts(H, T, forms):
    """Per committee the direction and the keys added, mixed directions in one set, the key equal
    to the oracle's, with pieces and fold in lane order and in row order."""
    rng = random.Random("keys")
    masks = [named for _, named in sorted(residue_masks().items())][::4]
    masks += [[0], [13], [25], list(range(13)), list(range(0, 13, 2))]
    mixed = 0
    for n, named in enumerate(masks):
        com = n % 3 if named[-1] + 2 < NTAB else 0
        kinds = [KINDS[(n + i) % len(KINDS)] for i in range(len(named))]
        per = [committee_bits(len(T.members(com + c)), kind, rng) for c, kind in zip(named, kinds)]
        part = [g for c, b in zip(named, per) for g, x in zip(T.members(com + c), b) if x]
        want = scalar_key(part)
        flat = [x for b in per for x in b]
        for bitlist in (False, True):
            field = encode(flat, bitlist)
            for offset in (0, 3):
                st, key, (k, M, pieces) = run(H, T, com, named, field, forms, offset)
                assert (st, key) == (SUCCESS, want), (named, kinds, bitlist, offset)
                assert (k, M) == (len(named), len(flat))
                for b, (p, sub, adds, flags) in zip(per, pieces):
                    m = len(b)
                    assert (p, sub, flags) == (sum(b), int(m - sum(b) < sum(b)), 0)
                    assert adds == (m - p if sub else p)  # a full committee adds nothing: its cached sum
                dirs = {(sub, adds == 0) for _, sub, adds, _ in pieces}
                mixed += len(dirs) >= 3
    assert mixed  # one set took C - S, S and C in its committees


def malformed(M, bits):
    v, l = encode(bits, False), encode(bits, True)
    out = {"vector one byte long": v + b"\0", "list one byte long": l + b"\0", "vector one byte short": v[:-1],
           "empty": b""}
    if M % 8:
        out["list one byte short"] = l[:-1]
    else:
        out["missing delimiter"] = l[:-1] + bytes([l[-1] & 0xFE])
    for name, s in (("vector", v), ("list", l)):
        top = 8 * len(s) - 1
        for pos in (M + 1, top):
            if M < pos <= top:
                t = bytearray(s)
                t[pos >> 3] |= 1 << (pos & 7)
                out["%s with a stray bit at %d" % (name, pos)] = bytes(t)
    return out


@pytest.mark.parametrize("forms", FORMS)
def test_malformed_strings_over_M(H, T, forms):
    rng = random.Random("malformed")
    seen = set()
    for named in ([0, 1], [1, 2, 3], [2, 5, 8, 9], [7, 8], list(range(13))):  # M = 8, 24, 59, 63, 361
        flat = [x for c in named for x in committee_bits(len(T.members(c)), "most", rng)]
        cases = malformed(len(flat), flat)
        seen |= {tag.split(" at ")[0] for tag in cases}
        for tag, field in cases.items():
            for offset in (0, 1):
                st, key, _ = run(H, T, 0, named, field, forms, offset)
                assert (st, key) == (BAD_ENCODING, bytes(96)), (named, tag)
    assert {"vector one byte long", "vector one byte short", "list one byte short", "missing delimiter",
            "list with a stray bit", "vector with a stray bit"} <= seen


@pytest.mark.parametrize("forms", FORMS)
def test_rejections(H, T, forms):
    rng = random.Random("rejections")
    named = [1, 2, 4]
    per = [committee_bits(len(T.members(c)), "most", rng) for c in named]
    good = encode([x for b in per for x in b], True)
    assert run(H, T, 0, named, good, forms)[0] == SUCCESS
    # an empty committee among non-empty ones, first, middle and last
    for i in range(3):
        holed = [b if j != i else [0] * len(b) for j, b in enumerate(per)]
        st, key, (_, _, pieces) = run(H, T, 0, named, encode([x for b in holed for x in b], True), forms)
        assert (st, key) == (BAD_ENCODING, bytes(96))
        assert [bool(f & SP_EMPTY) for _, _, _, f in pieces] == [j == i for j in range(3)]
    # all-zero committee_bits
    assert run(H, T, 0, [], b"", forms)[:2] == (BAD_ENCODING, bytes(96))
    assert run(H, T, 0, [], b"\x01", forms)[:2] == (BAD_ENCODING, bytes(96))
    # a named slot past the table; com + c wrapping 32 bits must not name slot 0 or 1
    st, key, (_, _, pieces) = run(H, T, NTAB - 3, named, good, forms)
    assert (st, key) == (BAD_ENCODING, bytes(96)) and pieces[2][3] & SP_BAD_SLOT
    for com, c in ((0xFFFFFFFF - 62, 63), (0xFFFFFFF0, 16), (0xFFFFFFF0, 17), (0xFFFFFFFE, 1)):
        one = encode([1] * len(T.members((com + c) & 0xFFFFFFFF)), True) if (com + c) & 0xFFFFFFFF < NTAB else b"\x03"
        st, key, (k, M, pieces) = run(H, T, com, [c], one, forms)
        assert (st, key, k, M) == (BAD_ENCODING, bytes(96), 1, 0), (com, c)
        assert pieces[0][3] & SP_BAD_SLOT
    # a slot that keeps no members; an invalid (all-zero) cached sum, in either direction
    keeps = bytearray(T.keeps)
    keeps[2] = 0
    assert run(H, T, 0, named, good, forms, table=(T.C, bytes(keeps), T.keys))[:2] == (BAD_ENCODING, bytes(96))
    C = bytearray(T.C)
    C[96 * 4:96 * 5] = bytes(96)
    for kind in ("full", "one-clear", "one-set"):
        f = encode([x for c in named for x in committee_bits(len(T.members(c)), kind, rng)], False)
        assert run(H, T, 0, named, f, forms, table=(bytes(C), T.keeps, T.keys))[:2] == (BAD_ENCODING, bytes(96))
    # an invalid member key among those added rejects; not among them, it does not
    keys = bytearray(T.keys)
    g = T.members(2)[len(T.members(2)) // 3]  # the one absentee of committee 2 under "one-clear"
    keys[96 * g:96 * g + 96] = bytes(96)
    f = encode([x for c in named for x in committee_bits(len(T.members(c)), "one-clear", rng)], True)
    assert run(H, T, 0, named, f, forms, table=(T.C, T.keeps, bytes(keys)))[:2] == (BAD_ENCODING, bytes(96))
    f = encode([x for c in named for x in committee_bits(len(T.members(c)), "full", rng)], True)
    assert run(H, T, 0, named, f, forms, table=(T.C, T.keeps, bytes(keys)))[0] == SUCCESS


def test_mask_to_pieces(H):
    counts = (ctypes.c_uint32 * 8)(5, 0, 9, 33, 64, 1, 0, 7)
    out = (ctypes.c_uint32 * 256)()
    M = ctypes.c_uint32()

    def pieces(com, named):
        k = H.h_span_pieces(com, mask_bytes(named), 8, counts, out, ctypes.byref(M))
        return [tuple(out[4 * i:4 * i + 4]) for i in range(k)], M.value

    assert pieces(0, [0, 2, 3]) == ([(0, 5, 0, 1), (2, 9, 5, 1), (3, 33, 14, 1)], 47)
    assert pieces(2, [0, 1, 5]) == ([(2, 9, 0, 1), (3, 33, 9, 1), (7, 7, 42, 1)], 49)
    assert pieces(0, [1, 2]) == ([(1, 0, 0, 0), (2, 9, 0, 1)], 9)        # slot 1 keeps none
    assert pieces(4, [0, 1, 4]) == ([(4, 64, 0, 1), (5, 1, 64, 1), (8, 0, 65, 0)], 65)  # slot 8: past the table
    assert pieces(0, []) == ([], 0)
    got, m = pieces(0xFFFFFFFF, [0, 1, 5])  # 2^32 - 1 is no slot, and + 1, + 5 do not wrap to slots 0 and 4
    assert [g[1:] for g in got] == [(0, 0, 0)] * 3 and m == 0
    assert all(g[0] >= 0xFFFFFFFE for g in got)
    got, m = pieces(0, list(range(64)))
    assert len(got) == 64 and m == sum(counts) and [g[0] for g in got] == list(range(64))


def test_degenerate_folds(H, T):
    """Twin committees (the same members in two slots) with the same bits double; two committees
    whose selected members are opposite cancel to infinity: all-zero with SUCCESS."""
    X = O.g1_mul(G1, 77)
    Y = O.g1_mul(G1, 5)
    off = (ctypes.c_uint32 * 4)(0, 2, 4, 6)
    keys = g1_b(X) + g1_b(Y) + g1_b(X) + g1_b(Y) + g1_b(O.g1_neg(X)) + g1_b(Y)
    C = g1_b(O.g1_add(X, Y)) * 2 + g1_b(O.g1_add(O.g1_neg(X), Y))
    out = ctypes.create_string_buffer(96)
    info = (ctypes.c_uint32 * (2 + 4 * 64))()
    for forms in FORMS:
        for bits, want in (([1, 0, 1, 0], O.g1_add(X, X)), ([1, 1, 1, 1], O.g1_add(O.g1_add(X, Y), O.g1_add(X, Y)))):
            f = encode(bits, True)
            st = H.h_span_key(0, mask_bytes([0, 1]), 3, C, off, b"\1\1\1", keys, ctypes.c_char_p(f), len(f), forms[0],
                              forms[1], out, info)
            assert (st, out.raw) == (SUCCESS, g1_b(want)), (forms, bits)
        f = encode([1, 0, 1, 0], False)  # slots 1 and 2: X and -X
        st = H.h_span_key(1, mask_bytes([0, 1]), 3, C, off, b"\1\1\1", keys, ctypes.c_char_p(f), len(f), forms[0],
                          forms[1], out, info)
        assert (st, out.raw) == (SUCCESS, bytes(96)), forms


def test_plain_sets(H, T):
    out = ctypes.create_string_buffer(96)
    assert H.h_span_plain(T.keys, 0, out) == AGGR_TYPE_MISMATCH and out.raw == bytes(96)
    assert H.h_span_plain(T.keys, 5, out) == SUCCESS and out.raw == scalar_key(range(5))
    assert H.h_span_plain(T.keys[:96] + bytes(96) + T.keys[192:384], 4, out) == BAD_ENCODING and out.raw == bytes(96)


def test_harness_under_asan_ubsan(tmp_path):
    """The harness as a stand-alone program (its own main) under ASan/UBSan, run once."""
    exe = str(tmp_path / "spans_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-DSPANS_MAIN",
                           "-I/opt/rocm/include", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    log = out.stdout[-3000:] + out.stderr[-3000:]
    assert out.returncode == 0, log
    assert "spans_harness: OK" in out.stdout, log
