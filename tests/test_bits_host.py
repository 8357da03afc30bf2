"""CPU: the per-set step of the aggregation-bit keys (grandine_amd/csrc/gbls_bits.h, the text
k_g1_bits_keys compiles for gfx950) built for the host (tests/native/bits_harness.cpp) and checked
against the pure-Python oracle: the repacking of a bit string that starts at any byte, both SSZ
encodings and every malformed string, the direction rule, and the accumulation in lane order and in
row order with the folds.  The oracle's key of a set is (sum of the participants' scalars) G.  The
same harness runs once as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "bits_harness.cpp")
SO = os.path.join(ROOT, "tests", "native", "_build", "libbits_harness.so")
MONT = 1 << 384
SUCCESS, BAD_ENCODING = 0, 1
FORMS = [1, 16]  # lanes per set: the kernel's lane form and its 16-lane row form
SIZES = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 512, 2048]
PATTERNS = ["all", "none", "one-set", "one-clear", "alternating", "half", "half+1", "random-a", "random-b"]
G1 = O.sk_to_pk(1)
BASE = 0x1234567  # member j's scalar is BASE + j


@pytest.fixture(scope="module")
def H():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    L.h_bits_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                             ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)]
    L.h_bits_work.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
    L.h_bits_work.restype = ctypes.c_uint32
    return L


def fp_b(x):
    return (x * MONT % O.P).to_bytes(48, "little")


def g1_b(p):
    return bytes(96) if p is None else fp_b(p[0]) + fp_b(p[1])


@pytest.fixture(scope="module")
def keys():
    """The 2048 members' keys (BASE + j) G, as the harness's bytes; a committee of m is the first m."""
    out, p = [], O.g1_mul(G1, BASE)
    for _ in range(max(SIZES)):
        out.append(g1_b(p))
        p = O.g1_add(p, G1)
    return b"".join(out)


def scalar_key(js):
    js = list(js)
    return g1_b(O.g1_mul(G1, sum(BASE + j for j in js) % O.R)) if js else bytes(96)


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
    if name in ("half", "half+1"):  # exactly half (the tie: participants) and one more (absentees)
        chosen = set(rng.sample(range(m), min(m, m // 2 + (name == "half+1"))))
        return [int(j in chosen) for j in range(m)]
    return [int(rng.random() < (0.9 if name == "random-a" else 0.3)) for j in range(m)]


def encode(bits, bitlist):
    m = len(bits)
    out = bytearray(m // 8 + 1 if bitlist else (m + 7) // 8)
    for j, b in enumerate(bits):
        out[j >> 3] |= b << (j & 7)
    if bitlist:
        out[m >> 3] |= 1 << (m & 7)
    return bytes(out)


def run(H, C, keys, m, field, lanes, offset=0, has_members=1):
    """The string placed at byte `offset` of a buffer that ends with it."""
    buf = ctypes.create_string_buffer(bytes(offset) + field, offset + len(field) or 1)
    out = ctypes.create_string_buffer(96)
    info = (ctypes.c_uint32 * 3)()
    st = H.h_bits_key(C, keys, m, has_members, ctypes.addressof(buf) + offset, len(field), lanes, out, info)
    return st, out.raw, list(info)


@pytest.mark.parametrize("m", SIZES)
def test_keys_equal_the_oracle(H, keys, m):
    C = scalar_key(range(m))
    for name in PATTERNS:
        bits = pattern_bits(m, name)
        part = [j for j in range(m) if bits[j]]
        p = len(part)
        want = scalar_key(part)
        subtract = m - p < p
        for bitlist in (False, True):
            field = encode(bits, bitlist)
            assert H.h_bits_work(field, len(field), m) == (m - p if subtract else p)
            for lanes in FORMS:
                for offset in range(4):
                    st, key, info = run(H, C, keys, m, field, lanes, offset)
                    assert (st, key) == (SUCCESS, want), (m, name, bitlist, lanes, offset)
                    # the direction: absentees only when they are the fewer; p == m adds nothing
                    assert info == [p, int(subtract), m - p if subtract else p], (m, name, bitlist, lanes, offset)


def malformed(m, bits):
    """Every malformed string over m members derived from the valid pattern `bits`."""
    v, l = encode(bits, False), encode(bits, True)
    out = {"vector one byte long": v + b"\0", "list one byte long": l + b"\0",
           "vector one byte short": v[:-1], "vector two bytes long": v + b"\0\0", "empty": b""}
    if m % 8:  # (a list of 8 k members less its delimiter byte IS the vector)
        out["list one byte short"] = l[:-1]
    else:
        out["long form without its delimiter"] = l[:-1] + bytes([l[-1] & 0xFE])
    for name, s in (("vector", v), ("list", l)):
        top = 8 * len(s) - 1
        for pos, tag in ((m + 1, "bit m+1"), (top, "last bit of the last byte")):
            if m < pos <= top:  # position m itself is the delimiter: the string would be a Bitlist
                t = bytearray(s)
                t[pos >> 3] |= 1 << (pos & 7)
                out["%s with %s" % (name, tag)] = bytes(t)
    # a bit at m AND one above it
    if m + 1 <= 8 * len(v) - 1:
        t = bytearray(v)
        t[m >> 3] |= 1 << (m & 7)
        t[(m + 1) >> 3] |= 1 << ((m + 1) & 7)
        out["bits m and m+1"] = bytes(t)
    return out


@pytest.mark.parametrize("m", SIZES)
def test_malformed_strings_are_rejected(H, keys, m):
    C = scalar_key(range(m))
    for name in ("all", "one-clear", "random-b"):
        bits = pattern_bits(m, name)
        cases = malformed(m, bits)
        assert len(cases) >= 5
        for tag, field in cases.items():
            for lanes in FORMS:
                for offset in range(4):
                    st, key, info = run(H, C, keys, m, field, lanes, offset)
                    assert (st, key, info[2]) == (BAD_ENCODING, bytes(96), 0), (m, name, tag, lanes, offset)


def test_bit_m_of_the_short_form_is_the_delimiter(H, keys):
    """When m % 8 != 0 both encodings have the same length and bit m decides: a Bitvector with bit m
    set IS the Bitlist with the same members, not a stray bit."""
    for m in (7, 9, 17, 33, 257):
        bits = pattern_bits(m, "random-a")
        v = bytearray(encode(bits, False))
        v[m >> 3] |= 1 << (m & 7)
        assert bytes(v) == encode(bits, True)
        assert run(H, scalar_key(range(m)), keys, m, bytes(v), 1)[:2] == (SUCCESS, scalar_key(j for j in range(m) if bits[j]))


@pytest.mark.parametrize("lanes", FORMS)
def test_slots_and_members(H, keys, lanes):
    m = 33
    C = scalar_key(range(m))
    full, most = encode([1] * m, True), encode(pattern_bits(m, "one-clear"), True)
    few = encode(pattern_bits(m, "one-set"), False)
    # an invalid (all-zero) cached sum rejects the set in either direction, and with every bit set
    for field in (full, most, few):
        assert run(H, bytes(96), keys, m, field, lanes)[:2] == (BAD_ENCODING, bytes(96))
        assert run(H, C, keys, m, field, lanes, has_members=0)[:2] == (BAD_ENCODING, bytes(96))
    # an invalid member key among those added
    bad = bytearray(keys[:96 * m])
    bad[96 * (m // 3):96 * (m // 3) + 96] = bytes(96)   # the one absentee of `most`
    assert run(H, C, bytes(bad), m, most, lanes)[:2] == (BAD_ENCODING, bytes(96))
    assert run(H, C, bytes(bad), m, full, lanes)[:2] == (SUCCESS, C)   # p == m: the cached sum, nothing added
    assert run(H, C, bytes(bad), m, few, lanes)[:2] == (SUCCESS, scalar_key([(2 * m) // 3]))


@pytest.mark.parametrize("lanes", FORMS)
def test_degenerate_final_addition(H, lanes):
    """The final mixed addition C - S of the absentee direction in its three cases.  Committee
    {P, -P, X} (cached sum X) with bits {P, X}: X + P, the generic case.  Committee {X, X, -X} with
    bits {X, X}: X - (-X), a doubling.  Committee {X, -X, X} with bits {X, -X}: X - X, the identity,
    written all-zero with SUCCESS."""
    X = O.g1_mul(G1, 77)
    P = O.g1_mul(G1, 5)
    nP, nX = O.g1_neg(P), O.g1_neg(X)
    com = g1_b(P) + g1_b(nP) + g1_b(X)
    assert run(H, g1_b(X), com, 3, encode([1, 0, 1], True), lanes)[:2] == (SUCCESS, g1_b(O.g1_add(X, P)))
    # {X, X, -X}: C = X; bits {X, X}: C - (-X) = 2 X, a doubling in jac_add_aff
    com = g1_b(X) + g1_b(X) + g1_b(nX)
    assert run(H, g1_b(X), com, 3, encode([1, 1, 0], False), lanes)[:2] == (SUCCESS, g1_b(O.g1_add(X, X)))
    # {X, -X, X}: C = X; bits {X, -X}: C - X = infinity, written all-zero with SUCCESS
    com = g1_b(X) + g1_b(nX) + g1_b(X)
    assert run(H, g1_b(X), com, 3, encode([1, 1, 0], True), lanes)[:2] == (SUCCESS, bytes(96))


def test_harness_under_asan_ubsan(tmp_path):
    """The harness as a stand-alone program (its own main) under ASan/UBSan, run once."""
    exe = str(tmp_path / "bits_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-DBITS_MAIN",
                           "-I/opt/rocm/include", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    log = out.stdout[-3000:] + out.stderr[-3000:]
    assert out.returncode == 0, log
    assert "bits_harness: OK" in out.stdout, log
