"""CPU: the per-set step of the cached-committee keys (grandine_amd/csrc/gbls_committees.h, the text
k_g1_committee_keys compiles for gfx950) built for the host (tests/native/committees_harness.cpp)
and checked against the pure-Python oracle: key = C - S for a committee set, S otherwise, exact
also where C - S is a doubling or the identity.  The same harness runs once as a stand-alone
program under AddressSanitizer and UBSan."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "committees_harness.cpp")
SO = os.path.join(ROOT, "tests", "native", "_build", "libcommittees_harness.so")
MONT = 1 << 384
SUCCESS, BAD_ENCODING, AGGR_TYPE_MISMATCH = 0, 1, 4
CK_COMMITTEE = 1
FORMS = [1, 16]  # lanes per set: the kernel's lane form and its 16-lane row form
G1 = O.sk_to_pk(1)


@pytest.fixture(scope="module")
def H():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-o", SO, SRC])
    L = ctypes.CDLL(SO)
    L.h_committee_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.c_uint32, ctypes.c_char_p]
    return L


def fp_b(x):
    return (x * MONT % O.P).to_bytes(48, "little")


def g1_b(p):
    return bytes(96) if p is None else fp_b(p[0]) + fp_b(p[1])


def total(pts):
    acc = None
    for p in pts:
        acc = O.g1_add(acc, p)
    return acc


def key(H, C, keys, committee, lanes):
    out = ctypes.create_string_buffer(96)
    st = H.h_committee_key(g1_b(C), b"".join(g1_b(p) for p in keys) or bytes(96), len(keys),
                           CK_COMMITTEE if committee else 0, lanes, out)
    return st, out.raw


@pytest.fixture(scope="module")
def members():
    rng = random.Random(31)
    return [O.g1_mul(G1, rng.randrange(1, O.R)) for _ in range(24)]


@pytest.mark.parametrize("lanes", FORMS)
def test_committee_minus_absentees(H, members, lanes):
    C = total(members)
    for m in (0, 1, 2, 17):
        absent = members[3:3 + m]
        want = O.g1_add(C, O.g1_neg(total(absent))) if m else C
        assert want == total(members[:3] + members[3 + m:])
        assert key(H, C, absent, True, lanes) == (SUCCESS, g1_b(want)), m
        # the participants without a committee give the same key
        assert key(H, C, members[:3] + members[3 + m:], False, lanes) == (SUCCESS, g1_b(want)), m


@pytest.mark.parametrize("lanes", FORMS)
def test_degenerate_sums_are_exact(H, members, lanes):
    C = total(members[:5])
    # S = C: the identity, written all-zero; every member absent is the same case
    assert key(H, C, [C], True, lanes) == (SUCCESS, bytes(96))
    assert key(H, C, members[:5], True, lanes) == (SUCCESS, bytes(96))
    # S = -C: a doubling
    assert key(H, C, [O.g1_neg(C)], True, lanes) == (SUCCESS, g1_b(O.g1_add(C, C)))
    assert key(H, C, [O.g1_neg(p) for p in members[:5]], True, lanes) == (SUCCESS, g1_b(O.g1_mul(C, 2)))
    # S infinite from a nonempty list of cancelling keys: the key is C
    p, q = members[7], members[8]
    assert key(H, C, [p, q, O.g1_neg(p), O.g1_neg(q)], True, lanes) == (SUCCESS, g1_b(C))
    # ... and without a committee an infinite sum is a SUCCESS written all-zero
    assert key(H, None, [p, O.g1_neg(p)], False, lanes) == (SUCCESS, bytes(96))


@pytest.mark.parametrize("lanes", FORMS)
def test_rejections(H, members, lanes):
    C = total(members[:5])
    # an invalid (all-zero) cached sum, with and without absentees
    assert key(H, None, [], True, lanes) == (BAD_ENCODING, bytes(96))
    assert key(H, None, members[:2], True, lanes) == (BAD_ENCODING, bytes(96))
    # no committee and an empty list
    assert key(H, None, [], False, lanes) == (AGGR_TYPE_MISMATCH, bytes(96))
    assert key(H, C, [], False, lanes) == (AGGR_TYPE_MISMATCH, bytes(96))
    # an invalid key in the list
    assert key(H, C, [members[0], None, members[1]], True, lanes) == (BAD_ENCODING, bytes(96))
    assert key(H, C, [members[0], None], False, lanes) == (BAD_ENCODING, bytes(96))
    # a committee with an empty list is the cached sum itself
    assert key(H, C, [], True, lanes) == (SUCCESS, g1_b(C))


def test_harness_under_asan_ubsan(tmp_path):
    """The harness as a stand-alone program (its own main) under ASan/UBSan, run once."""
    exe = str(tmp_path / "committees_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-DCOMMITTEES_MAIN",
                           "-I/opt/rocm/include", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    log = out.stdout[-3000:] + out.stderr[-3000:]
    assert out.returncode == 0, log
    assert "committees_harness: OK" in out.stdout, log
