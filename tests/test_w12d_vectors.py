"""CPU: the case generator and the expectations of the row-distributed Fp12 engine's GPU checker
(tools/ubench/w12d_vectors.py, tests/test_gpu_w12d.py) are themselves right: encodings
round-trip, every generated operand meets the contract it claims, the oracle expectations are
self-consistent, the engine's coefficient order is the one the host engine multiplies in, and the
checker cross-compiles."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
import w12d_vectors as V  # noqa: E402

O = V.O
P = O.P


@pytest.fixture(scope="module")
def cases():
    return V.build_cases()


def test_image_encoding_round_trips():
    rng = random.Random(1)
    for _ in range(20):
        a = V.random_f12(rng)
        img = V.image_of_f12(a)
        assert V.image_true(img) == a
        assert V.image_from_words(V.image_words(img)) == img
        assert V.image_true(V.image_of_f12(a, add=127 * P)) == a
        assert V.f12_from_engine_bytes(V.engine_bytes(a)) == a
        assert V.eng_to_f12(V.f12_to_eng(a)) == a
        red = [V.borrow(c, rng) for c in V.image_of_f12(a, add=127 * P)]
        assert V.image_true(red) == a
    assert V.image_true(V.image_of_values([V.ONE_M] + [0] * 11)) == O.f12_one()
    x = rng.randrange(P)
    assert V.int_of_words(V.words_of_int(x)) == x
    # borrow really produces redundant limbs when a limb allows it
    l = V.limbs_of((5 << 28) + 3)
    assert any(V.borrow(l, random.Random(s))[0] >= 1 << 28 for s in range(8))


def test_case_counts_and_records(cases, tmp_path):
    counts = {}
    for c in cases:
        counts[c.op] = counts.get(c.op, 0) + 1
        assert len(c.record()) == 4 + 2 * V.IMG and all(0 <= w < 1 << 32 for w in c.record())
    assert counts == V.COUNTS and set(counts) == set(V.OPS)
    assert all(counts[op] >= 80 for op in ("mul", "sqr", "conj", "frob", "frob2"))
    path = str(tmp_path / "cases.bin")
    V.write_cases(path, cases)
    assert os.path.getsize(path) == 4 + 4 * (4 + 2 * V.IMG) * len(cases)


def test_operands_meet_their_contracts(cases):
    tops = {}
    for c in cases:
        for img in (c.a, c.b):
            if img is None:
                continue
            for l in img:  # every operand limb and value is inside the engine's input contract
                assert all(0 <= x < V.LIMB_END for x in l) and l[14] == 0 and l[15] == 0
                assert V.value_of(l) <= 128 * P
        if c.op in ("mul", "sqr", "conj", "frob", "frob2", "easy_part", "chain") and c.kind.startswith("top"):
            top = [l for l in c.a if V.value_of(l) >= 127 * P]
            assert top
            for l in top:
                V.check_top(l)
            tops.setdefault(c.op, []).append(len(top))
        if c.kind == "random" and c.op != "chain":
            assert all(V.value_of(l) < P for l in c.a)
        if c.op in ("cyc_sqr", "exp_x_cyc", "chain_cyc"):
            a = V.image_true(c.a)
            assert O.f12_mul(a, O.f12_conj(a)) == O.f12_one()  # a^(p^6 + 1) = 1
            if c.kind == "cyc+127p":
                assert all(127 * P <= V.value_of(l) < 128 * P for l in c.a)
        if c.op == "inv_wave":
            assert V.int_of_words(c.words[:12]) < P
        if c.op == "load_scaled":
            assert all(V.int_of_words(c.words[12 * i:12 * i + 12]) < P for i in range(12))
    for op in ("mul", "sqr", "conj", "frob", "frob2"):
        assert len(tops[op]) >= 16 and 12 in tops[op]  # one image with all twelve at the top
    # the dense image: a presum of 8 coefficients sits just under 1024 p
    dense = next(c for c in cases if c.op == "sqr" and c.kind == "top")
    assert 8 * 127 * P <= sum(sorted(V.value_of(l) for l in dense.a)[:8]) < 1024 * P
    assert all(l[j] == V.LIMB_END - 1 for l in dense.a for j in range(12))
    # easy_part's special norms: F1 = 0 and F0 = 0
    for c in cases:
        if c.op == "easy_part" and c.kind in ("F1=0", "F0=0"):
            f = V.image_true(c.a)
            N = O.f12_mul(f, O.f12_conj(f))
            F = V.f6_norm(N[0], N[2], N[4])
            assert F[1 if c.kind == "F1=0" else 0] == 0 and F != (0, 0)
    # the rare exit path: g = x is 0 mod 2^30 (and mod 2^60, 2^90) and not zero
    xs = [V.int_of_words(c.words[:12]) for c in cases if c.op == "inv_wave"]
    assert sum(1 for x in xs if x and x % (1 << 60) == 0) >= 16 and sum(1 for x in xs if x and x % (1 << 90) == 0) >= 8
    assert xs.count(0) == 1


def test_flag_representatives():
    assert all(v % P == 0 for v in V.ZERO_REPS) and all(v % P for v in V.NONZERO_REPS)
    assert all(v * V.RINV % P == 1 for v in V.ONE_REPS) and all(v * V.RINV % P != 1 for v in V.NOT_ONE_REPS)
    assert all(v < (1 << 392) for v in V.ZERO_REPS + V.NONZERO_REPS + V.ONE_REPS + V.NOT_ONE_REPS)


def test_expectations_are_self_consistent(cases):
    by = {}
    for c in cases:
        by.setdefault(c.op, []).append(c)
    for s, m in list(zip(by["sqr"], by["mul_aa"]))[::7]:
        assert s.a == m.a and V.expected_f12(s) == V.expected_f12(m)
    for c in by["cyc_sqr"][::6]:
        a = V.image_true(c.a)
        assert V.expected_f12(c) == O.f12_mul(a, a)
    for c in by["exp_x_cyc"][1:4]:
        a, x = V.image_true(c.a), O.f12_one()
        for i in range(63, -1, -1):  # the header's square-and-multiply chain
            x = O.f12_sqr(x)
            if (O.X_ABS >> i) & 1:
                x = O.f12_mul(x, a)
        assert V.expected_f12(c) == O.f12_conj(x)
        # on the cyclotomic subgroup conj is the inverse: a^x for the negative x
        assert O.f12_mul(V.expected_f12(c), O.f12_pow(a, O.X_ABS)) == O.f12_one()
    steps = V.chain_expectations(by["chain_cyc"][0])
    a = V.image_true(by["chain_cyc"][0].a)
    assert steps[3][0] == O.f12_pow(a, 7) and len(steps) == V.CHAIN_STEPS
    # inv_wave's batch count: at least ceil(bits / 30)-ish and never the guard
    assert all(1 <= V.exact_batches(x) < 40 for x in (1, 2, P - 1, (1 << 90) * 5))


def test_coefficient_order_matches_host_engine():
    """The oracle's 6 Fp2 coefficients <-> the engine's 12-coefficient order, without a GPU: two
    oracle elements encoded to engine bytes, multiplied by the host build of the engine's
    product (tests/native/host_harness.cpp h_fp12_mul), decoded, against O.f12_mul."""
    so = os.path.join(ROOT, "tests", "native", "_build", "libhost_harness_w12d.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-o", so, os.path.join(ROOT, "tests", "native", "host_harness.cpp")])
    H = ctypes.CDLL(so)
    rng = random.Random(2)
    for _ in range(4):
        a, b = V.random_f12(rng), V.random_f12(rng)
        out = ctypes.create_string_buffer(576)
        H.h_fp12_mul(V.engine_bytes(a), V.engine_bytes(b), out)
        assert V.f12_from_engine_bytes(out.raw) == O.f12_mul(a, b)
    # a one-hot element pins each index: w^i u^k times w is w^(i+1) u^k (w^6 = 1 + u)
    w = [(0, 0), (1, 0)] + [(0, 0)] * 4
    for i in range(12):
        e = [0] * 12
        e[i] = 1
        out = ctypes.create_string_buffer(576)
        H.h_fp12_mul(V.engine_bytes(V.eng_to_f12(e)), V.engine_bytes(w), out)
        assert V.f12_from_engine_bytes(out.raw) == O.f12_mul(V.eng_to_f12(e), w)


def test_checker_cross_compiles():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "ubench"), "-s"])
    assert os.path.exists(os.path.join(ROOT, "tools", "ubench", "_bin", "w12d_check"))
