"""CPU: the cases and expectations of tools/ubench/h2c_vectors.py (tests/test_gpu_h2c_map.py runs
them on the GPU): the restated square-root formulas against the oracle's Fp2 arithmetic, the input
classes, the comparator on a model output and on corrupted ones, and the checker's host mode (the
lane policy through the headers' host branches)."""
import os
import struct
import subprocess
import sys

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
import h2c_vectors as V  # noqa: E402

P = O.P


@pytest.fixture(scope="module")
def orders():
    return V.build_orders()


def test_case_classes(orders):
    inter, sorted_, ragged = orders
    assert len(inter) == len(sorted_) == 138 and sorted(c.id for c in inter) == list(range(138))
    n = {op: sum(1 for c in inter if c.op == op) for op in V.OPS}
    assert n == {"sqrt_pow": 36, "sqrt_norm_inv": 60, "map_to_g2": 42}
    sq = [c for c in inter if c.op == "sqrt_pow"]
    cls = {k: [c for c in sq if c.cls == k] for k in {c.cls for c in sq}}
    assert set(cls) == {"zero", "one", "minus one", "a1=0 residue", "a1=0 non-residue", "a0=0", "random square",
                        "non-square"}
    assert all(c.a[1] == 0 and O.fp_is_square(c.a[0]) for c in cls["a1=0 residue"]) and len(cls["a1=0 residue"]) == 3
    assert all(c.a[1] == 0 and not O.fp_is_square(c.a[0]) for c in cls["a1=0 non-residue"] + cls["minus one"])
    assert all(c.a[0] == 0 and c.a[1] != 0 for c in cls["a0=0"]) and len(cls["a0=0"]) == 5
    assert len(cls["non-square"]) == 6 and len(cls["random square"]) == 16
    ni = [c for c in inter if c.op == "sqrt_norm_inv"]
    assert all(c.gamma * c.gamma % P == (c.a[0] ** 2 + c.a[1] ** 2) % P and c.nd != 0 for c in ni)
    assert {c.nd for c in ni} >= {1, 2, P - 1} and len({c.nd for c in ni}) == 6
    assert not any(c.cls.startswith("non-square") for c in ni)
    us = [c for c in inter if c.op == "map_to_g2"]
    assert [c.a for c in us[:5]] == [(0, 0), (1, 0), (0, 1), (P - 1, 0), (0, P - 1)]
    assert sum(1 for c in us if c.cls == "c0=0 odd c1" and c.a[0] == 0 and c.a[1] & 1) == 2
    assert sum(1 for c in us if c.cls == "c0=0 even c1" and c.a[0] == 0 and not c.a[1] & 1) == 2
    rnd = [V.gx1_is_square(c.a) for c in us if c.cls == "random"]
    assert len(rnd) == 32 and 8 <= sum(rnd) <= 24  # the gx1-square and the non-square branch both occur
    assert V.gx1_is_square((0, 0))  # u = 0: tv1 = 0, x1 = B / (Z A), whose g(x1) is a square
    # interleaved: every wave mixes the ops; ragged: 37 lanes in the last wave
    assert all(len({c.op for c in inter[k:k + 64]}) == 3 for k in (0, 64))
    assert len(ragged) == 101 and ragged == inter[:101]


def test_restated_square_roots_agree_with_the_oracle(orders):
    for c in orders[0]:
        if c.op == "sqrt_pow":
            flag, r = V.sqrt_pow(c.a)
            assert flag == O.f2_is_square(c.a), c.cls
            if flag:
                assert O.f2_sqr(r) == c.a and r in (O.f2_sqrt(c.a), O.f2_neg(O.f2_sqrt(c.a)))
            if c.cls in ("a1=0 non-residue", "minus one"):
                assert r[0] == 0 and r[1] != 0  # the delta == 0 fallback: a purely imaginary root
            if c.cls in ("a1=0 residue", "one"):
                assert r[1] == 0 and r[0] != 0
        elif c.op == "sqrt_norm_inv":
            r, ndinv = V.sqrt_norm_inv(c.a, c.gamma, c.nd)
            assert O.f2_sqr(r) == c.a and ndinv == O.fp_inv(c.nd) and (c.a != (0, 0) or r == (0, 0))
    assert V.sqrt_pow((P - 1, 0)) in ((True, (0, 1)), (True, (0, P - 1)))
    assert V.words(1) == [(((1 << 384) % P) >> (32 * i)) & 0xFFFFFFFF for i in range(12)]
    assert V.of_words(V.words(P - 5)) == (P - 5, True) and not V.of_words([0xFFFFFFFF] * 12)[1]


def test_comparator(orders):
    cases = orders[0]
    good = V.model_output(cases)
    rep = V.compare(cases, good, policies=("lane",))
    assert rep.ok and rep.total() == len(cases), rep.text()
    assert not V.compare(cases, good).ok  # the row half is still at its fill
    w = list(struct.unpack("<%dI" % (len(good) // 4), good))
    pos = {c.id: i for i, c in enumerate(cases)}

    def failing(mutate):
        m = list(w)
        mutate(m)
        return {(f[1], f[2]) for f in V.compare(cases, struct.pack("<%dI" % len(m), *m), policies=("lane",)).failed}

    imag = next(c for c in cases if c.op == "sqrt_pow" and c.cls == "a1=0 non-residue")
    ns = next(c for c in cases if c.op == "sqrt_pow" and c.cls == "non-square")
    ni = next(c for c in cases if c.op == "sqrt_norm_inv")
    mp = next(c for c in cases if c.op == "map_to_g2" and c.cls == "random")

    def neg_root(m):  # the other root: r^2 == a still holds, the formula's choice does not
        b = pos[imag.id] * V.OUT_WORDS + 1
        r = V.sqrt_pow(imag.a)[1]
        m[b:b + 24] = V.words(-r[0] % P) + V.words(-r[1] % P)

    assert failing(neg_root) == {(imag.id, "sqrt_pow")}
    assert failing(lambda m: m.__setitem__(pos[ns.id] * V.OUT_WORDS, 1)) == {(ns.id, "sqrt_pow")}
    assert failing(lambda m: m.__setitem__(pos[ni.id] * V.OUT_WORDS + 30, m[pos[ni.id] * V.OUT_WORDS + 30] ^ 1)) == {
        (ni.id, "sqrt_norm_inv")}
    assert failing(lambda m: m.__setitem__(pos[mp.id] * V.OUT_WORDS + 40, m[pos[mp.id] * V.OUT_WORDS + 40] ^ 4)) == {
        (mp.id, "map_to_g2")}
    assert failing(lambda m: m.__setitem__(pos[ni.id] * V.OUT_WORDS + 36, 0)) == {(ni.id, "sqrt_norm_inv")}  # past the result

    def add_p(m):  # the same residue, words not below p
        b = pos[ni.id] * V.OUT_WORDS
        v = sum(x << (32 * i) for i, x in enumerate(m[b:b + 12])) + P
        if v < 1 << 384:
            m[b:b + 12] = [(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)]
        else:
            m[b] ^= 1

    assert failing(add_p) == {(ni.id, "sqrt_norm_inv")}


def test_checker_cross_compiles_and_its_host_mode_passes(orders, tmp_path):
    """The lane policy through the headers' host branches, same checker and file layout: every case
    of the interleaved and the ragged order; the row half of OUT stays at its fill."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "ubench"), "-s"])
    exe = os.path.join(ROOT, "tools", "ubench", "_bin", "h2c_check")
    assert os.path.exists(exe)
    inter, _, ragged = orders
    for name, cases in (("interleaved", inter), ("ragged", ragged)):
        src, dst = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".out"))
        V.write_cases(src, cases)
        r = subprocess.run([exe, "--host", src, dst], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = open(dst, "rb").read()
        rep = V.compare(cases, out, policies=("lane",))
        assert rep.ok and rep.total() == len(cases), rep.text()
        assert out[len(out) // 2:] == b"\xee" * (len(out) // 2)
