"""The radix-2^28 field layer (grandine_amd/csrc/bls_field28.h) bit by bit on the GPU: the device
branch of its products is generated v_mad_u64_u32 assembly (bls_fpmul28_gen.h) that no host test
compiles, and fe2_mul3k's Karatsuba form exists on the device only.

tools/ubench/field28_check runs every product primitive in the forms the kernels call it (fresh
and aliased outputs), the Fp2 and sparse composites, the three Miller product forms, a 30-step
chain per form, the conversions and the (p-3)/4 exponentiation, one case per lane on RAW limb
images; tools/ubench/field28_vectors.py recomputes everything with Python integers.  The six
primitives, the conversions and the exponentiation are exact: every word must match, no tolerance.
A composite's representative depends on its internal sequence: each output coefficient is checked
for its residue mod p, limbs < 2^28 and the value bound the header states.

Three launches serve all tests: the cases interleaved (every 64-lane wave mixes ops and case
classes), the same cases sorted by op (uniform waves) and a short list whose last wave is partly
filled."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "ubench", "_bin")
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
import field28_vectors as V  # noqa: E402


def _exe(name):
    path = os.path.join(BIN, name)
    if not os.path.exists(path):
        raise AssertionError("%s not built (make -C tools/ubench)" % path)
    return path


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{order name: (cases, the checker's OUT bytes)}: one launch of field28_check per order."""
    d = tmp_path_factory.mktemp("field28")
    out = {}
    for name, cases in zip(("interleaved", "sorted", "ragged"), V.build_orders()):
        src, dst = str(d / (name + ".bin")), str(d / (name + ".out"))
        V.write_cases(src, cases)
        r = subprocess.run([_exe("field28_check"), src, dst], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[name] = (cases, open(dst, "rb").read())
    return out


def _check(runs, funcs, order="interleaved"):
    cases, out = runs[order]
    ops = {op for fn in funcs for op in V.FUNCS[fn]}
    rep = V.compare(cases, out, ops=ops)
    want = {}
    for c in cases:
        if c.op in ops:
            want[c.op] = want.get(c.op, 0) + 1
    assert rep.compared == want and set(want) == ops  # no case skipped or filtered
    assert rep.ok, rep.text()
    return rep


def test_field28_primitives_exact(runs):
    """mul, sqr, mul2, mul4, mul6: every word equal to (T + m p) / 2^392 on canonical and lazy
    operands, 0 / 1 / Montgomery one / p-1 / p / 2p-1, one-hot limb pairs at their limits for every
    (i, j) of every pair (one generated term line each), and the top-of-contract patterns (limbs at
    2^28 - 1 / 2^29 - 1, values at 32 p, 1.1 p x 5.1 p: column peaks up to 2^63.33)."""
    _check(runs, ("mul", "sqr", "mul2", "mul4", "mul6"))


def test_field28_aliasing_and_square(runs):
    """mul with r = a, r = b and a == b by reference, sqr with r = a, mul2 with r = c: the forms of
    one operand set return the same words, and sqr(a) == mul(a, a) word for word."""
    rep = _check(runs, ("mul", "sqr", "mul2"))
    cases = runs["interleaved"][0]
    by, disagree = V.group_disagreements(cases, rep)
    assert not disagree, disagree[:4]
    forms = {}
    for cs in by.values():
        key = tuple(sorted(c.op for c in cs))
        forms[key] = forms.get(key, 0) + 1
    assert forms[("mul", "mul_ra", "mul_rb")] == 69 and forms[("mul_aa", "sqr", "sqr_ra")] == 69
    assert forms[("mul_aa", "sqr")] == 105 and forms[("mul2", "mul2_rc")] == 45


def test_field28_mul3k(runs):
    """fe2_mul3k (device only): exact against T0 = A - B + 17 p^2, T1 = C - A - B, the sums formed
    with fe2_sum; one-hot A and B terms of every pair, A = 0 with B = 16.83 p^2 against the bias,
    B = 0 with A at its maximum, operands in opposite limb ranges (the signed accumulator negative
    in every column in turn)."""
    rep = _check(runs, ("fe2_mul3k",))
    cases = runs["interleaved"][0]
    special = {c.cls for c in cases if c.op == "mul3k" and c.id in rep.words}
    assert {"A=0 B max", "B=0 A max", "A high B low", "A low B high", "top", "onehot"} <= special


def test_field28_fp2_and_sparse_composites(runs):
    """fe2_mul (r fresh, r = a), fe2_sqr, fe2_mul_fe, sp_from_engine (exact), sp_mul_sp_lazy and
    sp_mul_sp: residues against the Fp2 / Fp12 formulas, limbs < 2^28, the header's bounds."""
    _check(runs, ("fe2_mul", "fe2_sqr", "fe2_mul_fe", "sp_from_engine", "sp_mul_sp_lazy", "sp_mul_sp"))


def test_field28_miller_forms_and_chains(runs):
    """fe12_mul_034 and its _st, _lazy, _lazy_st, _kara_st forms on one operand set (f and the line
    coefficients canonical, in [p, 1.1 p), at 1.1 p - 1 with every limb full), and per stashed form
    the inner loop of k_ml_group28 in miniature: sp_mul_sp_lazy, then 30 dense x sparse steps fed
    back, every accumulator written and checked (outputs < 1.1 p / 1.02 p / 1.03 p)."""
    _check(runs, ("fe12_mul_034", "fe12_mul_034_st", "fe12_mul_034_lazy", "fe12_mul_034_lazy_st",
                  "fe12_mul_034_kara_st", "miller_chain"))
    cases = runs["interleaved"][0]
    assert sorted(V.FORMS[c.aux] for c in cases if c.op == "chain") == sorted(V.CHAIN_FORMS * 4)


def test_field28_conversions_and_exponentiation(runs):
    """from_fp, to_fp, fe12_to_engine_scaled and fp_pow_pm3d4 (its table in LDS, 64 lanes per
    work-group) are canonical or single products: exact words; the exponentiation against
    pow(a, (p-3)/4, p) in the engine's Montgomery form, also on 0, one, p-1 and words above p."""
    _check(runs, ("from_fp", "to_fp", "fe12_to_engine_scaled", "fp_pow_pm3d4"))


def test_field28_interleaved_equals_sorted(runs):
    """The same case returns the same words whether its wave's other lanes run other ops
    (interleaved) or the same one (sorted)."""
    a = V.compare(*runs["interleaved"])
    b = V.compare(*runs["sorted"])
    assert a.total() == b.total() == len(runs["interleaved"][0]) == len(runs["sorted"][0])
    assert set(a.words) == set(b.words)
    diff = [i for i in a.words if a.words[i] != b.words[i]]
    assert not diff, "%d cases differ between the orders, first ids %s" % (len(diff), diff[:8])
    assert b.ok, b.text()


def test_field28_ragged_tail(runs):
    """101 cases, every op and chain form among them: the last wave holds 37 lanes, the rest
    return early."""
    cases, out = runs["ragged"]
    assert len(cases) % 64 == 37 and {c.op for c in cases} == set(V.OPS)
    rep = V.compare(cases, out)
    assert rep.total() == len(cases) and rep.ok, rep.text()
