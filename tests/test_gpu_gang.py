"""The quad and row gang curve arithmetic (grandine_amd/csrc/bls_gang.h) bit by bit on the GPU,
below the level of a verdict.

tools/ubench/gang_check runs every function of the header, in the forms the kernels call it
(fresh and aliased outputs), one DPP quad or one DPP row per case, and writes the result words of
every lane; tools/ubench/gang_vectors.py recomputes every word with Python integers (the
formulas of the header comments over Fp and Fp2; on-curve cases are pinned to the oracle's group
law by tests/test_gang_vectors.py).  Everything the header computes is canonical, so the
tolerance is none: every word of every lane of every case must match.

Three launches serve all tests: the cases interleaved (every wave of 16 quads / 4 rows holds a
generic addition, one that takes the doubling branch, one with an infinite result and one that
copies an operand), the same cases sorted by op and outcome (uniform waves), and a short list
whose last waves are partly filled."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "ubench", "_bin")
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
import gang_vectors as V  # noqa: E402


def _exe(name):
    path = os.path.join(BIN, name)
    if not os.path.exists(path):
        raise AssertionError("%s not built (make -C tools/ubench)" % path)
    return path


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{order name: (cases, the checker's OUT bytes)}: one launch of gang_check per order."""
    d = tmp_path_factory.mktemp("gang")
    out = {}
    for name, cases in zip(("interleaved", "sorted", "ragged"), V.build_orders()):
        src, dst = str(d / (name + ".bin")), str(d / (name + ".out"))
        V.write_cases(src, cases)
        r = subprocess.run([_exe("gang_check"), src, dst], capture_output=True, text=True, timeout=120)
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


def test_gang_fp2_products(runs):
    """gang_fp2_mul (r fresh, r aliasing a, r aliasing b, a == b) and row_mul4 (four distinct
    products, outputs aliasing inputs, the (t, x, x, x) form): random operands and 0 / Montgomery
    one / p - 1 patterns, c0 = c1 = p - 1 (lazy sum 2p - 2), c0 = 0, c1 = 0."""
    _check(runs, ("gang_fp2_mul", "row_mul4"))


def test_gang_g2_quad_point_ops(runs):
    """gang_dbl and gang_add, r fresh and aliased: off-curve triples, on-curve points in and
    outside the subgroup with random Z, edge coordinates, Y = 0, infinite operands with arbitrary
    words, a = +-b in the same and in a scaled representation, H = 0 with R != 0."""
    _check(runs, ("gang_dbl", "gang_add"))


def test_gang_g2_row_point_ops(runs):
    """row_dbl and row_add on the same kinds of operands; three of every four row cases are
    additions that leave the generic formula, so every wave of 4 rows diverges."""
    _check(runs, ("row_dbl", "row_add"))


def test_gang_g1_quad_ops(runs):
    """gang1_dbl and gang1_add over Fp: multiples of the G1 generator with random Z, off-curve
    triples, edge coordinates and every degenerate addition."""
    _check(runs, ("gang1_dbl", "gang1_add"))


def test_gang_line_steps(runs):
    """The Miller doubling and addition steps on quads and rows: the new T and L0, L2, L3 (T with
    random Z, Z = 1, off-curve operands, theta = lambda = 0)."""
    _check(runs, ("gang_line_dbl", "gang_line_add_aff", "row_line_dbl", "row_line_add_aff"))


def test_gang_xabs_and_scalar_chains(runs):
    """[|x|]P on quads and rows and the MSB-first chains of k_mv_g1mul (then g1s_from_jac) and
    k_mv_g2mul (both 32-bit halves; scalars 1, 2, 2^32 - 1, 2^32, 2^63, 2^64 - 1 and random):
    every intermediate accumulator, and the final value in every lane."""
    _check(runs, ("gang_mul_by_xabs", "row_mul_by_xabs", "k_mv_g1mul", "k_mv_g2mul"))


def test_gang_line_chains(runs):
    """The 68-event loops of k_lines and k_lines_row: every event's three coefficients and the
    final T, in every lane."""
    _check(runs, ("k_lines", "k_lines_row"))


def test_gang_interleaved_equals_sorted(runs):
    """The same case returns the same words whether its wave's other quads / rows take other
    branches (interleaved) or the same one (sorted)."""
    a = V.compare(*runs["interleaved"])
    b = V.compare(*runs["sorted"])
    assert a.total() == b.total() == len(runs["interleaved"][0]) == len(runs["sorted"][0])
    assert set(a.words) == set(b.words)
    diff = [i for i in a.words if a.words[i] != b.words[i]]
    assert not diff, "%d cases differ between the orders, first ids %s" % (len(diff), diff[:8])
    assert b.ok, b.text()


def test_gang_ragged_tail(runs):
    """21 quad cases and 5 row cases: whole quads / rows return early inside the last wave."""
    cases, out = runs["ragged"]
    assert sum(1 for c in cases if not V.is_row(c.op)) % 16 == 5 and sum(1 for c in cases if V.is_row(c.op)) % 16 == 5
    rep = V.compare(cases, out)
    assert rep.total() == len(cases) and rep.ok, rep.text()
