"""The map stage of hash_to_G2 and the decoder's Fp2 square root on raw field elements, on the GPU.

Whole hashes of random messages never reach u = 0 (tv1 = 0), sgn0's c0 == 0 case, a y^2 that lies
in Fp (the delta == 0 fallback of the square root) or the inversion path of fp2_sqrt_norm_inv.
tools/ubench/h2c_check feeds such elements straight to fp2_sqrt_pow, fp2_sqrt_norm_inv and
map_to_g2, every case once per lane (fp_pow_pm3d4, as k_h2c_map and k_g2_decompress run) and once
per 16-lane row (RowPow of bls_dfp.h, the struct k_h2c_map_row and k_g2_decompress_row pass);
tools/ubench/h2c_vectors.py recomputes everything with Python integers.  The square roots are exact
(flag and every word of the root the formula selects), the map is compared as the affine point
against the oracle's iso_map_g2(map_to_curve_sswu(u)).  No tolerance, no case skipped.

Three launches serve all tests: the cases interleaved (every wave mixes ops and classes), the same
cases sorted by op, and a short list whose last wave is partly filled."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "ubench", "_bin")
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
import h2c_vectors as V  # noqa: E402


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{order name: (cases, the checker's OUT bytes)}: one run of h2c_check per order."""
    exe = os.path.join(BIN, "h2c_check")
    if not os.path.exists(exe):
        raise AssertionError("%s not built (make -C tools/ubench)" % exe)
    d = tmp_path_factory.mktemp("h2c")
    out = {}
    for name, cases in zip(("interleaved", "sorted", "ragged"), V.build_orders()):
        src, dst = str(d / (name + ".bin")), str(d / (name + ".out"))
        V.write_cases(src, cases)
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[name] = (cases, open(dst, "rb").read())
    return out


def _check(runs, op, order="interleaved"):
    cases, out = runs[order]
    rep = V.compare(cases, out)
    want = sum(1 for c in cases if c.op == op)
    assert want and all(rep.compared[(p, op)] == want for p in V.POLICIES)  # no case skipped or filtered
    bad = [f for f in rep.failed if f[2] == op]
    assert not bad, "%d of %d failed: %s" % (len(bad), 2 * want, bad[:6])
    return rep, [c for c in cases if c.op == op]


def test_fp2_sqrt_pow_exact(runs):
    """The decoder's square root on 0, 1, -1, a1 = 0 with a0 a residue and a non-residue (the
    delta == 0 fallback), a0 = 0, random squares and non-squares: the flag and every word of the
    root the formula selects, under both exponentiations, which return the same words."""
    rep, cs = _check(runs, "sqrt_pow")
    assert len(cs) == 36 and {c.cls for c in cs} >= {"zero", "a1=0 residue", "a1=0 non-residue", "a0=0", "non-square"}
    assert all(rep.words[("lane", c.id)] == rep.words[("row", c.id)] for c in cs)


def test_fp2_sqrt_norm_inv_exact(runs):
    """The map's square root with 1 / nd from the same exponentiation, both roots of the norm as
    gamma, nd in {1, 2, 3, p-1, random}: r^2 == a, ndinv nd == 1, every word the formula's; a = 0
    takes the inversion path."""
    rep, cs = _check(runs, "sqrt_norm_inv")
    assert len(cs) == 60 and sum(1 for c in cs if c.a == (0, 0)) == 2
    assert all(rep.words[("lane", c.id)] == rep.words[("row", c.id)] for c in cs)


def test_map_to_g2_against_the_oracle(runs):
    """u = 0 (tv1 = 0), 1, (0, 1), (p-1, 0), (0, p-1), c0 = 0 with odd and even c1 (sgn0 decided by
    c1), c1 = 0 and 32 random u, both SSWU branches among them: the affine point equals
    iso_map_g2(map_to_curve_sswu(u)) under the lane and the row policy."""
    rep, cs = _check(runs, "map_to_g2")
    assert len(cs) == 42
    rnd = [V.gx1_is_square(c.a) for c in cs if c.cls == "random"]
    assert len(rnd) == 32 and any(rnd) and not all(rnd)


def test_interleaved_equals_sorted(runs):
    """The same case returns the same words whether its wave's other lanes (rows) run other ops
    or the same one."""
    a = V.compare(*runs["interleaved"])
    b = V.compare(*runs["sorted"])
    n = len(runs["interleaved"][0])
    assert a.total() == b.total() == 2 * n == 2 * len(runs["sorted"][0]) and set(a.words) == set(b.words)
    diff = [k for k in a.words if a.words[k] != b.words[k]]
    assert not diff, "%d results differ between the orders, first %s" % (len(diff), diff[:8])
    assert a.ok and b.ok, a.text() + b.text()


def test_ragged_tail(runs):
    """101 cases: the lane launch's last wave holds 37 lanes, the row launch's last block one row
    of four; the rest return early."""
    cases, out = runs["ragged"]
    assert len(cases) % 64 == 37 and (16 * len(cases)) % 64 == 16 and {c.op for c in cases} == set(V.OPS)
    rep = V.compare(cases, out)
    assert rep.total() == 2 * len(cases) and rep.ok, rep.text()
