"""The radix-2^28 curve layer (grandine_amd/csrc/bls_curve28.h) bit by bit on the GPU: the lane
regime's point formulas with their lazy combinations, degenerate branches and representations of
infinity, under the device products (generated v_mad_u64_u32 assembly that no host test compiles)
and the kernels' register pressure.

tools/ubench/curve28_check runs every routine of the header in the forms the kernels call it
(fresh and aliased outputs, the [|x|] chain with k_h2c_chain28's attributes and its base in LDS and
again in registers, membership with the base in LDS, the 68 line events with Q in LDS), one case
per lane on RAW limb images; tools/ubench/curve28_vectors.py recomputes everything with Python
integers from formulas restated independently of the engine.  Canonical, single-product, repacked
and copied outputs and booleans must match in every word; every other coordinate is checked for its
residue mod p, limbs < 2^28 and the value bound the header states.  There is no tolerance.

Three launches serve all tests: the cases interleaved (every 64-lane wave mixes ops, generic cases
and degenerate branches), the same cases sorted by op and class (uniform waves) and a short list
whose last wave holds 37 lanes.  The host branches run the same sequences on the same integers, so
the GPU's OUT bytes also equal the checker's --host OUT bytes, for every op."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "ubench", "_bin")
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
import curve28_vectors as V  # noqa: E402


def _exe(name):
    path = os.path.join(BIN, name)
    if not os.path.exists(path):
        raise AssertionError("%s not built (make -C tools/ubench)" % path)
    return path


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{order name: (cases, the checker's OUT bytes, its --host OUT bytes)}: one launch of
    curve28_check per order."""
    d = tmp_path_factory.mktemp("curve28")
    out = {}
    for name, cases in zip(("interleaved", "sorted", "ragged"), V.build_orders()):
        src, dst, hst = str(d / (name + ".bin")), str(d / (name + ".out")), str(d / (name + ".host"))
        V.write_cases(src, cases)
        r = subprocess.run([_exe("curve28_check"), src, dst], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        r = subprocess.run([_exe("curve28_check"), "--host", src, hst], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out[name] = (cases, open(dst, "rb").read(), open(hst, "rb").read())
    return out


def _check(runs, group, order="interleaved", classes=None):
    """Every case of the group's ops (of the given classes) compared; the compared counts are the
    planned ones."""
    cases, out, _ = runs[order]
    ops = {op for fn in V.GROUPS[group] for op in V.FUNCS[fn]}
    if classes is not None:
        keep = [c for c in cases if c.op in ops and c.cls in classes]
        assert {c.cls for c in keep} == set(classes)
    rep = V.compare(cases, out, ops=ops)
    want = {}
    for c in cases:
        if c.op in ops:
            want[c.op] = want.get(c.op, 0) + 1
    assert rep.compared == want and set(want) == ops  # no case skipped or filtered
    if classes is not None:
        bad = {k: v for k, v in rep.mismatch.items() if k[1] in classes}
        assert not bad, rep.text()
        return rep
    assert rep.ok, rep.text()
    return rep


def test_curve28_point_formulas(runs):
    """jac_dbl28 (r fresh, r = p), jac_add28 (r fresh, r = a) over fe2 and fe, jac_add_aff28<true>
    and <false> (r fresh, r = a), jac_neg, jac_eq: residues against dbl-2009-l, add-2007-bl and
    madd-2007-bl coordinate by coordinate, X3, Y3 < 1.03 p, the doubling's Z3 < 2.03 p; on random
    points, coordinates at their largest representative below 2.1 p (one, all), and every limb
    full.  The aliased forms return the words of the fresh ones."""
    rep = _check(runs, "point formulas")
    assert rep.total() == 506
    by, disagree = V.group_disagreements(runs["interleaved"][0], rep)
    assert not disagree, disagree[:4]
    assert sum(1 for cs in by.values() if cs[0].op.startswith(("g2_", "g1_"))) >= 180


def test_curve28_degenerate_branches_and_infinity_representatives(runs):
    """a = b as different Jacobian representatives (the doubling branch), a = -b (jac_set_inf, exact
    words), a, b or both infinite with Z = 0, p and 2p in raw limbs (the copied operand, exact
    words), the affine (0, 0) as 0 and as p; jac_eq on equal, different, negated and infinite points
    including X = Y = Z = 0; the doubling, psi and affine conversion of an infinite point."""
    rep = _check(runs, "point formulas", classes=V.DEGENERATE)
    cases = runs["interleaved"][0]
    n = sum(1 for c in cases if c.id in rep.words and c.cls in V.DEGENERATE)
    assert n == 2 * (21 + 21 + 21 + 15)  # jac_add28 over fe2 and fe, jac_add_aff28<true>, <false>
    _check(runs, "point formulas", classes=("inf Z=0", "inf Z=p", "inf Z=2p", "inf finite", "finite inf", "inf inf",
                                            "zero finite", "finite zero", "equal", "negated", "different"))
    _check(runs, "g1h28", classes=("dbl branch", "neg branch", "a inf Z=0", "a inf Z=p", "a inf Z=2p", "b inf Z=0",
                                   "b inf Z=p", "b inf Z=2p", "both inf", "a zero", "inf Z=0", "inf Z=p", "inf Z=2p"))
    _check(runs, "maps and conversions", classes=("inf Z=0", "inf Z=p", "inf Z=2p", "aff00", "aff00 p", "aff x=0", "zero"))


def test_curve28_maps_and_conversions(runs):
    """g2_psi28, g2_psi2_28, g2j_of_aff28, jac_to_aff28, fe2_inv, inv (0 -> 0, also 0 given as p
    and 2p), half and fe2_half (exact: 0, 1, p - 1, p, the largest value below 1.03 p, odd and
    even), fe2_mul_3b up to 4 p, store12 / load12 and the g2j / g2a pairs (exact round trips),
    g2j_in (exact single products) and g2j_out (canonical)."""
    rep = _check(runs, "maps and conversions")
    assert rep.total() == 229


def test_curve28_line_steps_and_chain(runs):
    """line_dbl28 and line_add28 as single steps (T random, at the top of its 1.03 p contract, every
    limb full) and the 68 events from an affine Q parked in LDS: L0, L2, L3 of every event and the
    final T, residues and < 1.03 p."""
    rep = _check(runs, "lines")
    assert rep.compared == {"line_dbl": 19, "line_add": 19, "line_chain": 8}


def test_curve28_xabs_chain_and_membership(runs):
    """g2_xabs_aff28 in a kernel with k_h2c_chain28's attributes and the base in LDS, and again with
    the base in registers (both results compared), on subgroup points, map outputs, the clearing's
    bases, the (0, 0) base and the points of order 13, 23, 2713 and 11953 with their negations and
    sums with the generator (order 13 passes through infinity at bit 60); g2_in_group28 with the
    base in LDS: the verdicts."""
    rep = _check(runs, "xabs")
    assert rep.compared == {"xabs": 39, "in_group": 26}
    cases = runs["interleaved"][0]
    verdicts = {c.cls: set() for c in cases if c.op == "in_group"}
    for c in cases:
        if c.op == "in_group":
            verdicts[c.cls].add(rep.words[c.id])
    one, zero = (1).to_bytes(4, "little"), bytes(4)
    assert verdicts.pop("in group") == {one} and all(v == {zero} for v in verdicts.values()) and len(verdicts) == 5


def test_curve28_clearing_stages(runs):
    """clear_mid28, clear_post28, clear_cofactor28_staged and clear_cofactor28 on P = Q0 + Q1 of
    seeded map outputs, Q0 = Q1, Q0 = -Q1 (P infinite) and one Q infinite; the pre stage's
    jac_add28 and jac_to_aff28 and both chains on the same inputs."""
    rep = _check(runs, "clearing")
    assert rep.compared == {"clear_mid": 10, "clear_post": 10, "clear_staged": 10, "clear_full": 10}
    _check(runs, "point formulas", classes=("clear pre Q0 + Q1", "clear pre Q0 = Q1", "clear pre Q0 = -Q1",
                                            "clear pre Q0 inf", "clear pre Q1 inf"))
    _check(runs, "xabs", classes=("clear Q0 + Q1", "clear Q0 = Q1", "clear Q0 = -Q1", "clear Q0 inf", "clear Q1 inf"))


def test_curve28_g1_scalar_multiplication(runs):
    """g1_mul_u64_w3_28 then g1s_from_jac28, exact words: 0 ... 8, 2^63, 2^64 - 1, every digit 4,
    every digit 5 (a carry into every window, top digit 2), every signed digit value in every
    window, 64 random scalars, on a subgroup point and on the point of order 11 (the window
    additions meet acc = +-q) and on the base (0, 0)."""
    rep = _check(runs, "g1mul")
    assert rep.compared == {"g1mul": 263}


def test_curve28_g1h28(runs):
    """g1h28_load (exact), g1h28_add (r fresh, r = a, r = b: the same words) against the complete
    addition restated, g1h28_store (canonical, infinity all-zero)."""
    rep = _check(runs, "g1h28")
    assert rep.compared == {"g1h_load": 8, "g1h_add": 37, "g1h_add_ra": 37, "g1h_add_rb": 37, "g1h_store": 12}
    _, disagree = V.group_disagreements(runs["interleaved"][0], rep)
    assert not disagree, disagree[:4]


def test_curve28_interleaved_equals_sorted(runs):
    """The same case returns the same words whether its wave's other lanes run other ops and
    branches (interleaved) or the same one (sorted)."""
    a = V.compare(*runs["interleaved"][:2])
    b = V.compare(*runs["sorted"][:2])
    assert a.total() == b.total() == len(runs["interleaved"][0]) == len(runs["sorted"][0]) == 1280
    assert set(a.words) == set(b.words)
    diff = [i for i in a.words if a.words[i] != b.words[i]]
    assert not diff, "%d cases differ between the orders, first ids %s" % (len(diff), diff[:8])
    assert a.ok and b.ok, a.text() + " / " + b.text()
    assert set(a.compared) == set(V.OPS)


def test_curve28_ragged_tail(runs):
    """101 cases, every op among them: the last wave holds 37 lanes, the rest return early."""
    cases, out, _ = runs["ragged"]
    assert len(cases) % 64 == 37 and {c.op for c in cases} == set(V.OPS)
    rep = V.compare(cases, out)
    assert rep.total() == len(cases) and rep.ok, rep.text()


def test_curve28_gpu_bytes_equal_host_bytes(runs):
    """The device products return the integers the host products return and every other step is
    the same code, so each order's OUT file equals the --host OUT file byte for byte: no op is
    excluded."""
    for name, (cases, out, host) in runs.items():
        assert len(out) == len(host) == sum(c.out_bytes() for c in cases)
        if out != host:
            a, b = V.compare(cases, out), V.compare(cases, host)
            diff = sorted({c.op for c in cases if a.words[c.id] != b.words[c.id]})
            raise AssertionError("%s: GPU and host words differ in ops %s" % (name, diff))
