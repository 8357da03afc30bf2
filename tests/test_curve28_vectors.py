"""CPU: the case generator, the restated formulas and the comparator of the radix-2^28 curve
checker (tools/ubench/curve28_vectors.py, tests/test_gpu_curve28.py) are themselves right.

* every case class the GPU tests rely on is there, with its count;
* the restated formulas agree with oracle/bls12_381.py's group law as points (add, double, negate,
  psi, the [|x|] chain, membership, Budroni-Pintore clearing, the windowed scalar multiplication,
  the complete homogeneous addition), and the 68 restated line coefficients, evaluated at a G1
  point and multiplied through, give the oracle's pairing after the final exponentiation;
* the comparator passes a model output and sees a flipped low bit, the same residue plus p, a
  limb at 2^28, a word changed past a result and a wrong boolean, each under its own case;
* the checker cross-compiles, and its host mode (the headers' plain-C branches) passes every case
  of the interleaved and ragged orders."""
import os
import re
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import curve28_vectors as V  # noqa: E402
from oracle import bls12_381 as O  # noqa: E402

P = V.P
assert P == O.P and V.X_ABS == O.X_ABS


@pytest.fixture(scope="module")
def orders():
    return V.build_orders()


@pytest.fixture(scope="module")
def cases(orders):
    return orders[0]


def _classes(cases):
    n = {}
    for c in cases:
        n.setdefault(c.op, {}).setdefault(c.cls, 0)
        n[c.op][c.cls] += 1
    return n


def test_constants_are_the_header_s():
    src = open(os.path.join(ROOT, "grandine_amd", "csrc", "bls_r28_consts.h")).read()

    def const(name):
        body = re.search(r"constexpr fe %s = \{\{([^}]*)\}\}" % name, src).group(1)
        return [int(x.strip().rstrip("u"), 16) for x in body.split(",")]

    val = lambda name: V.int_of(const(name)) * V.RINV % P
    assert const("K28_ONE") == V.ONE_L and val("K28_ONE") == 1
    assert V.PSI_CX == (0, val("K28_PSI_CX1")) and V.PSI_CY == (val("K28_PSI_CY0"), val("K28_PSI_CY1"))
    assert V.PSI2_CX == val("K28_PSI2_CX") and V.PSI2_CY == val("K28_PSI2_CY") == P - 1
    assert tuple(O.PSI_CX) == V.PSI_CX and tuple(O.PSI_CY) == V.PSI_CY
    hdr = open(os.path.join(ROOT, "grandine_amd", "csrc", "bls_curve28.h")).read()
    for text in ("input coordinates normalized and < 2.1 p; X3, Y3 < 1.03 p, Z3 normalized and\n// < 2.03 p",
                 "a normalized, < 1.03 p", "a normalized, < 4 p", "coordinates normalized, < 1.03 p",
                 "Coordinates stay normalized and < 1.03 p"):
        assert text in hdr, text
    assert V.IN_POINT == 21 * P // 10 and (V.B_F, V.B_Z2) == (103, 203)
    assert sum(V.EV_DBL) == 63 and len(V.EV_DBL) == 68 and [i for i, d in enumerate(V.EV_DBL) if not d] == [1, 4, 8, 18, 51]


def test_case_classes_and_counts(cases):
    n = _classes(cases)
    assert set(n) == set(V.OPS) == set(V.FUNC_OF) and len(cases) == sum(sum(d.values()) for d in n.values())
    for op in ("g2_dbl", "g2_dbl_rp", "g1_dbl", "g1_dbl_rp"):
        assert n[op] == {"random": 8, "top": 8, "top all": 1, "top full": 1, "inf Z=0": 1, "inf Z=p": 1, "inf Z=2p": 1}
    inf6 = {"a inf Z=0": 1, "a inf Z=p": 1, "a inf Z=2p": 1, "b inf Z=0": 1, "b inf Z=p": 1, "b inf Z=2p": 1}
    for op in ("g1_add", "g1_add_ra"):
        assert n[op] == dict({"random": 8, "top": 8, "top all": 1, "top full": 1, "dbl branch": 6, "neg branch": 6,
                              "both inf": 3}, **inf6)
    pre = {"clear pre Q0 + Q1": 6, "clear pre Q0 = Q1": 1, "clear pre Q0 = -Q1": 1, "clear pre Q0 inf": 1,
           "clear pre Q1 inf": 1}
    for op in ("g2_add", "g2_add_ra"):
        assert n[op] == dict({"random": 8, "top": 8, "top all": 1, "top full": 1, "dbl branch": 6, "neg branch": 6,
                              "both inf": 3}, **inf6, **pre)
    for op in ("g2_madd_t", "g2_madd_t_ra"):
        assert n[op] == {"random": 8, "top": 8, "top all": 1, "top full": 1, "dbl branch": 6, "neg branch": 6,
                         "a inf Z=0": 1, "a inf Z=p": 1, "a inf Z=2p": 1, "b aff00": 1, "b aff00 p": 2,
                         "a inf b aff00": 3}
    for op in ("g2_madd_f", "g2_madd_f_ra"):
        assert n[op] == {"random": 8, "top": 8, "top all": 1, "top full": 1, "dbl branch": 6, "neg branch": 6,
                         "a inf Z=0": 1, "a inf Z=p": 1, "a inf Z=2p": 1}
    for op in ("g1h_add", "g1h_add_ra", "g1h_add_rb"):
        assert n[op] == dict({"random": 8, "top": 8, "top full": 1, "dbl branch": 4, "neg branch": 4, "both inf": 3,
                              "a zero": 3}, **inf6)
    for op in ("g2_eq", "g1_eq"):
        assert n[op] == {"equal": 6, "different": 6, "negated": 6, "inf finite": 3, "finite inf": 3, "inf inf": 3,
                         "zero finite": 3, "finite zero": 3}
    small = {"small order %d" % q: 3 for q in (13, 23, 2713, 11953)}
    assert n["in_group"] == dict({"in group": 8, "map output": 6}, **small)
    assert n["xabs"] == dict({"in group": 8, "map output": 6, "aff00": 1, "aff00 p": 2, "clear Q0 + Q1": 6,
                              "clear Q0 = Q1": 1, "clear Q0 = -Q1": 1, "clear Q0 inf": 1, "clear Q1 inf": 1}, **small)
    for op in ("clear_mid", "clear_post", "clear_staged", "clear_full"):
        assert n[op] == {"Q0 + Q1": 6, "Q0 = Q1": 1, "Q0 = -Q1": 1, "Q0 inf": 1, "Q1 inf": 1}
    assert n["g1mul"] == {"digit": 171, "random": 64, "fixed order 11": 10, "fixed in group": 10, "base 00": 4,
                          "all 4 order 11": 1, "all 5 order 11": 1, "all 4 in group": 1, "all 5 in group": 1}
    assert n["line_dbl"] == n["line_add"] == {"random": 8, "top": 8, "top all": 2, "top full": 1}
    assert n["line_chain"] == {"random": 6, "top all": 2}
    assert n["half"] == {"odd": 5, "even": 5, "0": 1, "1": 1, "p-1": 1, "p": 1, "top": 1, "top even": 1,
                         "full limbs": 1, "full limbs even": 1} and sum(n["fe2_half"].values()) == 18
    assert n["mul_3b"] == {"random": 4, "top": 4, "top full": 2}
    for op in ("g2_neg", "g1_neg", "psi2"):
        assert n[op] == {"random": 8, "top": 8, "top all": 1, "top full": 1}
    assert n["psi"]["inf Z=p"] == 1 and n["to_aff"]["inf Z=2p"] == 1 and n["of_aff"]["aff00 p"] == 2
    assert set(V.DEGENERATE) == {cls for op in ("g2_add", "g2_madd_t", "g1_add") for cls in n[op]
                                 if ("inf" in cls or "branch" in cls or "aff00" in cls) and "clear" not in cls}
    assert V.UNDEFINED == ()


def test_inputs_are_inside_the_contract(cases):
    """Raw operand limbs are normalized and below the routine's input bound; the top classes reach
    it (a coordinate within p of the bound, full limbs in the 'top full' cases)."""
    bound = {"line_dbl": V.IN_LINE_T, "line_add": V.IN_LINE_T, "line_chain": V.IN_LINE_T, "g1h_add": V.IN_LINE_T,
             "g1h_add_ra": V.IN_LINE_T, "g1h_add_rb": V.IN_LINE_T, "g1h_store": V.IN_LINE_T, "half": V.IN_LINE_T,
             "fe2_half": V.IN_LINE_T, "mul_3b": V.IN_3B, "store12": V.R384, "inv": 16 * P}
    engine = ("load12", "g2j_in", "g1h_load", "g1mul")
    reached = {}
    for c in cases:
        if c.op in engine:
            continue
        b = bound.get(c.op, V.IN_POINT)
        fes = V._fes(c.words)
        if c.op in ("line_dbl", "line_add"):
            fes = fes[:6]   # T; Q is a product operand (normalized, < 5 p)
        for l in fes:
            # a zero given as 2p (an infinite g1h28 point's c) is above the 1.03 p of a finite coordinate
            zero2p = V.int_of(l) == 2 * P and ("inf" in c.cls or "zero" in c.cls)
            assert max(l) <= V.M28 and (V.int_of(l) < b or zero2p), (c.op, c.cls)
        if c.cls.startswith("top"):
            reached[c.op] = max(reached.get(c.op, 0), max(V.int_of(l) for l in fes) + P >= b)
        if c.cls == "top full":
            assert any(l[:13] == [V.M28] * 13 for l in fes), c.op
    assert all(reached.values()) and len(reached) >= 24, reached
    # all coordinates at their largest representative in the 'top all' point cases
    for c in cases:
        if c.cls == "top all" and V.FUNC_OF[c.op] in ("jac_dbl28", "jac_add28", "jac_add_aff28"):
            assert all(V.int_of(l) + P >= V.IN_POINT for l in V._fes(c.words)), c.op


def test_scalars_of_the_windowed_multiplication(cases):
    g = [c for c in cases if c.op == "g1mul"]
    ks = {c.cls: [] for c in g}
    for c in g:
        ks[c.cls].append(c.scalar)
        assert c.record()[2] | c.record()[3] << 32 == c.scalar < 1 << 64
    assert sorted(ks["fixed order 11"]) == sorted(ks["fixed in group"]) == [0, 1, 2, 3, 4, 5, 7, 8, 1 << 63, (1 << 64) - 1]
    assert V.signed_digits(V.K_ALL4) == [4] * 21 + [0] and [(V.K_ALL4 >> 3 * i) & 7 for i in range(21)] == [4] * 21
    d5 = V.signed_digits(V.K_ALL5)
    assert [(V.K_ALL5 >> 3 * i) & 7 for i in range(21)] == [5] * 21 and d5 == [-3] + [-2] * 20 + [2]
    seen = set()
    for k in ks["digit"]:
        d = V.signed_digits(k)
        assert sum(x * 8 ** i for i, x in enumerate(d)) == k
        seen |= {(i, x) for i, x in enumerate(d)}
    assert seen >= {(i, x) for i in range(21) for x in range(-3, 5)} | {(21, 0), (21, 1), (21, 2)}
    # the order-11 base: some window addition meets acc = +-q (the doubling or the infinity branch)
    t11 = V.g1_rec(next(e for e in V.gold("small_order")["e1"] if e["order"] == 11)["T"])
    assert O.g1_mul(t11, 11) is None and O.g1_on_curve(t11)
    hits = 0
    for c in g:
        if V.int12(c.words[:12]) * V.R384INV % P == t11[0]:
            d = V.signed_digits(c.scalar)
            acc = d[21]
            for i in range(20, -1, -1):
                acc = acc * 8 % 11
                if d[i] and acc in (d[i] % 11, -d[i] % 11):  # acc = q: doubling; acc = -q: infinity
                    hits += 1
                acc = (acc + d[i]) % 11
    assert hits >= 20


def _g(K):
    return (O.g1_add, O.g1_mul, O.g1_neg) if K is V.K1 else (O.g2_add, O.g2_mul, O.g2_neg)


def _t(pt):
    return None if pt is None else tuple(tuple(c) if isinstance(c, (tuple, list)) else c for c in pt)


def _hom_aff(K, T):
    if K.is_zero(T[2]):
        return None
    zi = K.inv(T[2])
    return (K.mul(T[0], zi), K.mul(T[1], zi))


def test_restated_formulas_agree_with_the_oracle_s_group_law(cases):
    seen = {}
    for c in cases:
        if c.oracle is None:
            continue
        (kind, *args), K, res = c.oracle
        add, mul, neg = _g(K)
        seen[kind] = seen.get(kind, 0) + 1
        if kind == "dbl":
            assert V.aff_of(K, res) == _t(add(args[0], args[0])), (c.op, c.cls)
        elif kind == "neg":
            assert V.aff_of(K, res) == _t(neg(args[0]))
        elif kind == "id":
            assert V.aff_of(K, res) == _t(args[0])
        elif kind == "psi":
            assert V.aff_of(K, res) == _t(O.g2_psi(args[0]))
        elif kind == "psi2":
            assert V.aff_of(K, res) == _t(O.g2_psi(O.g2_psi(args[0])))
        elif kind == "add":
            assert V.aff_of(K, res) == _t(add(args[0], args[1])), (c.op, c.cls)
        elif kind == "mul":
            assert V.aff_of(K, res) == _t(mul(args[0], args[1])), (c.op, c.cls)
        elif kind == "in_group":
            want = O.g2_mul(args[0], O.R) is None
            assert c.items == [("exact", [1 if want else 0])], c.cls
            assert want == (c.cls == "in group")
        elif kind == "hdbl":
            assert _hom_aff(K, res) == _t(add(args[0], args[0]))
        elif kind == "hadd":
            assert _hom_aff(K, res) == _t(add(args[0], args[1]))
        elif kind == "hadd1":
            assert _hom_aff(K, [co.v for co in res]) == _t(add(args[0], args[1])), c.cls
        elif kind == "mid":
            t2a, T = res
            pp = args[0]
            want_t2 = O.g2_add(O.g2_mul(pp, O.X), O.g2_psi(pp))
            got_t2 = None if V.aff_is_inf(V.K2, t2a) else (t2a[0].v, t2a[1].v)
            assert got_t2 == _t(want_t2)
            want_T = O.g2_add(O.g2_add(O.g2_mul(pp, O.X_ABS - 1), O.g2_psi(O.g2_psi(O.g2_add(pp, pp)))),
                              O.g2_neg(O.g2_psi(pp)))
            assert V.aff_of(K, T) == _t(want_T)
        elif kind == "clear":
            assert V.aff_of(K, res) == _t(O.clear_cofactor_g2_bp(args[0])), (c.op, c.cls)
        elif kind == "chain":
            assert _hom_aff(K, res[1]) == _t(O.g2_mul(args[0], O.X_ABS))
    assert seen == {"dbl": 68, "neg": 34, "id": 17, "psi": 17, "psi2": 17, "add": 312, "mul": 299, "in_group": 26,
                    "hdbl": 18, "hadd": 18, "hadd1": 108, "mid": 10, "clear": 30, "chain": 8}, seen
    # the clearing equals the plain multiplication by h_eff on one case
    c = next(c for c in cases if c.op == "clear_staged" and c.cls == "Q0 + Q1")
    assert V.aff_of(V.K2, c.oracle[2]) == _t(O.clear_cofactor_g2(c.oracle[0][1]))


def test_restated_lines_give_the_oracle_s_pairing(cases):
    """The 68 coefficient triples of one chain case as sparse elements L0 + L2 xP w^2 + L3 yP w^3,
    squared and multiplied through as the Miller loop does, conjugated (x < 0): equal to the
    oracle's pairing after the final exponentiation (the lines differ by Fp2 factors only)."""
    c = next(c for c in cases if c.op == "line_chain")
    (_, q), _, (Ls, _) = c.oracle
    g1 = O.g1_mul(O.G1_GEN, 0x1234567)
    f = O.f12_one()
    z = (0, 0)
    for dbl, (L0, L2, L3) in zip(V.EV_DBL, Ls):
        line = [L0, z, O.f2_muls(L2, g1[0]), O.f2_muls(L3, g1[1]), z, z]
        f = O.f12_mul(O.f12_sqr(f), line) if dbl else O.f12_mul(f, line)
    assert O.f12_eq(O.final_exp(O.f12_conj(f)), O.pairing(g1, q))
    # and the recorded residues are those coefficients in the 2^392 form
    want = [x * V.R % P for L in Ls for co in L for x in co]
    assert [it[1] for it in c.items[:len(want)]] == want and all(it[2] == 103 * P // 100 for it in c.items)


def test_files_layout_and_interleaving(orders, tmp_path):
    inter, srt, ragged = orders
    assert sorted(c.id for c in inter) == sorted(c.id for c in srt) and len({c.id for c in inter}) == len(inter) == 1280
    path = str(tmp_path / "interleaved.bin")
    V.write_cases(path, inter)
    assert os.path.getsize(path) == 4 + 4 * V.IN_WORDS * len(inter)
    raw = open(path, "rb").read()
    for i in (0, 77, len(inter) - 1):
        w = struct.unpack_from("<%dI" % V.IN_WORDS, raw, 4 + 4 * V.IN_WORDS * i)
        c = inter[i]
        assert w[0] == V.OPS[c.op] and w[1] == 0 and list(w[4:4 + len(c.words)]) == c.words
        assert not any(w[4 + len(c.words):])
    degenerate = lambda c: c.cls in V.DEGENERATE or c.cls.startswith(("inf", "zero", "small order"))
    for w in range(0, len(inter), 64):
        wave = inter[w:w + 64]
        assert len({c.op for c in wave}) >= 16 and any(degenerate(c) for c in wave) and \
            any(c.cls == "random" for c in wave), w
    mixed = sum(1 for w in range(0, len(srt), 64) if len({c.op for c in srt[w:w + 64]}) > 1)
    assert mixed <= len(V.OPS) and sum(1 for w in range(0, len(srt), 64) if len({c.op for c in srt[w:w + 64]}) == 1) >= 4
    assert len(ragged) == 101 and len(ragged) % 64 == 37 and {c.id for c in ragged} <= {c.id for c in inter}
    assert {c.op for c in ragged} == set(V.OPS)


def test_comparator(cases):
    model = V.model_output(cases)
    rep = V.compare(cases, model)
    assert rep.ok and rep.total() == len(cases) and "no mismatch" in rep.text()
    with pytest.raises(AssertionError):
        V.compare(cases, model[:-4])
    offs, o = {}, 0
    for c in cases:
        offs[c.id] = o
        o += c.out_bytes()
    first = {}
    for c in cases:
        first.setdefault(c.op, c)

    def only(bad, c):
        rep = V.compare(cases, bytes(bad))
        assert not rep.ok and rep.ops_failed() == [c.op], (c.op, rep.text())
        assert [x[0] for x in rep.mismatch[(c.op, c.cls)]] == [c.id]
        assert V.compare(cases, bytes(bad), ops={op for op in V.OPS if op != c.op}).ok
        return rep.text()

    for i, (op, c) in enumerate(sorted(first.items())):  # a flipped low bit of one word of one case
        bad = bytearray(model)
        bad[offs[c.id] + 4 * (i % c.out_words())] ^= 1
        only(bad, c)
        # a word changed past the result: the case after it fails, this one does not
        nxt = next((d for d in cases if offs[d.id] == offs[c.id] + c.out_bytes()), None)
        if nxt is not None and nxt.op != c.op:
            bad = bytearray(model)
            bad[offs[nxt.id]] ^= 1
            only(bad, nxt)
    # a residue item: the same residue plus p (above 1.03 p), and a limb at 2^28
    for op in ("g2_add", "g1_dbl", "line_add", "clear_full", "xabs", "g1h_add_rb"):
        c = next(c for c in cases if c.op == op and c.cls == "random" or c.op == op and c.cls.endswith("Q0 + Q1"))
        k, o = next((k, sum(len(j[1]) if j[0] == "exact" else 14 for j in c.items[:k]))
                    for k, it in enumerate(c.items) if it[0] == "res" and it[1] > P // 10)
        bad = bytearray(model)
        bad[offs[c.id] + 4 * o:offs[c.id] + 4 * o + 56] = V.pack_words(V.limbs_of(c.items[k][1] + (2 if k % 3 == 2 and op == "g1_dbl" else 1) * P))
        assert "bound" in only(bad, c)
        l = V.limbs_of(c.items[k][1])
        if l[1] == 0:
            l = V.limbs_of(c.items[k][1] + P)
        l[0] += 1 << 28
        l[1] -= 1
        bad = bytearray(model)
        bad[offs[c.id] + 4 * o:offs[c.id] + 4 * o + 56] = V.pack_words(l)
        assert ">= 2^28" in only(bad, c)
    for op in ("g2_eq", "g1_eq", "in_group"):  # a wrong boolean
        for c in [c for c in cases if c.op == op][:6]:
            bad = bytearray(model)
            bad[offs[c.id]] ^= 1
            only(bad, c)
    # aliasing groups: r fresh and r aliased return the same words
    rep = V.compare(cases, model)
    by, disagree = V.group_disagreements(cases, rep)
    assert not disagree and len(by) > 200
    c = first["g2_add_ra"]
    bad = bytearray(model)
    bad[offs[c.id]] ^= 1
    _, disagree = V.group_disagreements(cases, V.compare(cases, bytes(bad)))
    assert disagree == [(c.group, ["g2_add", "g2_add_ra"])]


def test_checker_cross_compiles_and_its_host_mode_passes(orders, tmp_path):
    """The host branches of the headers through the same checker and file layout: every case of
    the interleaved and the ragged order, exact words, residues, limbs and bounds."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "ubench"), "-s"])
    exe = os.path.join(ROOT, "tools", "ubench", "_bin", "curve28_check")
    assert os.path.exists(exe)
    inter, _, ragged = orders
    for name, cs in (("interleaved", inter), ("ragged", ragged)):
        src, dst = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".out"))
        V.write_cases(src, cs)
        r = subprocess.run([exe, "--host", src, dst], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rep = V.compare(cs, open(dst, "rb").read())
        assert rep.ok, rep.text()
        assert rep.total() == len(cs) and set(rep.compared) == {c.op for c in cs}
        _, disagree = V.group_disagreements(cs, rep)
        assert not disagree, disagree[:4]
