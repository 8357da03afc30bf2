"""CPU: the case generator, the integer reference and the comparator of the quad / row gang
checker (tools/ubench/gang_vectors.py, tests/test_gpu_gang.py) are themselves right: on every
on-curve case the reference agrees with the oracle's group law, the written file holds the
cases and the wave layout it promises, and the comparator sees a single flipped limb of a single
lane, under the right op."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
import gang_vectors as V  # noqa: E402

O = V.O
P = O.P

# words per lane and words written before the lanes' blocks (from lane 0), per op
PER = {"q_fp2mul": 24, "q_fp2mul_ra": 24, "q_fp2mul_rb": 24, "q_fp2mul_aa": 24, "q_dbl": 72, "q_dbl_rp": 72,
       "q_add": 72, "q_add_ra": 72, "q1_dbl": 36, "q1_dbl_rp": 36, "q1_add": 36, "q1_add_ra": 36,
       "q_line_dbl": 144, "q_line_add": 144, "q_xabs": 72, "q_g1mul": 72, "q_g2mul": 72,
       "q_lines": 68 * 72 + 72, "r_mul4": 96, "r_mul4_alias": 96, "r_mul4_txxx": 48, "r_dbl": 72,
       "r_dbl_rp": 72, "r_add": 72, "r_add_ra": 72, "r_line_dbl": 144, "r_line_add": 144, "r_xabs": 72,
       "r_lines": 68 * 72 + 72}
PRE = {"q_xabs": 68 * 72, "r_xabs": 68 * 72}


@pytest.fixture(scope="module")
def orders():
    return V.build_orders()


@pytest.fixture(scope="module")
def cases(orders):
    return orders[0]


def test_images_round_trip():
    assert V.val(V.ONE_W) == 1 and V.img(1) == V.ONE_W and V.val(V.img(P - 1)) == P - 1
    x = 0x123456789abcdef0fedcba9876543210 << 200 | 77
    assert V.int_of_words(V.words_of_int(x)) == x and V.words_of_int(x)[0] == 77
    assert V.Fp2.enc(V.Fp2.dec([5, V.ONE_W])) == [5, V.ONE_W]
    assert V.inf_image(V.Fp1) == [V.ONE_W, V.ONE_W, 0]
    assert sum(V.EVENTS) == 63 and len(V.EVENTS) == 68 and V.EVENTS[0] and not V.EVENTS[1]


def test_reference_agrees_with_the_oracle_group_law(cases):
    """Every case whose operands are curve points: doublings, sums, [|x|]P, [k]P and the new T
    as affine points, the lines proportional to (lambda x_T - y_T, -lambda, 1)."""
    seen = {}
    for c in cases:
        errs = V.oracle_check(c)
        if errs is None:
            continue
        assert not errs, (c.op, c.cls, c.id, errs)
        assert c.cls != "random" and "off curve" not in c.cls
        fn = V.FUNC_OF[c.op]
        seen[fn] = seen.get(fn, 0) + 1
    assert set(seen) == set(V.FUNCS) - {"gang_fp2_mul", "row_mul4"}
    for fn, n in seen.items():
        floor = {"gang_mul_by_xabs": 3, "row_mul_by_xabs": 3, "k_lines": 3, "k_lines_row": 3,
                 "k_mv_g1mul": 14, "k_mv_g2mul": 28}.get(fn, 16)
        assert n >= floor, (fn, n)
    # the labels say what the points are: every "gen" / "offsub" case above was on the curve, and
    # the pools are in / outside the subgroup
    pts = V.Points(2300)
    assert all(O.g2_in_group(p) for p in pts.g2[:4]) and all(O.g1_in_group(p) for p in pts.g1[:4])
    assert all(O.g2_on_curve(p) and not O.g2_in_group(p) for p in pts.off[:4])
    assert all(O.g2_on_curve(p) for p in pts.off + pts.g2)


def test_reference_against_the_oracle_on_special_cases():
    """The degenerate branches as group elements: a + a = 2a also across representations,
    a - a = O, O + b = b; and the reference's Fp2 is the oracle's."""
    import random
    rng = random.Random(5)
    pts = V.Points(7, n=4)
    for F in (V.Fp1, V.Fp2):
        pt = pts.pick(F, 0)[0]
        a = V.jac_of(F, pt, V.rnd_elem(F, rng))
        b = V.rescale(F, a, V.rnd_elem(F, rng))
        r, o = V.add_image(F, a, b)
        assert o == "dbl" and r == V.dbl_image(F, b) and r != V.dbl_image(F, a)
        assert V._jac_affine(F, r) == F.oadd(pt, pt) == V._jac_affine(F, V.dbl_image(F, a))
        assert V.add_image(F, a, V.rescale(F, a, V.rnd_elem(F, rng), neg=True)) == (V.inf_image(F), "inf")
        inf = [P + 5] * (2 * F.N) + [0] * F.N
        assert V.add_image(F, inf, b) == (b, "copy") and V.add_image(F, a, inf) == (a, "copy")
        assert V.add_image(F, inf, inf) == (inf, "copy")
    x, y = (rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P))
    assert V.Fp2.mul(x, y) == O.f2_mul(x, y) and V.Fp2.mul(x, V.Fp2.inv(x)) == (1, 0)
    assert V.Fp2.mul(V.B3, x) == O.f2_muls(O.f2_mul(O.B2, x), 3)


def test_case_counts(cases):
    by = {}
    for c in cases:
        by.setdefault(V.FUNC_OF[c.op], []).append(c)
    assert set(by) == set(V.FUNCS)
    n = lambda fn, pred: sum(1 for c in by[fn] if pred(c))
    for fn in ("gang_fp2_mul", "row_mul4", "gang_dbl", "row_dbl", "gang_add", "row_add", "gang1_dbl", "gang1_add",
               "gang_line_dbl", "gang_line_add_aff", "row_line_dbl", "row_line_add_aff"):
        assert n(fn, lambda c: c.cls == "random") >= 32, fn
        assert n(fn, lambda c: c.cls == "edge") >= 8, fn
        for form in V.FUNCS[fn]:  # every form gets its share
            assert n(fn, lambda c: c.op == form and c.cls == "random") >= 16, form
    for fn in ("gang_dbl", "row_dbl", "gang_add", "row_add", "gang_line_dbl", "gang_line_add_aff", "row_line_dbl",
               "row_line_add_aff"):
        assert n(fn, lambda c: c.cls.startswith("gen")) >= 8 and n(fn, lambda c: c.cls.startswith("offsub")) >= 8, fn
    for fn in ("gang1_dbl", "gang1_add"):
        assert n(fn, lambda c: c.cls == "gen") >= 16, fn
    for fn in ("gang_dbl", "row_dbl", "gang1_dbl"):
        for form in V.FUNCS[fn]:
            assert n(fn, lambda c: c.op == form and c.cls == "Y=0") >= 1
            assert n(fn, lambda c: c.op == form and c.cls == "infinite") >= 1
    for fn in ("gang_add", "row_add", "gang1_add"):
        for form in V.FUNCS[fn]:
            for classes in V.DEGENERATE.values():
                for cls in classes:
                    assert n(fn, lambda c: c.op == form and c.cls == cls) >= 1, (form, cls)
    for fn in ("gang_line_dbl", "row_line_dbl", "gang_line_add_aff", "row_line_add_aff"):
        assert n(fn, lambda c: c.cls.endswith("Z=1")) >= 4
    for fn in ("gang_line_add_aff", "row_line_add_aff"):
        assert n(fn, lambda c: c.cls == "theta=lambda=0") >= 4
    for fn in ("gang_mul_by_xabs", "row_mul_by_xabs", "k_lines", "k_lines_row"):
        assert len(by[fn]) == 4
    for fn, per_k in (("k_mv_g1mul", 1), ("k_mv_g2mul", 2)):
        ks = [c.k for c in by[fn] if c.cls.startswith(("gen", "offsub"))]
        for k in V.SCALARS:
            assert ks.count(k) == per_k, (fn, hex(k))  # G2: both halves
        assert len(set(ks) - set(V.SCALARS)) >= 8
    # the low half of 2^32 is zero: the identity comes out
    c = next(c for c in by["k_mv_g2mul"] if c.k == 1 << 32 and c.aux == 0)
    assert c.pre == b"" and c.per == V.pack(V.inf_image(V.Fp2))


def test_edge_operands_are_what_they_claim():
    import random
    rng = random.Random(3)
    assert V.edge_operands(rng, 4, 2) == [P - 1] * 4  # c0 = c1 = p - 1: the lazy sum is 2p - 2
    assert V.edge_operands(rng, 4, 0) == [0] * 4 and V.edge_operands(rng, 4, 1) == [V.ONE_W] * 4
    e = V.edge_operands(rng, 6, 3)
    assert e[0] == e[2] == e[4] == 0 and all(e[1::2])
    e = V.edge_operands(rng, 6, 4)
    assert e[1] == e[3] == e[5] == 0 and all(e[0::2])
    assert all(w < P for j in range(8) for w in V.edge_operands(rng, 16, j))
    for fam in ("q", "q1", "r"):  # arbitrary words really leave the canonical range
        c = V.degenerate_add(fam, "copy", 0, rng, V.Points(9, n=4))
        assert c.cls == "a inf" and c.ws[0] == (1 << 384) - 1
        c = V.degenerate_add(fam, "copy", 2, rng, V.Points(9, n=4))
        assert c.cls == "both inf" and c.per == V.pack(c.ws[:len(c.ws) // 2])


def test_files_layout_and_interleaving(orders, tmp_path):
    inter, srt, ragged = orders
    assert sorted(c.id for c in inter) == sorted(c.id for c in srt) and len({c.id for c in inter}) == len(inter)
    path = str(tmp_path / "interleaved.bin")
    V.write_cases(path, inter)
    assert V.IN_WORDS == 196 and os.path.getsize(path) == 4 + 4 * 196 * len(inter)
    recs = V.read_cases(path)
    assert len(recs) == len(inter) <= 1 << 16
    # the rule, from the file alone: outcomes recomputed from the records
    outcomes = {False: [], True: []}
    for (op, aux, k, ws), c in zip(recs, inter):
        assert (op, aux, k) == (c.op, c.aux, c.k) and ws[:len(c.ws)] == c.ws and not any(ws[len(c.ws):])
        pre, per, outcome = V.expect(op, aux, k, ws)
        assert (pre, per, outcome) == (c.pre, c.per, c.outcome)
        outcomes[V.is_row(op)].append(outcome)
    for row, size in ((False, 16), (True, 4)):
        seq = outcomes[row]
        assert len(seq) >= 4 * size
        for w in range(0, len(seq), size):
            assert set(seq[w:w + size]) == set(V.OUTCOMES), (row, w)
    # the sorted order's waves are uniform except where an op or outcome ends
    for row, size in ((False, 16), (True, 4)):
        seq = [(c.op, c.outcome) for c in srt if V.is_row(c.op) == row]
        mixed = sum(1 for w in range(0, len(seq), size) if len(set(seq[w:w + size])) > 1)
        assert mixed <= len(set(seq))
    # ragged: both kernels end in a partly filled wave
    nq = sum(1 for c in ragged if not V.is_row(c.op))
    assert nq % 16 == 5 and (len(ragged) - nq) % 16 == 5 and (len(ragged) - nq) % 4 == 1


def test_out_layout_sizes(cases):
    for c in cases:
        pre = PRE.get(c.op, 0)
        if c.op in ("q_g1mul", "q_g2mul"):
            k = c.k if c.op == "q_g1mul" else ((c.k >> 32) if c.aux else c.k & 0xffffffff)
            steps = 0 if (k == 0 or not any(c.ws)) else k.bit_length() - 1 + bin(k).count("1") - 1
            pre = steps * (36 if c.op == "q_g1mul" else 72)
        assert len(c.pre) == 4 * pre and len(c.per) == 4 * PER[c.op], c.op
        assert c.out_bytes() == 4 * (pre + (16 if V.is_row(c.op) else 4) * PER[c.op])
    assert set(PER) == set(V.OPS)


def test_comparator(cases):
    model = V.model_output(cases)
    rep = V.compare(cases, model)
    assert rep.ok and rep.total() == len(cases) and "mismatches by op: none" in rep.text()
    with pytest.raises(AssertionError):
        V.compare(cases, model[:-4])
    offs, o = {}, 0
    for c in cases:
        offs[c.id] = o
        o += c.out_bytes()
    first = {}
    for c in cases:
        first.setdefault(c.op, c)
    assert set(first) == set(V.OPS)
    for i, (op, c) in enumerate(sorted(first.items())):  # one limb of one lane of one case
        lane = i % V.lanes(op)
        at = offs[c.id] + len(c.pre) + lane * len(c.per) + 4 * (i % (len(c.per) // 4))
        bad = bytearray(model)
        bad[at] ^= 1 << (i % 8)
        rep = V.compare(cases, bytes(bad))
        assert not rep.ok and rep.ops_failed() == [op], (op, rep.text())
        assert list(rep.mismatch) == [(op, c.cls)] and rep.mismatch[(op, c.cls)] == [c.id]
        assert list(rep.lanes) == [(op, c.cls)]
        assert V.compare(cases, bytes(bad), ops={o for o in V.OPS if o != op}).ok
    # only the last lane of a gang differs
    for op, lane in (("q_add", 3), ("r_add", 15), ("q1_dbl", 3), ("r_line_dbl", 15)):
        c = first[op]
        bad = bytearray(model)
        bad[offs[c.id] + len(c.pre) + lane * len(c.per) + 5] ^= 0x80
        rep = V.compare(cases, bytes(bad))
        assert rep.lanes == {(op, c.cls): [c.id]} and rep.mismatch == {(op, c.cls): [c.id]}
        assert "lanes of a gang disagree: %s" % op in rep.text()
    # all lanes wrong in the same way: a mismatch, and the lanes agree
    c = first["q_dbl"]
    bad = bytearray(model)
    for lane in range(4):
        bad[offs[c.id] + lane * len(c.per)] ^= 1
    rep = V.compare(cases, bytes(bad))
    assert not rep.lanes and rep.mismatch == {("q_dbl", c.cls): [c.id]}
    # an intermediate of a chain (written from lane 0 only)
    c = first["r_xabs"]
    bad = bytearray(model)
    bad[offs[c.id] + 17 * 288 + 3] ^= 4
    rep = V.compare(cases, bytes(bad))
    assert not rep.lanes and rep.mismatch == {("r_xabs", c.cls): [c.id]}


def test_checker_cross_compiles():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "ubench"), "-s"])
    assert os.path.exists(os.path.join(ROOT, "tools", "ubench", "_bin", "gang_check"))
