"""CPU: the case generator, the integer reference and the comparator of the radix-2^28 field
checker (tools/ubench/field28_vectors.py, tests/test_gpu_field28.py) are themselves right.

* every primitive case is inside its header contract, no modeled 64-bit accumulator overflows,
  every primitive has its top-of-contract case and fe2_mul3k cases that drive the signed
  accumulator negative;
* the exact value (T + m p) / 2^392 IS what the column loop returns, word for word, on every
  primitive case (mul_n of the header; the signed two-accumulator loop of the generator);
* the composite expectations agree with oracle/bls12_381.py field arithmetic, with the 2^-392,
  2^-16 and 2^8 scalings the header states;
* the committed bls_fpmul28_gen.h is what tools/gen_fpmul28.py writes;
* the checker's host mode (the header's plain-C branch) passes the comparator on the written
  file, and the comparator sees a single flipped bit under the right op."""
import math
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import field28_vectors as V  # noqa: E402
from oracle import bls12_381 as O  # noqa: E402

P = V.P
assert P == O.P


@pytest.fixture(scope="module")
def orders():
    return V.build_orders()


@pytest.fixture(scope="module")
def cases(orders):
    return orders[0]


@pytest.fixture(scope="module")
def prims(cases):
    return [c for c in cases if V.FUNC_OF[c.op] in V.PRIMITIVES]


def test_constants_are_the_header_s():
    src = open(os.path.join(ROOT, "grandine_amd", "csrc", "bls_field28.h")).read()

    def macro(name):
        body = src.split("#define " + name)[1].split("\n//")[0].replace("\\", " ")
        return [int(x, 16) for x in body.replace(",", " ").split()]

    assert macro("GBLS_R28_P") == V.P_L and V.int_of(V.P_L) == P
    assert macro("GBLS_R28_BIAS4P") == V.BIAS4P == V.make_bias(4, 1) and V.int_of(V.BIAS4P) == 4 * P
    assert macro("GBLS_R28_CIN") == V.limbs_of(V.CIN) and macro("GBLS_R28_COUT") == V.limbs_of(V.COUT)
    assert "kPinv = 0x%08x" % V.PINV28 in src and V.PINV28 * P % (1 << 28) == (1 << 28) - 1
    gen = open(os.path.join(ROOT, "tools", "gen_fpmul28.py")).read()
    assert "BIAS_KARA = 17 * P_INT * P_INT" in gen and "P_INT = %#x" % P in gen
    assert V.limbs_of(V.int_of(V.top_pattern(V.N11))) == V.top_pattern(V.N11)
    assert V.words12(V.int12(V.words12(P - 1))) == V.words12(P - 1)


def test_primitive_cases_are_inside_the_contract(prims):
    assert len(prims) > 3000
    for c in prims:
        assert V.in_contract(c), (c.op, c.cls, c.id)
    # and the contract check itself refuses what is outside: a limb at 2^29, a value at the bound
    c = next(c for c in prims if c.op == "mul6" and c.cls == "top")
    f = c.fes()
    assert f[0][:13] == [(1 << 28) - 1] * 13 and f[1][:13] == [(1 << 29) - 1] * 13
    assert V.int_of(f[0]) + (1 << V.TOP_SHIFT) >= 11 * P // 10 and V.int_of(f[1]) + (1 << V.TOP_SHIFT) >= 51 * P // 10
    assert not V.in_role(f[0][:13] + [f[0][13] + 1], V.N11) and not V.in_role([1 << 29] + [0] * 13, V.L51)


def test_accumulators_of_every_case_fit(prims):
    """The integer model of the column loop on the case list: nothing exceeds 64 bits unsigned
    (63 signed for fe2_mul3k's acc0), the peaks are the ones DESIGN.md records, reached by the
    top-of-contract cases, and acc0 is negative in the columns listed."""
    pk, neg = V.peaks(prims)
    assert set(pk) == set(V.PRIMITIVES)
    log = {fn: {k: math.log2(v) for k, (v, _) in d.items()} for fn, d in pk.items()}
    print("modeled peaks (log2):", log, "acc0 negative in columns", neg)
    for fn, d in pk.items():
        for name, (v, cls) in d.items():
            assert v < (1 << 63 if name == "acc0" else 1 << 64), (fn, name)
    for fn in ("mul", "sqr", "mul2", "mul4", "mul6"):
        assert pk[fn]["acc"][1] == "top", fn
    assert pk["fe2_mul3k"]["acc1"][1] == "top"
    assert abs(log["mul6"]["acc"] - 63.33) < 0.01 and abs(log["mul2"]["acc"] - 62.76) < 0.01
    assert abs(log["mul"]["acc"] - 61.82) < 0.01 and abs(log["mul4"]["acc"] - 62.76) < 0.01
    assert abs(log["fe2_mul3k"]["acc1"] - 63.29) < 0.01 and abs(log["fe2_mul3k"]["acc0"] - 61.44) < 0.01
    assert neg == list(range(27))
    # per class: the opposite-range operands go negative where B sits and A does not
    by = {c.cls: V.model(c)[2] for c in prims if c.op == "mul3k" and c.cls not in ("canon", "lazy", "special", "onehot")}
    assert by["A=0 B max"] == list(range(27)) and by["B=0 A max"] == []
    assert set(range(13)) <= set(by["A high B low"]) and set(range(14, 27)) <= set(by["A low B high"])
    c = next(c for c in prims if c.cls == "A=0 B max")
    f = c.fes()
    B = sum(V.int_of(f[4 * q + 1]) * V.int_of(f[4 * q + 3]) for q in range(3))
    assert 16.82 * P * P < B < 16.83 * P * P < V.BIAS_KARA


def test_every_primitive_has_its_case_kinds(prims):
    by = {}
    for c in prims:
        by.setdefault(c.op, {}).setdefault(c.cls, []).append(c)
    for op in ("mul", "mul_ra", "mul_rb", "mul_aa", "sqr", "sqr_ra", "mul2", "mul2_rc", "mul4", "mul6", "mul3k"):
        assert len(by[op]["canon"]) == 16 and len(by[op]["lazy"]) == 16 and len(by[op]["top"]) == 1, op
        assert len(by[op]["special"]) >= 6, op
        roles = V.ROLES[V.FUNC_OF[op]]
        assert by[op]["top"][0].fes() == [V.top_pattern(r) for r in roles][:V.IN_FE[op]]
    assert len(by["mul"]["special"]) == 36
    # one-hot: every (i, j) of every pair, each isolating one product term
    assert len(by["mul"]["onehot"]) == 196 and len(by["sqr"]["onehot"]) == len(by["mul_aa"]["onehot"]) == 105
    for op, npair in (("mul2", 2), ("mul4", 4), ("mul6", 6)):
        seen = set()
        for c in by[op]["onehot"]:
            f = c.fes()
            nz = [(k, i) for k, l in enumerate(f) for i, x in enumerate(l) if x]
            assert len(nz) == 2 and nz[0][0] + 1 == nz[1][0] and nz[0][0] % 2 == 0
            roles = V.ROLES[op]
            assert f[nz[0][0]][nz[0][1]] == V.limb_limit(roles[nz[0][0]], nz[0][1])
            assert f[nz[1][0]][nz[1][1]] == V.limb_limit(roles[nz[1][0]], nz[1][1])
            seen.add((nz[0][0] // 2, nz[0][1], nz[1][1]))
        assert len(seen) == npair * 196, op
    seen = set()
    for c in by["mul3k"]["onehot"]:
        nz = [(k, i) for k, l in enumerate(c.fes()) for i, x in enumerate(l) if x]
        assert len(nz) == 2 and nz[1][0] == nz[0][0] + 2
        seen.add((nz[0][0] // 4, nz[0][0] % 4, nz[0][1], nz[1][1]))
    assert len(seen) == 3 * 2 * 196 and {s[1] for s in seen} == {0, 1}
    for cls in ("A=0 B max", "B=0 A max", "A high B low", "A low B high"):
        assert len(by["mul3k"][cls]) == 1
    # lazy operands really are lazy: some limb at or above 2^28, in both constructions
    big = [c for c in by["mul6"]["lazy"] if max(max(l) for l in c.fes()) >= 1 << 28]
    assert len(big) == 16
    assert V.limb_limit(V.L32, 13) == (32 * P - 1) >> 364 and V.limb_limit(V.L32, 3) == (1 << 29) - 1


def test_exact_value_is_what_the_column_loop_returns(prims):
    """The "unique integer" claim, case by case: product-scanning REDC with 28-bit digits m_k
    (the header's mul_n, the generator's signed Karatsuba loop) ends on exactly
    (T + m p) / 2^392, m = -T / p mod 2^392."""
    n = 0
    for c in prims:
        words, _, _ = V.model(c)
        assert V.pack_words(words) == c.exact, (c.op, c.cls, c.id)
        n += 1
    assert n == len(prims)
    # sqr(a) and mul(a, a), and the forms of one operand set, expect the same words
    by = {}
    for c in prims:
        by.setdefault(c.group, []).append(c)
    multi = [g for g in by.values() if len(g) > 1]
    assert len(multi) == 69 + 69 + 105 + 45
    for g in multi:
        assert len({c.exact for c in g}) == 1 and len({tuple(c.words[:14]) for c in g}) == 1
    # the value: the operands' product over 2^392, mod p
    for c in prims[::37]:
        r = struct.unpack("<%dI" % (len(c.exact) // 4), c.exact)
        f = c.fes()
        if c.op == "mul3k":
            x = [(V.int_of(f[4 * q]), V.int_of(f[4 * q + 1])) for q in range(3)]
            u = [(V.int_of(f[4 * q + 2]), V.int_of(f[4 * q + 3])) for q in range(3)]
            s = (0, 0)
            for q in range(3):
                s = O.f2_add(s, O.f2_mul((x[q][0] % P, x[q][1] % P), (u[q][0] % P, u[q][1] % P)))
            assert (V.int_of(r[:14]) % P, V.int_of(r[14:]) % P) == O.f2_muls(s, V.RINV)
            assert max(r) < 1 << 28 and V.int_of(r[:14]) < 103 * P // 100 and V.int_of(r[14:]) < 103 * P // 100
        else:
            T = sum(V.int_of(a) * V.int_of(b) for a, b in V.primitive_pairs(c))
            assert V.int_of(r) % P == T * V.RINV % P and max(r[:13]) < 1 << 28


def _field(x):
    return x * V.RINV % P


def test_composite_expectations_agree_with_the_oracle(cases):
    seen = {}
    for c in cases:
        if c.res is None:
            continue
        seen[c.op] = seen.get(c.op, 0) + 1
        v = [(_field(V.int_of(a)), _field(V.int_of(b))) for a, b in zip(c.fes()[0::2], c.fes()[1::2])]
        want = None
        if c.op in ("fe2_mul", "fe2_mul_ra"):
            want = [O.f2_mul(v[0], v[1])]
        elif c.op == "fe2_sqr":
            want = [O.f2_sqr(v[0])]
        elif c.op == "fe2_mul_fe":
            want = [O.f2_muls(v[0], _field(V.int_of(c.fes()[2])))]
        elif c.op in ("sp_mul_sp_lazy", "sp_mul_sp"):
            want = V.mem_from_w(O.f12_mul(V.sp_w(v[0:3]), V.sp_w(v[3:6])))
        elif c.op in V.FORMS:
            want = V.mem_from_w(O.f12_mul(V.w_from_mem(v[0:6]), V.sp_w(v[6:9])))
        elif c.op == "chain":
            s = [V.sp_w(v[0:3]), V.sp_w(v[3:6]), V.sp_w(v[6:9])]
            acc = O.f12_mul(s[0], s[1])
            want = V.mem_from_w(acc)
            for j in range(V.CHAIN_STEPS):
                acc = O.f12_mul(acc, s[(j + 2) % 3])
                want = want + V.mem_from_w(acc)
        got = [(_field(c.res[2 * i]), _field(c.res[2 * i + 1])) for i in range(len(c.res) // 2)]
        assert got == [tuple(w) for w in want], (c.op, c.cls)
        assert c.bound == V.BOUND[V.FORMS[c.aux] if c.op == "chain" else c.op] * P // 100
    assert set(seen) == set(V.BOUND) | {"chain"} and seen["chain"] == 12 and all(n >= 12 for n in seen.values())
    assert {V.FORMS[c.aux] for c in cases if c.op == "chain"} == set(V.CHAIN_FORMS)
    assert V.sp_w([1, 2, 3]) == [1, V.Z2, 2, 3, V.Z2, V.Z2] and V.w_from_mem(V.mem_from_w(list(range(6)))) == list(range(6))


def test_exact_conversions_agree_with_the_oracle(cases):
    """from_fp / to_fp move between x 2^384 (engine) and x 2^392; sp_from_engine is the product
    times 2^-16 in the radix-2^28 form; fe12_to_engine_scaled reads as the value times 2^8 in the
    engine's form; fp_pow_pm3d4 is a^((p-3)/4) in the engine's Montgomery form, canonical."""
    r384 = pow(V.R384, -1, P)
    n = {}
    for c in cases:
        if c.exact is None or V.FUNC_OF[c.op] in V.PRIMITIVES:
            continue
        n[c.op] = n.get(c.op, 0) + 1
        r = struct.unpack("<%dI" % (len(c.exact) // 4), c.exact)
        if c.op == "from_fp":
            x = V.int12(c.words[:12]) * r384 % P
            assert _field(V.int_of(r)) == x and max(r) < 1 << 28 and V.int_of(r) < 102 * P // 100
        elif c.op == "to_fp":
            assert V.int12(r) < P and V.int12(r) * r384 % P == _field(V.int_of(c.words[:14]))
        elif c.op == "pow_pm3d4":
            a = V.int12(c.words[:12]) * r384 % P
            assert V.int12(r) < P and V.int12(r) * r384 % P == pow(a, (P - 3) // 4, P)
            if a:  # a^((p-3)/4) is 1 / sqrt(a) up to a fourth root of unity: (r^2 a)^2 = 1
                assert pow(V.int12(r) * r384 % P, 4, P) * a * a % P == 1
        elif c.op == "sp_from_engine":
            w = [V.int12(c.words[12 * i:12 * i + 12]) * r384 % P for i in range(9)]
            q = [w[8], w[8], w[6], w[6], w[7], w[7]]
            for k in range(6):
                x = V.int_of(r[14 * k:14 * k + 14])
                assert _field(x) == w[k] * q[k] * pow(2, -16, P) % P and x < 105 * P // 100
        elif c.op == "to_engine_scaled":
            for k, l in enumerate(c.fes()):
                got = V.int12(r[12 * k:12 * k + 12])
                assert got < P and got * r384 % P == _field(V.int_of(l)) * 256 % P
    assert n == {"from_fp": 16, "to_fp": 16, "pow_pm3d4": 24, "sp_from_engine": 16, "to_engine_scaled": 16}


def test_generated_header_is_what_the_generator_writes():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fpmul28.py")], capture_output=True,
                         env={k: v for k, v in os.environ.items() if k != "GEN28_SPLIT"}, check=True).stdout
    committed = open(os.path.join(ROOT, "grandine_amd", "csrc", "bls_fpmul28_gen.h"), "rb").read()
    assert out == committed and out.count(b"v_mad_u64_u32") > 5000


def test_files_layout_and_interleaving(orders, tmp_path):
    inter, srt, ragged = orders
    assert sorted(c.id for c in inter) == sorted(c.id for c in srt) and len({c.id for c in inter}) == len(inter)
    assert 3000 < len(inter) < 6000  # a few thousand lanes
    assert {c.op for c in inter} == set(V.OPS) and set(V.FUNC_OF) == set(V.OPS)
    path = str(tmp_path / "interleaved.bin")
    V.write_cases(path, inter)
    assert os.path.getsize(path) == 4 + 4 * 256 * len(inter)
    raw = open(path, "rb").read()
    for i in (0, 77, len(inter) - 1):
        w = struct.unpack_from("<256I", raw, 4 + 1024 * i)
        c = inter[i]
        assert w[0] == V.OPS[c.op] and w[1] == c.aux and list(w[4:4 + len(c.words)]) == c.words
        assert not any(w[4 + len(c.words):])
    # every 64-lane wave mixes ops and classes
    for w in range(0, len(inter) - 63, 64):
        wave = inter[w:w + 64]
        assert len({c.op for c in wave}) >= 6 and len({c.cls for c in wave}) >= 2, w
    assert sum(1 for w in range(0, len(inter), 64) if len({c.op for c in inter[w:w + 64]}) >= 10) >= 40
    # sorted: uniform waves except where an op ends
    mixed = sum(1 for w in range(0, len(srt), 64) if len({c.op for c in srt[w:w + 64]}) > 1)
    assert mixed <= len(V.OPS)
    assert len(ragged) % 64 == 37 and len(ragged) > 64 and {c.id for c in ragged} <= {c.id for c in inter}
    assert {c.op for c in ragged} == set(V.OPS)
    assert {c.aux for c in ragged if c.op == "chain"} == {V.FORMS.index(f) for f in V.CHAIN_FORMS}
    assert all(c.out_bytes() == 4 * V.OUT_WORDS[c.op] == (len(c.exact) if c.exact else 56 * len(c.res)) for c in inter)


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
    for i, (op, c) in enumerate(sorted(first.items())):  # one bit of one word of one case
        bad = bytearray(model)
        bad[offs[c.id] + 4 * (i % (c.out_bytes() // 4))] ^= 1 << (i % 8)
        rep = V.compare(cases, bytes(bad))
        assert not rep.ok and rep.ops_failed() == [op], (op, rep.text())
        assert [x[0] for x in rep.mismatch[(op, c.cls)]] == [c.id]
        assert V.compare(cases, bytes(bad), ops={o for o in V.OPS if o != op}).ok
    # a composite: right residue but a limb at 2^28, a value above the bound, a late chain step
    c = first["m034_lazy"]
    l = V.limbs_of(c.res[3])
    if l[0] == 0:
        l = V.limbs_of(c.res[3] + P)
    l[0] += 1 << 28
    l[1] -= 1
    if l[1] >= 0:
        bad = bytearray(model)
        bad[offs[c.id] + 56 * 3:offs[c.id] + 56 * 4] = V.pack_words(l)
        assert ">= 2^28" in V.compare(cases, bytes(bad)).text()
    bad = bytearray(model)
    bad[offs[c.id] + 56 * 5:offs[c.id] + 56 * 6] = V.pack_words(V.limbs_of(c.res[5] + P))  # < 2p, > 1.02p
    rep = V.compare(cases, bytes(bad))
    assert rep.ops_failed() == ["m034_lazy"] and "bound 1.02 p" in rep.text()
    c = first["chain"]
    bad = bytearray(model)
    bad[offs[c.id] + 4 * (29 * 168 + 5)] ^= 2
    assert V.compare(cases, bytes(bad)).ops_failed() == ["chain"]
    # aliasing groups: the forms of one operand set
    rep = V.compare(cases, model)
    by, disagree = V.group_disagreements(cases, rep)
    assert not disagree and len(by) > 4000
    c = first["sqr_ra"]
    bad = bytearray(model)
    bad[offs[c.id]] ^= 1
    _, disagree = V.group_disagreements(cases, V.compare(cases, bytes(bad)))
    assert disagree == [(c.group, ["mul_aa", "sqr", "sqr_ra"])]


def test_checker_cross_compiles_and_its_host_mode_passes(orders, tmp_path):
    """The host branch of the header (mul_n) through the same checker and file layout: every word
    of every single-product result, every composite's residue, limbs and bound.  fe2_mul3k's host
    branch is the schoolbook form: equal mod p, another representative."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "ubench"), "-s"])
    exe = os.path.join(ROOT, "tools", "ubench", "_bin", "field28_check")
    assert os.path.exists(exe)
    inter, _, ragged = orders
    for name, cases in (("interleaved", inter), ("ragged", ragged)):
        src, dst = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".out"))
        V.write_cases(src, cases)
        r = subprocess.run([exe, "--host", src, dst], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = open(dst, "rb").read()
        rep = V.compare(cases, out, ops=set(V.OPS) - {"mul3k"})
        assert rep.ok, rep.text()
        assert rep.total() == sum(1 for c in cases if c.op != "mul3k")
        k3 = V.compare(cases, out, ops={"mul3k"})
        n3 = 0
        for c in cases:
            if c.op == "mul3k":
                got = struct.unpack("<28I", k3.words[c.id])
                want = struct.unpack("<28I", c.exact)
                assert got[14:] == want[14:]  # c1: the same T, the same integer
                # c0 rides on neg_lazy(u.c1) on the host: only where 4p - u.c1 has no negative limb
                f = c.fes()
                if all(x <= b for q in range(3) for x, b in zip(f[4 * q + 3], V.BIAS4P)):
                    assert V.int_of(got[:14]) % P == V.int_of(want[:14]) % P
                    n3 += 1
        assert n3 >= (1000 if name == "interleaved" else 1)
