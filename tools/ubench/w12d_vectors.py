"""Cases and expectations for tools/ubench/w12d_check (tests/test_gpu_w12d.py, tests/test_w12d_vectors.py).

The checker runs grandine_amd/csrc/bls_w12d.h operation by operation on RAW LDS images (12
coefficients x 16 limb words), so every limb of every operand is chosen here, and everything it
returns is recomputed here with Python integers and oracle/bls12_381.py -- never with the
engine's own formulas.

Model.  The value of an image coefficient is V = sum l_j 2^(28 j); the field element it stands
for ("true" value) is V 2^-448 mod p (Montgomery form, R = 2^448).  Every Fp12 operation of the
header is a homomorphism on true values.  store_words writes true 2^384 mod p (canonical engine
form); load_scaled repacks engine-form words W as limbs, so the image's true value is
W 2^-448 = (engine value) 2^-64.  inv_wave maps 12 canonical words x to x^-1 mod p as plain
integers.  Engine coefficient i = 6 h + 2 jj + k is component k of the oracle's Fp2
coefficient of w^(2 jj + h).

Contracts checked on every output coefficient: the residue, every limb < 2^28 + 2^9 with limbs
14 and 15 zero, and the value bound the header states for the operation (BOUNDS).
"""
import os
import random
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import bls12_381 as O  # noqa: E402

P = O.P
M28 = (1 << 28) - 1
LIMB_END = (1 << 28) + (1 << 9)  # every stored limb is below this
R448 = 1 << 448
RINV = pow(R448, -1, P)
R384 = 1 << 384
ONE_M = R448 % P  # the canonical limb value of the field element 1
IMG = 192
CHAIN_STEPS = 200

OPS = {"mul": 0, "mul_ca": 1, "mul_cb": 2, "mul_aa": 3, "sqr": 4, "sqr_ca": 5, "cyc_sqr": 6, "conj": 7,
       "frob": 8, "frob2": 9, "exp_x_cyc": 10, "easy_part": 11, "inv_wave": 12, "load_scaled": 13,
       "one_flags": 14, "zero_flags": 15, "chain": 16, "chain_cyc": 17}

# exclusive value bounds from the header comments of bls_w12d.h / bls_dfp.h
B_COEF = 128 * P            # R2 outputs of mul / sqr
B_CONJ = 128 * P + 1        # conj: the 128 p bias minus the coefficient (128 p for a zero image)
B_CYC = 40 * P              # cyc_sqr
B_PROD = P + (1 << 336)     # dfp::mul (frob2)
B_PROD2 = P + (1 << 337)    # dfp::mul2 (frob)
BOUNDS = {"mul": B_COEF, "mul_ca": B_COEF, "mul_cb": B_COEF, "mul_aa": B_COEF, "sqr": B_COEF, "sqr_ca": B_COEF,
          "cyc_sqr": B_CYC, "conj": B_CONJ, "frob": B_PROD2, "frob2": B_PROD, "exp_x_cyc": B_CONJ}

# the fixed number of cases per op (tests assert them)
COUNTS = {"mul": 80, "mul_ca": 80, "mul_cb": 80, "mul_aa": 80, "sqr": 80, "sqr_ca": 80, "cyc_sqr": 49, "conj": 80,
          "frob": 80, "frob2": 80, "exp_x_cyc": 49, "easy_part": 28, "inv_wave": 237, "load_scaled": 60,
          "one_flags": 54, "zero_flags": 40, "chain": 2, "chain_cyc": 2}


# ---------------------------------------------------------------- limbs and images
def limbs_of(v):
    assert 0 <= v < R448
    return [(v >> (28 * j)) & M28 for j in range(16)]


def value_of(limbs):
    return sum(l << (28 * j) for j, l in enumerate(limbs))


def borrow(limbs, rng):
    """The same value with redundant limbs: wherever limb j is below 2^9 and limb j + 1 is not
    zero, limb j may take 2^28 from the limb above (with probability 1/2)."""
    l = list(limbs)
    for j in range(13):
        if l[j] < (1 << 9) and l[j + 1] >= 1 and rng.random() < 0.5:
            l[j] += 1 << 28
            l[j + 1] -= 1
    assert value_of(l) == value_of(limbs) and all(0 <= x < LIMB_END for x in l)
    return l


def image_of_values(vals):
    assert len(vals) == 12
    return [limbs_of(v) for v in vals]


def image_words(img):
    assert len(img) == 12 and all(len(c) == 16 for c in img)
    return [l for c in img for l in c]


def image_from_words(words):
    assert len(words) == IMG
    return [list(words[16 * c:16 * c + 16]) for c in range(12)]


def eng_to_f12(c):
    """12 engine-ordered Fp values -> the oracle's 6 Fp2 coefficients."""
    out = [None] * 6
    for h in range(2):
        for jj in range(3):
            out[2 * jj + h] = (c[6 * h + 2 * jj] % P, c[6 * h + 2 * jj + 1] % P)
    return out


def f12_to_eng(a):
    c = [0] * 12
    for h in range(2):
        for jj in range(3):
            c[6 * h + 2 * jj], c[6 * h + 2 * jj + 1] = a[2 * jj + h]
    return c


def image_true(img):
    """The Fp12 element (oracle form) an image stands for."""
    return eng_to_f12([value_of(c) * RINV % P for c in img])


def image_of_f12(a, add=0):
    """The canonical image of an oracle element, `add` (a multiple of p) on every coefficient."""
    return image_of_values([x * R448 % P + add for x in f12_to_eng(a)])


def engine_bytes(a):
    """The 576 bytes of the engine's fp12 (12 x 48 bytes, value 2^384 mod p) of an oracle element."""
    return b"".join((x * R384 % P).to_bytes(48, "little") for x in f12_to_eng(a))


def f12_from_engine_bytes(b):
    assert len(b) == 576
    ri = pow(R384, -1, P)
    return eng_to_f12([int.from_bytes(b[48 * i:48 * i + 48], "little") * ri % P for i in range(12)])


def words_of_int(x, n=12):
    return [(x >> (32 * i)) & 0xffffffff for i in range(n)]


def int_of_words(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


# ---------------------------------------------------------------- operand generators
def top_coeff(rng, dense=False):
    """Limbs of a value in [127 p, 128 p) with redundant limbs: limbs 0..11 at 2^28 + 2^9 - 1
    (all of them if dense, else each with probability 1/2; the excess over 2^28 is what a
    canonical form would carry into the limb above), the top two limbs from a random value of
    that range.  The value is x + 127 p for the canonical x = value - 127 p."""
    low = [(LIMB_END - 1) if (dense or rng.random() < 0.5) else rng.randrange(1 << 28) for _ in range(12)]
    if not any(l >= 1 << 28 for l in low):
        low[rng.randrange(12)] = LIMB_END - 1
    t = rng.randrange(127 * P + (1 << 342), 128 * P - (1 << 342))
    hi = t >> 336
    l = low + [hi & M28, hi >> 28, 0, 0]
    check_top(l)
    return l


def check_top(l):
    v = value_of(l)
    assert 127 * P <= v < 128 * P, "not in [127 p, 128 p)"
    assert any(x >= 1 << 28 for x in l), "no redundant limb"
    assert all(0 <= x < LIMB_END for x in l) and l[14] == 0 and l[15] == 0


def random_f12(rng):
    return [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]


def cyclotomic(f):
    """f^((p^6 - 1)(p^2 + 1)) with the oracle's inversion, conjugation and Frobenius."""
    g = O.f12_mul(O.f12_conj(f), O.f12_inv(f))
    return O.f12_mul(O.f12_frob(O.f12_frob(g)), g)


def element_pool(seed):
    """80 (kind, image) operands: 48 random canonical, 12 edge patterns of 0 / 1 / p - 1, the
    elements 0, 1, an Fp scalar and an Fp6 element, and 16 top-of-contract images (the first
    with all twelve coefficients dense at the top, so that presums of 8 sit just under 1024 p;
    the others with a random subset at the top and the rest canonical or zero)."""
    rng = random.Random(seed)
    pool = []
    for _ in range(48):
        pool.append(("random", image_of_values([rng.randrange(P) for _ in range(12)])))
    edge = [0, 1, P - 1]
    for e in edge:
        pool.append(("edge", image_of_values([e] * 12)))
    for _ in range(9):
        pool.append(("edge", image_of_values([rng.choice(edge) for _ in range(12)])))
    pool.append(("elem", image_of_values([0] * 12)))
    pool.append(("elem", image_of_values([ONE_M] + [0] * 11)))
    pool.append(("elem", image_of_values([rng.randrange(P)] + [0] * 11)))
    pool.append(("elem", image_of_values([rng.randrange(P) for _ in range(6)] + [0] * 6)))
    pool.append(("top", [top_coeff(rng, dense=True) for _ in range(12)]))
    pool.append(("top", [top_coeff(rng) for _ in range(12)]))
    for t in range(14):
        img = []
        for c in range(12):
            r = rng.random()
            if r < 0.5:
                img.append(top_coeff(rng, dense=(t % 2 == 0)))
            elif r < 0.75:
                img.append(limbs_of(0))
            else:
                img.append(limbs_of(rng.randrange(P)))
        if not any(value_of(c) >= 127 * P for c in img):
            img[rng.randrange(12)] = top_coeff(rng)
        pool.append(("top", img))
    assert len(pool) == 80
    return pool


def cyclotomic_pool(seed):
    """49 (kind, image): the element 1, 24 cyclotomic elements (canonical), and the same 24 with
    127 p added to every coefficient (limbs borrowed where a limb allows it)."""
    rng = random.Random(seed)
    els = [cyclotomic(random_f12(rng)) for _ in range(24)]
    pool = [("one", image_of_f12(O.f12_one()))]
    pool += [("cyc", image_of_f12(a)) for a in els]
    for a in els:
        pool.append(("cyc+127p", [borrow(c, rng) for c in image_of_f12(a, add=127 * P)]))
    assert len(pool) == 49
    return pool


class Case:
    def __init__(self, op, kind, a=None, b=None, words=None):
        self.op, self.kind, self.a, self.b, self.words = op, kind, a, b, words

    def record(self):
        w = [OPS[self.op], 0, 0, 0]
        if self.words is not None:
            w += list(self.words) + [0] * (2 * IMG - len(self.words))
        else:
            w += image_words(self.a) + (image_words(self.b) if self.b is not None else [0] * IMG)
        assert len(w) == 4 + 2 * IMG
        return w

    def out_words(self):
        if self.op == "easy_part":
            return IMG + 24 + IMG + 144
        if self.op == "inv_wave":
            return 13
        if self.op in ("one_flags", "zero_flags"):
            return 12
        if self.op in ("chain", "chain_cyc"):
            return CHAIN_STEPS * IMG + 144
        return IMG + 144


ZERO_REPS = [0, P, 2 * P, 127 * P, 128 * P]
NONZERO_REPS = [1, P + 1, P - 1, 2 * P - 1, 127 * P + 1, 1 << 336, (1 << 336) + 1, P + (1 << 336) - 1,
                P + (1 << 336), 127 * P + (1 << 336) + 1, 128 * P - 1]
ONE_REPS = [ONE_M, ONE_M + P, ONE_M + 2 * P, ONE_M + 127 * P]
NOT_ONE_REPS = [ONE_M + 1, ONE_M - 1, ONE_M + P + 1, ONE_M + 127 * P - 1]


def inv_inputs(seed):
    rng = random.Random(seed)
    xs = [1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2]
    xs += [(1 << k) % P for k in range(0, 381, 29)]
    # g = 0 mod 2^30 with g != 0 after one or two batches: the rare exit-test path
    xs += [(rng.randrange(1 << 300) | 1) << 60 for _ in range(8)]
    xs += [(rng.randrange(1 << 280) | 1) << 90 for _ in range(8)]
    xs += [rng.randrange(1, P) for _ in range(200)]
    xs += [0]
    assert all(0 <= x < P for x in xs) and len(xs) == 237
    return xs


def build_cases():
    """Every case of every op, in a fixed order (seeded)."""
    cases = []
    pa, pb = element_pool(1201), element_pool(1202)
    rng = random.Random(1203)
    perm = list(range(80))
    rng.shuffle(perm)
    for op in ("mul", "mul_ca", "mul_cb"):
        for i in range(80):
            # top-of-contract operands meet each other (i and perm[i] both in the last 16) in some
            # cases and canonical ones in others
            j = i if op == "mul" and i >= 64 else perm[i]
            cases.append(Case(op, pa[i][0] + "*" + pb[j][0], pa[i][1], pb[j][1]))
    for op in ("mul_aa", "sqr", "sqr_ca", "conj", "frob", "frob2"):
        for kind, img in pa:
            cases.append(Case(op, kind, img))
    cyc = cyclotomic_pool(1204)
    for op in ("cyc_sqr", "exp_x_cyc"):
        for kind, img in cyc:
            cases.append(Case(op, kind, img))
    # easy_part: 12 random, 4 Fp6, 2 with F1 = 0 (Fp scalars), 2 with F0 = 0 (s (1 + u): the
    # norm is -8 s^6 u), 8 top-of-contract
    rng = random.Random(1205)
    for _ in range(12):
        cases.append(Case("easy_part", "random", image_of_values([rng.randrange(1, P) for _ in range(12)])))
    for _ in range(4):
        cases.append(Case("easy_part", "fp6", image_of_values([rng.randrange(1, P) for _ in range(6)] + [0] * 6)))
    for _ in range(2):
        cases.append(Case("easy_part", "F1=0", image_of_values([rng.randrange(1, P)] + [0] * 11)))
    for _ in range(2):
        s = rng.randrange(1, P)
        cases.append(Case("easy_part", "F0=0", image_of_values([s, s] + [0] * 10)))
    cases.append(Case("easy_part", "top", [top_coeff(rng, dense=True) for _ in range(12)]))
    for _ in range(7):
        cases.append(Case("easy_part", "top", [top_coeff(rng) if rng.random() < 0.7 else limbs_of(rng.randrange(P))
                                               for _ in range(12)]))
    for x in inv_inputs(1206):
        cases.append(Case("inv_wave", "x", words=words_of_int(x)))
    # load_scaled + store_words: canonical engine-form words
    rng = random.Random(1207)
    edge = [0, 1, P - 1]
    loads = [[rng.randrange(P) for _ in range(12)] for _ in range(48)]
    loads += [[e] * 12 for e in edge] + [[rng.choice(edge) for _ in range(12)] for _ in range(9)]
    for vals in loads:
        cases.append(Case("load_scaled", "words", words=[w for v in vals for w in words_of_int(v)]))
    # flags: every representative in every coefficient, then mixtures
    rng = random.Random(1208)
    reps = ZERO_REPS + NONZERO_REPS
    for v in reps:
        cases.append(Case("zero_flags", "all-equal", [borrow(limbs_of(v), rng) for _ in range(12)]))
    for _ in range(24):
        cases.append(Case("zero_flags", "mixed", [borrow(limbs_of(rng.choice(ZERO_REPS if rng.random() < 0.5 else reps)), rng)
                                                  for _ in range(12)]))
    oreps = reps + ONE_REPS + NOT_ONE_REPS
    for v in ONE_REPS + NOT_ONE_REPS + [0, P, 1, P + 1, 128 * P - 1, P + (1 << 336)]:
        cases.append(Case("one_flags", "all-equal", [borrow(limbs_of(v), rng) for _ in range(12)]))
    for _ in range(16):  # the element 1 in non-canonical forms: every flag set
        cases.append(Case("one_flags", "is-one", [borrow(limbs_of(rng.choice(ONE_REPS)), rng)] +
                          [borrow(limbs_of(rng.choice(ZERO_REPS)), rng) for _ in range(11)]))
    for _ in range(24):
        cases.append(Case("one_flags", "mixed", [borrow(limbs_of(rng.choice(oreps)), rng) for _ in range(12)]))
    # chains: a canonical seed and a top-of-contract seed; cyclotomic seeds canonical and + 127 p
    rng = random.Random(1209)
    cases.append(Case("chain", "random", image_of_values([rng.randrange(P) for _ in range(12)])))
    cases.append(Case("chain", "top", [top_coeff(rng, dense=True) for _ in range(12)]))
    cases.append(Case("chain_cyc", "cyc", cyc[1][1]))
    cases.append(Case("chain_cyc", "cyc+127p", cyc[26][1]))
    counts = {}
    for c in cases:
        counts[c.op] = counts.get(c.op, 0) + 1
    assert counts == COUNTS, counts
    return cases


def write_cases(path, cases):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for c in cases:
            fh.write(struct.pack("<%dI" % (4 + 2 * IMG), *c.record()))


def read_results(path, cases):
    raw = open(path, "rb").read()
    total = sum(c.out_words() for c in cases)
    assert len(raw) == 4 * total, (len(raw), 4 * total)
    words = struct.unpack("<%dI" % total, raw)
    out, o = [], 0
    for c in cases:
        out.append(words[o:o + c.out_words()])
        o += c.out_words()
    return out


# ---------------------------------------------------------------- expectations
def exact_batches(x):
    """The number of 30-divstep batches of the safegcd iteration (f = p, g = x, eta = -1 at the
    start; a step: if g is odd, swap (f, g) -> (g, -f) when eta < 0, and add f to g; then halve
    g and decrement eta) until g = 0 at a batch boundary, on exact integers: what inv_wave runs
    when its exit test sees g = 0 as soon as it holds."""
    f, g, eta, n = P, x, -1, 0
    while g != 0 and n < 40:
        for _ in range(30):
            if g & 1:
                if eta < 0:
                    eta, f, g = -eta, g, -f
                g += f
            g >>= 1
            eta -= 1
        n += 1
    return n


def expected_f12(case):
    """The oracle's value of the op's result on the case's operands."""
    a = image_true(case.a)
    op = case.op
    if op in ("mul", "mul_ca", "mul_cb"):
        return O.f12_mul(a, image_true(case.b))
    if op in ("mul_aa", "sqr", "sqr_ca", "cyc_sqr"):
        return O.f12_sqr(a) if op != "mul_aa" else O.f12_mul(a, a)
    if op == "conj":
        return O.f12_conj(a)
    if op == "frob":
        return O.f12_frob(a)
    if op == "frob2":
        return O.f12_frob(O.f12_frob(a))
    if op == "exp_x_cyc":
        return O.f12_conj(O.f12_pow(a, O.X_ABS))
    raise KeyError(op)


def check_image(words, want, bound, what):
    """Residue, limb contract and value bound of one output image; returns error strings."""
    errs = []
    img = image_from_words(words)
    for c, l in enumerate(img):
        if not all(x < LIMB_END for x in l) or l[14] or l[15]:
            errs.append("%s: coefficient %d breaks the limb contract: %s" % (what, c, [hex(x) for x in l]))
        if value_of(l) >= bound:
            errs.append("%s: coefficient %d = %.3f p, bound %.3f p" % (what, c, value_of(l) / P, bound / P))
    if image_true(img) != [tuple(x) for x in want]:
        errs.append("%s: wrong residue" % what)
    return errs


def check_words(words, want, what):
    """store_words: canonical engine form (true 2^384 mod p) of the expected element."""
    got = [int_of_words(words[12 * i:12 * i + 12]) for i in range(12)]
    exp = [x * R384 % P for x in f12_to_eng(want)]
    return [] if got == exp else ["%s: store_words differ in coefficients %s" %
                                  (what, [i for i in range(12) if got[i] != exp[i]])]


def f6_norm(n0, n1, n2):
    """The Fp6 -> Fp2 norm of n0 + n1 v + n2 v^2 (v^3 = xi)."""
    A = O.f2_sub(O.f2_sqr(n0), O.f2_mul(O.XI, O.f2_mul(n1, n2)))
    B = O.f2_sub(O.f2_mul(O.XI, O.f2_sqr(n2)), O.f2_mul(n0, n1))
    C = O.f2_sub(O.f2_sqr(n1), O.f2_mul(n0, n2))
    return O.f2_add(O.f2_mul(n0, A), O.f2_mul(O.XI, O.f2_add(O.f2_mul(n2, B), O.f2_mul(n1, C))))


def chain_expectations(case):
    a = image_true(case.a)
    x, out = a, []
    for i in range(CHAIN_STEPS):
        if case.op == "chain":
            k = i % 5
            if k == 0:
                x, b = O.f12_sqr(x), B_COEF
            elif k == 1:
                x, b = O.f12_mul(x, a), B_COEF
            elif k == 2:
                x, b = O.f12_frob(x), B_PROD2
            elif k == 3:
                x, b = O.f12_conj(x), B_CONJ
            else:
                x, b = O.f12_frob(O.f12_frob(x)), B_PROD
        elif i % 2 == 0:
            x, b = O.f12_sqr(x), B_CYC
        else:
            x, b = O.f12_mul(x, a), B_COEF
        out.append((x, b))
    return out


def check_case(idx, case, res):
    """Error strings of one case (empty: the case passes)."""
    op = case.op
    what = "case %d %s[%s]" % (idx, op, case.kind)
    if op in BOUNDS:
        want = expected_f12(case)
        return check_image(res[:IMG], want, BOUNDS[op], what) + check_words(res[IMG:], want, what)
    if op == "load_scaled":
        vals = [int_of_words(case.words[12 * i:12 * i + 12]) for i in range(12)]
        img = image_from_words(res[:IMG])
        errs = []
        if [value_of(c) for c in img] != vals or any(x > M28 for c in img for x in c):
            errs.append("%s: the image is not the repacked words" % what)
        # true value of the image: W 2^-448 = (W 2^-384) 2^-64
        want = eng_to_f12([v * RINV % P for v in vals])
        scale = pow(1 << 64, -1, P)
        assert want == eng_to_f12([v * pow(R384, -1, P) * scale % P for v in vals])
        return errs + check_words(res[IMG:], want, what)
    if op in ("one_flags", "zero_flags"):
        exp = []
        for r in range(12):
            t = value_of(case.a[r]) * RINV % P
            exp.append(1 if t == (1 if (op == "one_flags" and r == 0) else 0) else 0)
        return [] if list(res) == exp else ["%s: flags %s, expected %s" % (what, list(res), exp)]
    if op == "inv_wave":
        x = int_of_words(case.words[:12])
        if x == 0:
            return []  # garbage, never a hang: the run ended
        y, nb = int_of_words(res[:12]), res[12]
        errs = []
        if not (y < P and y * x % P == 1):
            errs.append("%s: x = %#x: out is not x^-1 mod p (out < p: %s)" % (what, x, y < P))
        # the exit test must see g = 0 at once, also when its limbs are a redundant zero
        if nb != exact_batches(x):
            errs.append("%s: x = %#x: %d batches, the exact iteration ends after %d" % (what, x, nb, exact_batches(x)))
        return errs
    if op == "easy_part":
        f = image_true(case.a)
        N = O.f12_mul(f, O.f12_conj(f))
        F = f6_norm(N[0], N[2], N[4])
        D = (F[0] * F[0] + F[1] * F[1]) % P
        c0 = O.f12_mul(O.f12_conj(f), O.f12_inv(f))  # f^(p^6 - 1)
        t = O.f12_frob(O.f12_frob(c0))
        c = O.f12_mul(t, c0)
        assert c == cyclotomic(f)
        errs = check_image(res[:IMG], c, B_COEF, what + " c")
        dw, iw = int_of_words(res[IMG:IMG + 12]), int_of_words(res[IMG + 12:IMG + 24])
        if dw != D * R384 % P:
            errs.append("%s: words[0..12) is not D = F0^2 + F1^2 in engine form" % what)
        if not (iw < P and iw * dw % P == 1):
            errs.append("%s: words[12..24) is not the inverse of words[0..12)" % what)
        # easy_part leaves frob2(f^(p^6 - 1)) in t (it overwrites N^-1 with its last operand)
        errs += check_image(res[IMG + 24:2 * IMG + 24], t, B_PROD, what + " t")
        return errs + check_words(res[2 * IMG + 24:], c, what)
    if op in ("chain", "chain_cyc"):
        errs = []
        steps = chain_expectations(case)
        for i, (want, bound) in enumerate(steps):
            errs += check_image(res[i * IMG:(i + 1) * IMG], want, bound, "%s step %d" % (what, i))
            if len(errs) > 8:
                break
        return errs + check_words(res[CHAIN_STEPS * IMG:], steps[-1][0], what)
    raise KeyError(op)


def check_all(cases, results, ops=None):
    """(count of cases checked per op, error strings) over the given ops (default: all)."""
    counts, errs = {}, []
    for i, (c, r) in enumerate(zip(cases, results)):
        if ops is not None and c.op not in ops:
            continue
        counts[c.op] = counts.get(c.op, 0) + 1
        errs += check_case(i, c, r)
    return counts, errs
