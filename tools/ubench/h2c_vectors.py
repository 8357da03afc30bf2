"""Cases, integer reference and comparator for tools/ubench/h2c_check
(tests/test_gpu_h2c_map.py, tests/test_h2c_vectors.py).

The checker runs fp2_sqrt_pow (bls_curve.h: the square root of point decoding), fp2_sqrt_norm_inv
and map_to_g2 (bls_hash.h: the SSWU map and the 3-isogeny) on RAW engine-form field elements (12
words per Fp element, x 2^384 mod p), every case once per lane with the lane exponentiation and once
per 16-lane row with the row exponentiation (RowPow, bls_dfp.h).  Everything it returns is
recomputed here with Python integers: the two square roots by restating their formulas (the flag
and the exact root the formula selects, every word), the map through oracle/bls12_381.py, compared
as the affine point because the Jacobian representative is the implementation's choice.  Nothing
is imported from the engine.

OUT is the lane policy's n x 72 words followed by the row policy's."""
import os
import random
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import bls12_381 as O  # noqa: E402

P = O.P
R384 = 1 << 384
RINV = pow(R384, -1, P)
INV2 = (P + 1) // 2
PM3D4 = (P - 3) // 4
FP = 12
IN_WORDS = 4 + 4 * FP
OUT_WORDS = 72
FILL = 0xEEEEEEEE
OPS = ("sqrt_pow", "sqrt_norm_inv", "map_to_g2")
POLICIES = ("lane", "row")


def words(x):
    """The engine's image of x in Fp: x 2^384 mod p, 12 little-endian words."""
    v = x * R384 % P
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(FP)]


def of_words(w):
    """(x, canonical): the element of a 12-word image, and whether the image is < p."""
    v = sum(int(x) << (32 * i) for i, x in enumerate(w))
    return v * RINV % P, v < P


# ---------------------------------------------------------------- the formulas restated
def sqrt_pow(a):
    """fp2_sqrt_pow: (flag, the root the formula selects).  gamma = n^((p+1)/4) for the norm n;
    delta = (a0 + gamma) / 2, or (a0 - gamma) / 2 when that is 0 (a1 == 0 and a0 a non-residue);
    t = delta^((p-3)/4), x0 = delta t: (x0, a1 t / 2) if x0^2 == delta, else (-a1 t / 2, x0)."""
    a0, a1 = a
    if a0 == 0 and a1 == 0:
        return True, (0, 0)
    n = (a0 * a0 + a1 * a1) % P
    gamma = pow(n, PM3D4, P) * n % P
    if gamma * gamma % P != n:
        return False, None
    r = _root(a, gamma, 1)[0]
    return O.f2_sqr(r) == (a0, a1), r


def _root(a, gamma, nd):
    a0, a1 = a
    delta = (a0 + gamma) * INV2 % P
    if delta == 0:
        delta = (a0 - gamma) * INV2 % P
    nd2 = nd * nd % P
    tp = pow(delta * nd2 * nd2 % P, PM3D4, P)
    t = tp * nd2 % P
    x0 = delta * t % P
    half = a1 * t * INV2 % P
    sq = x0 * x0 % P == delta
    r = (x0, half) if sq else (-half % P, x0)
    if delta == 0:
        return r, O.fp_inv(nd)
    u = nd * tp * x0 % P
    return r, (u if sq else -u % P)


def sqrt_norm_inv(a, gamma, nd):
    """fp2_sqrt_norm_inv: (root, 1 / nd) for a square a, gamma either root of its norm, nd != 0."""
    return _root(a, gamma % P, nd)


def gx1_is_square(u):
    """Whether the SSWU map of u takes x1 (else x2 = Z u^2 x1)."""
    A, B, Z = O.SSWU_A, O.SSWU_B, O.SSWU_Z
    zu2 = O.f2_mul(Z, O.f2_sqr(u))
    tv1 = O.f2_add(O.f2_sqr(zu2), zu2)
    if O.f2_is_zero(tv1):
        x1 = O.f2_mul(B, O.f2_inv(O.f2_mul(Z, A)))
    else:
        x1 = O.f2_mul(O.f2_mul(O.f2_neg(B), O.f2_inv(A)), O.f2_add(O.F2_ONE, O.f2_inv(tv1)))
    return O.f2_is_square(O.f2_add(O.f2_add(O.f2_mul(O.f2_sqr(x1), x1), O.f2_mul(A, x1)), B))


# ---------------------------------------------------------------- cases
class Case:
    def __init__(self, op, cls, a, gamma=0, nd=0):
        self.op, self.cls, self.a, self.gamma, self.nd = op, cls, a, gamma % P, nd % P
        self.id = None

    def record(self):
        w = [OPS.index(self.op), 0, 0, 0] + words(self.a[0]) + words(self.a[1]) + words(self.gamma) + words(self.nd)
        assert len(w) == IN_WORDS
        return struct.pack("<%dI" % IN_WORDS, *w)


def _residue(rng, want):
    while True:
        x = rng.randrange(2, P)
        if O.fp_is_square(x) == want:
            return x


def sqrt_inputs(rng):
    """[(class, a)]: the input classes of the two square roots."""
    out = [("zero", (0, 0)), ("one", (1, 0)), ("minus one", (P - 1, 0))]
    out += [("a1=0 residue", (_residue(rng, True), 0)) for _ in range(3)]
    out += [("a1=0 non-residue", (_residue(rng, False), 0)) for _ in range(3)]  # the delta == 0 fallback
    out += [("a0=0", (0, rng.randrange(1, P))) for _ in range(3)]
    out += [("a0=0", (0, 1)), ("a0=0", (0, P - 1))]
    for _ in range(16):
        b = (rng.randrange(P), rng.randrange(P))
        out.append(("random square", O.f2_sqr(b)))
    while sum(1 for c, _ in out if c == "non-square") < 6:
        a = (rng.randrange(P), rng.randrange(P))
        if not O.f2_is_square(a):
            out.append(("non-square", a))
    return out


def build_cases(seed=9380):
    rng = random.Random(seed)
    cases = []
    ins = sqrt_inputs(rng)
    for cls, a in ins:
        cases.append(Case("sqrt_pow", cls, a))
    nds = [1, 2, P - 1, rng.randrange(2, P), rng.randrange(2, P), 3]
    k = 0
    for cls, a in ins:
        if cls == "non-square":
            continue  # the caller has decided that a is a square
        n = (a[0] * a[0] + a[1] * a[1]) % P
        g = O.fp_sqrt(n)
        assert g is not None
        for sign in (1, -1):
            cases.append(Case("sqrt_norm_inv", cls + (" gamma" if sign == 1 else " -gamma"), a, sign * g, nds[k % len(nds)]))
            k += 1
    us = [("u=0", (0, 0)), ("u=1", (1, 0)), ("u=(0,1)", (0, 1)), ("u=(p-1,0)", (P - 1, 0)), ("u=(0,p-1)", (0, P - 1))]
    for _ in range(2):
        c1 = rng.randrange(1, P)
        us.append(("c0=0 odd c1", (0, c1 | 1)))
        us.append(("c0=0 even c1", (0, c1 & ~1 or 2)))
    us += [("c1=0", (rng.randrange(1, P), 0))]
    us += [("random", (rng.randrange(P), rng.randrange(P))) for _ in range(32)]
    for cls, u in us:
        cases.append(Case("map_to_g2", cls, u))
    for i, c in enumerate(cases):
        c.id = i
    return cases


def build_orders(seed=9380):
    """(interleaved, sorted, ragged): the cases with the ops mixed in every wave, the same cases
    op by op, and a short list whose last wave holds 37 lanes (its last row block 37 rows)."""
    cases = build_cases(seed)
    by_op = {op: [c for c in cases if c.op == op] for op in OPS}
    inter, k = [], 0
    while any(by_op.values()):
        op = OPS[k % len(OPS)]
        k += 1
        if by_op[op]:
            inter.append(by_op[op].pop(0))
    sorted_ = sorted(inter, key=lambda c: (OPS.index(c.op), c.id))
    ragged = inter[:101]
    assert len(ragged) % 64 == 37 and {c.op for c in ragged} == set(OPS)
    return inter, sorted_, ragged


def write_cases(path, cases):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for c in cases:
            fh.write(c.record())


# ---------------------------------------------------------------- comparison
def _fp(w, errs, what):
    x, canon = of_words(w)
    if not canon:
        errs.append(what + ": words not below p")
    return x


def _f2(w, errs, what):
    return (_fp(w[:FP], errs, what + ".c0"), _fp(w[FP:2 * FP], errs, what + ".c1"))


def check_case(c, w):
    """The errors of one case's 72 result words (none: the case passed)."""
    errs = []
    if c.op == "sqrt_pow":
        flag, r = sqrt_pow(c.a)
        if w[0] != int(flag):
            errs.append("flag %d, want %d" % (w[0], int(flag)))
        elif flag:
            got = _f2(w[1:1 + 2 * FP], errs, "r")
            if got != r:
                errs.append("root differs from the formula's (r^2 == a: %s)" % (O.f2_sqr(got) == c.a))
            if list(w[1:1 + 2 * FP]) != words(r[0]) + words(r[1]):
                errs.append("root words")
        used = 1 + 2 * FP
    elif c.op == "sqrt_norm_inv":
        r, ndinv = sqrt_norm_inv(c.a, c.gamma, c.nd)
        assert O.f2_sqr(r) == c.a and ndinv * c.nd % P == 1
        got = _f2(w[:2 * FP], errs, "r")
        gi = _fp(w[2 * FP:3 * FP], errs, "ndinv")
        if O.f2_sqr(got) != c.a:
            errs.append("r^2 != a")
        if gi * c.nd % P != 1:
            errs.append("ndinv nd != 1")
        if list(w[:3 * FP]) != words(r[0]) + words(r[1]) + words(ndinv):
            errs.append("words differ from the formula's")
        used = 3 * FP
    else:
        want = O.iso_map_g2(O.map_to_curve_sswu(c.a))
        x, y, z = (_f2(w[2 * FP * k:2 * FP * (k + 1)], errs, "XYZ"[k]) for k in range(3))
        if O.f2_is_zero(z):
            got = None
        else:
            zi = O.f2_inv(z)
            zi2 = O.f2_sqr(zi)
            got = (O.f2_mul(x, zi2), O.f2_mul(y, O.f2_mul(zi2, zi)))
        if got != want:
            errs.append("affine point differs from the oracle's")
        used = OUT_WORDS
    if any(x != FILL for x in w[used:]):
        errs.append("words written past the result")
    return errs


class Report:
    def __init__(self):
        self.compared = {}   # (policy, op) -> cases compared
        self.failed = []     # (policy, case id, op, class, errors)
        self.words = {}      # (policy, case id) -> the result words

    @property
    def ok(self):
        return not self.failed

    def total(self):
        return sum(self.compared.values())

    def text(self):
        return "%d of %d failed: %s" % (len(self.failed), self.total(), self.failed[:6])


def compare(cases, out, policies=POLICIES):
    n = len(cases)
    assert len(out) == 2 * n * OUT_WORDS * 4, "OUT holds %d bytes, %d cases" % (len(out), n)
    w = struct.unpack("<%dI" % (2 * n * OUT_WORDS), out)
    rep = Report()
    for p in policies:
        base = POLICIES.index(p) * n * OUT_WORDS
        for i, c in enumerate(cases):
            got = w[base + i * OUT_WORDS:base + (i + 1) * OUT_WORDS]
            rep.words[(p, c.id)] = got
            rep.compared[(p, c.op)] = rep.compared.get((p, c.op), 0) + 1
            errs = check_case(c, got)
            if errs:
                rep.failed.append((p, c.id, c.op, c.cls, errs))
    return rep


def model_output(cases):
    """The OUT bytes a correct lane-policy run returns for the two square roots (map cases and
    the row half at the fill): the comparator's own self-test."""
    half = []
    for c in cases:
        w = [FILL] * OUT_WORDS
        if c.op == "sqrt_pow":
            flag, r = sqrt_pow(c.a)
            w[0] = int(flag)
            w[1:1 + 2 * FP] = (words(r[0]) + words(r[1])) if flag else [0] * (2 * FP)
        elif c.op == "sqrt_norm_inv":
            r, ndinv = sqrt_norm_inv(c.a, c.gamma, c.nd)
            w[:3 * FP] = words(r[0]) + words(r[1]) + words(ndinv)
        else:
            pt = O.iso_map_g2(O.map_to_curve_sswu(c.a))
            w[:] = words(pt[0][0]) + words(pt[0][1]) + words(pt[1][0]) + words(pt[1][1]) + words(1) + words(0)
        half += w
    return struct.pack("<%dI" % (2 * len(half)), *(half + [FILL] * len(half)))
