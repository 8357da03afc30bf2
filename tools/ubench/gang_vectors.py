"""Cases, integer reference and comparator for tools/ubench/gang_check (tests/test_gpu_gang.py,
tests/test_gang_vectors.py).

The checker runs grandine_amd/csrc/bls_gang.h function by function, one DPP quad (4 lanes) or one
DPP row (16 lanes) per case, on RAW operand images (12 x 32-bit Montgomery limbs per Fp), and
writes the result words of EVERY lane.  Everything it returns is recomputed here.

Model.  An image W (an integer below p) stands for the field element W 2^-384 mod p.  Every
output of the header is canonical (fp_mul, fp_add, fp_sub reduce to [0, p)) and the formulas are
fixed (dbl-2009-l, add-2007-bl, the Miller steps of bls_pairing.h), so every output word is a
function of the input words: the reference evaluates the formulas with Python integers over Fp
and Fp2 = Fp[u] / (u^2 + 1), multiplies by 2^384 mod p and compares word for word.  Where the
code copies an operand (r = a, r = b) the expectation is that operand's exact image, canonical
or not.  On on-curve operands oracle/bls12_381.py (affine group law) must agree as well
(oracle_check): that pins the formulas to the group, and does not merely restate them.

Layout.  64 threads per work-group: a wave holds 16 quad cases or 4 row cases.  The case list is
written interleaved, every wave holding all four outcomes of the additions' branches (generic,
doubling branch, infinite result, operand copied), and a second time sorted by op and outcome
(uniform waves): both runs must return the same words for every case.
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
R384 = 1 << 384
RINV = pow(R384, -1, P)
ONE_W = R384 % P  # the image of the field element 1
M32 = 0xffffffff
IN_WORDS = 4 + 192
ML_EVENTS = 68
XABS_STEPS = 68  # 63 doublings + 5 additions
HALF = (P + 1) // 2

OPS = {"q_fp2mul": 0, "q_fp2mul_ra": 1, "q_fp2mul_rb": 2, "q_fp2mul_aa": 3, "q_dbl": 4, "q_dbl_rp": 5,
       "q_add": 6, "q_add_ra": 7, "q1_dbl": 8, "q1_dbl_rp": 9, "q1_add": 10, "q1_add_ra": 11,
       "q_line_dbl": 12, "q_line_add": 13, "q_xabs": 14, "q_g1mul": 15, "q_g2mul": 16, "q_lines": 17,
       "r_mul4": 18, "r_mul4_alias": 19, "r_mul4_txxx": 20, "r_dbl": 21, "r_dbl_rp": 22, "r_add": 23,
       "r_add_ra": 24, "r_line_dbl": 25, "r_line_add": 26, "r_xabs": 27, "r_lines": 28}
OP_NAMES = {v: k for k, v in OPS.items()}
OUTCOMES = ("generic", "dbl", "inf", "copy")
# the header's functions ("ops" of the case counts) and the forms they are called in
FUNCS = {"gang_fp2_mul": ("q_fp2mul", "q_fp2mul_ra", "q_fp2mul_rb", "q_fp2mul_aa"),
         "row_mul4": ("r_mul4", "r_mul4_alias", "r_mul4_txxx"),
         "gang_dbl": ("q_dbl", "q_dbl_rp"), "row_dbl": ("r_dbl", "r_dbl_rp"),
         "gang_add": ("q_add", "q_add_ra"), "row_add": ("r_add", "r_add_ra"),
         "gang1_dbl": ("q1_dbl", "q1_dbl_rp"), "gang1_add": ("q1_add", "q1_add_ra"),
         "gang_line_dbl": ("q_line_dbl",), "gang_line_add_aff": ("q_line_add",),
         "row_line_dbl": ("r_line_dbl",), "row_line_add_aff": ("r_line_add",),
         "gang_mul_by_xabs": ("q_xabs",), "row_mul_by_xabs": ("r_xabs",),
         "k_mv_g1mul": ("q_g1mul",), "k_mv_g2mul": ("q_g2mul",), "k_lines": ("q_lines",),
         "k_lines_row": ("r_lines",)}
FUNC_OF = {op: fn for fn, ops in FUNCS.items() for op in ops}
SCALARS = [1, 2, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1]


def is_row(op):
    return OPS[op] >= OPS["r_mul4"]


def lanes(op):
    return 16 if is_row(op) else 4


# ---------------------------------------------------------------- words and images
def words_of_int(x, n=12):
    assert 0 <= x < 1 << (32 * n)
    return [(x >> (32 * i)) & M32 for i in range(n)]


def int_of_words(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def img(v):
    """The image of a field element (an integer mod p)."""
    return v % P * R384 % P


def val(w):
    """The field element of a canonical image."""
    assert 0 <= w < P, "formula operand is not canonical"
    return w * RINV % P


class Fp1:
    """Fp: elements are integers; an element's image is one integer."""
    N = 1
    zero, one, b = 0, 1, 4
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    mul = staticmethod(lambda a, b: a * b % P)
    inv = staticmethod(lambda a: pow(a, -1, P))
    dec = staticmethod(lambda ws: val(ws[0]))
    enc = staticmethod(lambda v: [img(v)])
    oadd, omul = staticmethod(O.g1_add), staticmethod(O.g1_mul)


class Fp2:
    """Fp2 = Fp[u] / (u^2 + 1): elements are pairs; an element's image is two integers."""
    N = 2
    zero, one, b = (0, 0), (1, 0), (4, 4)
    add = staticmethod(lambda a, b: ((a[0] + b[0]) % P, (a[1] + b[1]) % P))
    sub = staticmethod(lambda a, b: ((a[0] - b[0]) % P, (a[1] - b[1]) % P))
    mul = staticmethod(lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P))
    dec = staticmethod(lambda ws: (val(ws[0]), val(ws[1])))
    enc = staticmethod(lambda v: [img(v[0]), img(v[1])])
    oadd, omul = staticmethod(O.g2_add), staticmethod(O.g2_mul)

    @staticmethod
    def inv(a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
        return (a[0] * n % P, -a[1] * n % P)


def f_sqr(F, a):
    return F.mul(a, a)


def f_neg(F, a):
    return F.sub(F.zero, a)


def f_small(F, a, k):
    """k a for a small integer k, by additions."""
    r = F.zero
    for _ in range(k):
        r = F.add(r, a)
    return r


def f2_scale(a, s):
    return (a[0] * s % P, a[1] * s % P)


def dec_n(F, ws, n):
    """n field elements from a list of image integers."""
    return [F.dec(ws[F.N * i:F.N * i + F.N]) for i in range(n)]


def enc_all(F, vals):
    return [w for v in vals for w in F.enc(v)]


# ---------------------------------------------------------------- the formulas (header comments)
def f_dbl_2009_l(F, X, Y, Z):
    """dbl-2009-l, a = 0."""
    A, B = f_sqr(F, X), f_sqr(F, Y)
    C = f_sqr(F, B)
    D = f_small(F, F.sub(F.sub(f_sqr(F, F.add(X, B)), A), C), 2)
    E = f_small(F, A, 3)
    X3 = F.sub(f_sqr(F, E), f_small(F, D, 2))
    Y3 = F.sub(F.mul(E, F.sub(D, X3)), f_small(F, C, 8))
    Z3 = f_small(F, F.mul(Y, Z), 2)
    return X3, Y3, Z3


def dbl_image(F, pw):
    return enc_all(F, f_dbl_2009_l(F, *dec_n(F, pw, 3)))


def inf_image(F):
    return enc_all(F, [F.one, F.one, F.zero])


def add_image(F, aw, bw):
    """add-2007-bl with the header's branches -> (image, outcome).  Infinite operands (Z image all
    zero) are tested first, b before a, and the other operand's image is returned as it is."""
    n = F.N
    if not any(bw[2 * n:3 * n]):
        return list(aw), "copy"
    if not any(aw[2 * n:3 * n]):
        return list(bw), "copy"
    X1, Y1, Z1 = dec_n(F, aw, 3)
    X2, Y2, Z2 = dec_n(F, bw, 3)
    Z1Z1, Z2Z2 = f_sqr(F, Z1), f_sqr(F, Z2)
    U1, U2 = F.mul(X1, Z2Z2), F.mul(X2, Z1Z1)
    S1, S2 = F.mul(F.mul(Y1, Z2), Z2Z2), F.mul(F.mul(Y2, Z1), Z1Z1)
    H = F.sub(U2, U1)
    r = f_small(F, F.sub(S2, S1), 2)
    if H == F.zero:
        if r == F.zero:
            return dbl_image(F, bw), "dbl"
        return inf_image(F), "inf"
    I = f_sqr(F, f_small(F, H, 2))
    J, V = F.mul(H, I), F.mul(U1, I)
    X3 = F.sub(F.sub(f_sqr(F, r), J), f_small(F, V, 2))
    Y3 = F.sub(F.mul(r, F.sub(V, X3)), f_small(F, F.mul(S1, J), 2))
    Z3 = F.mul(F.sub(F.sub(f_sqr(F, F.add(Z1, Z2)), Z1Z1), Z2Z2), H)
    return enc_all(F, [X3, Y3, Z3]), "generic"


B3 = (12, 12)  # 3 b' = 12 (1 + u)


def line_dbl_image(tw):
    """Miller doubling step on a homogeneous T: (T', L0, L2, L3) as one image list.
    A = XY/2, B = Y^2, C = Z^2, E = 3b'C, F = 3E, G = (B+F)/2, H = 2YZ;
    L0 = E - B, L2 = 3X^2, L3 = -H; X3 = A (B - F), Y3 = G^2 - 3E^2, Z3 = B H."""
    F = Fp2
    X, Y, Z = dec_n(F, tw, 3)
    A = f2_scale(F.mul(X, Y), HALF)
    B, C = f_sqr(F, Y), f_sqr(F, Z)
    E = F.mul(B3, C)
    Fv = f_small(F, E, 3)
    G = f2_scale(F.add(B, Fv), HALF)
    H = f_small(F, F.mul(Y, Z), 2)
    L0, L2, L3 = F.sub(E, B), f_small(F, f_sqr(F, X), 3), f_neg(F, H)
    X3 = F.mul(A, F.sub(B, Fv))
    Y3 = F.sub(f_sqr(F, G), f_small(F, f_sqr(F, E), 3))
    Z3 = F.mul(B, H)
    return enc_all(F, [X3, Y3, Z3, L0, L2, L3])


def line_add_image(tw, qw):
    """Miller addition step T + Q, Q = (x2, y2) affine (add-1998-cmo-2 with Z2 = 1):
    theta = Y1 - y2 Z1, lambda = X1 - x2 Z1; L0 = theta x2 - lambda y2, L2 = -theta, L3 = lambda;
    with u = -theta, v = -lambda: A = u^2 Z1 - v^3 - 2 v^2 X1, X3 = v A,
    Y3 = u (v^2 X1 - A) - v^3 Y1, Z3 = v^3 Z1."""
    F = Fp2
    X, Y, Z = dec_n(F, tw, 3)
    x2, y2 = dec_n(F, qw, 2)
    th, la = F.sub(Y, F.mul(y2, Z)), F.sub(X, F.mul(x2, Z))
    L0, L2, L3 = F.sub(F.mul(th, x2), F.mul(la, y2)), f_neg(F, th), la
    u, v = f_neg(F, th), f_neg(F, la)
    vv = f_sqr(F, v)
    vvv = F.mul(vv, v)
    Rr = F.mul(vv, X)
    A = F.sub(F.sub(F.mul(f_sqr(F, u), Z), vvv), f_small(F, Rr, 2))
    X3 = F.mul(v, A)
    Y3 = F.sub(F.mul(u, F.sub(Rr, A)), F.mul(vvv, Y))
    Z3 = F.mul(vvv, Z)
    return enc_all(F, [X3, Y3, Z3, L0, L2, L3])


def xabs_chain(F, pw):
    """[|x|]P as the header writes it: acc = P; for bits 62..0: double, add P on a set bit."""
    acc, steps = list(pw), []
    for i in range(62, -1, -1):
        acc = dbl_image(F, acc)
        steps.append(acc)
        if (O.X_ABS >> i) & 1:
            acc, _ = add_image(F, acc, pw)
            steps.append(acc)
    assert len(steps) == XABS_STEPS
    return steps, acc


def scalar_chain(F, basew, k):
    """The MSB-first double-and-add of k_mv_g1mul / k_mv_g2mul on an affine base image: the
    identity for k = 0 or an all-zero base, else acc = (x, y, 1), then every bit below the top."""
    if k == 0 or not any(basew):
        return [], inf_image(F)
    bj = list(basew) + F.enc(F.one)
    acc, steps = bj, []
    for b in range(k.bit_length() - 2, -1, -1):
        acc = dbl_image(F, acc)
        steps.append(acc)
        if (k >> b) & 1:
            acc, _ = add_image(F, acc, bj)
            steps.append(acc)
    return steps, acc


def g1s_image(accw):
    """g1s_from_jac: (X Z, Y copied, Z^3), all zero for an infinite point."""
    if accw[2] == 0:
        return [0, 0, 0]
    X, _, Z = dec_n(Fp1, accw, 3)
    return [img(X * Z), accw[1], img(Z * Z * Z)]


def ev_is_dbl():
    """The 68 events along |x|: for each bit below the top a doubling, then an addition if set."""
    ev = []
    for i in range(62, -1, -1):
        ev.append(True)
        if (O.X_ABS >> i) & 1:
            ev.append(False)
    assert len(ev) == ML_EVENTS
    return ev


EVENTS = ev_is_dbl()


def lines_chain(qw):
    """k_lines' loop from T = (x, y, 1): every event's (L0, L2, L3), and the final T."""
    T = list(qw) + Fp2.enc(Fp2.one)
    out = []
    for d in EVENTS:
        r = line_dbl_image(T) if d else line_add_image(T, qw)
        T = r[:6]
        out.append(r[6:])
    return out, T


# ---------------------------------------------------------------- cases
class Case:
    """op, the class label (reporting only), the operands as image integers (one per Fp, each
    below 2^384; canonical unless the class says otherwise), the 64-bit scalar and aux word."""
    _next = 0

    def __init__(self, op, cls, ws, k=0, aux=0):
        assert op in OPS and len(ws) <= 16 and all(0 <= w < R384 for w in ws) and 0 <= k < 1 << 64
        self.op, self.cls, self.ws, self.k, self.aux = op, cls, list(ws), k, aux
        self.id = Case._next
        Case._next += 1
        self.pre, self.per, self.outcome = expect(op, aux, k, self.ws)

    def record(self):
        w = [OPS[self.op], self.aux, self.k & M32, self.k >> 32]
        for x in self.ws:
            w += words_of_int(x)
        return w + [0] * (IN_WORDS - len(w))

    def out_bytes(self):
        return len(self.pre) + lanes(self.op) * len(self.per)


def pack(ws):
    return b"".join(w.to_bytes(48, "little") for w in ws)


def expect(op, aux, k, ws):
    """(words written from lane 0 before the lanes' blocks, the block every lane writes, outcome),
    the words as bytes."""
    base = op[2:] if op[1] == "_" else op[3:]
    G = Fp1 if op.startswith("q1_") else Fp2
    n3 = 3 * G.N
    if base.startswith("fp2mul"):
        a, b = dec_n(Fp2, ws, 2)
        return b"", pack(Fp2.enc(Fp2.mul(a, a if base == "fp2mul_aa" else b))), "generic"
    if op in ("r_mul4", "r_mul4_alias"):
        v = dec_n(Fp2, ws, 8)
        return b"", pack(enc_all(Fp2, [Fp2.mul(v[j], v[4 + j]) for j in range(4)])), "generic"
    if op == "r_mul4_txxx":
        e, t = dec_n(Fp2, ws, 2)
        return b"", pack(Fp2.enc(Fp2.mul(e, t)) * 2), "generic"
    if base in ("dbl", "dbl_rp"):
        return b"", pack(dbl_image(G, ws[:n3])), "generic"
    if base in ("add", "add_ra"):
        r, outcome = add_image(G, ws[:n3], ws[n3:2 * n3])
        return b"", pack(r), outcome
    if base == "line_dbl":
        return b"", pack(line_dbl_image(ws[:6])), "generic"
    if base == "line_add":
        return b"", pack(line_add_image(ws[:6], ws[6:10])), "generic"
    if base == "xabs":
        steps, acc = xabs_chain(Fp2, ws[:6])
        return b"".join(pack(s) for s in steps), pack(acc), "generic"
    if op == "q_g1mul":
        steps, acc = scalar_chain(Fp1, ws[:2], k)
        return b"".join(pack(s) for s in steps), pack(acc + g1s_image(acc)), "generic"
    if op == "q_g2mul":
        steps, acc = scalar_chain(Fp2, ws[:4], (k >> 32) if aux else (k & M32))
        return b"".join(pack(s) for s in steps), pack(acc), "generic"
    if base == "lines":
        ls, T = lines_chain(ws[:4])
        return b"", b"".join(pack(l) for l in ls) + pack(T), "generic"
    raise KeyError(op)


# ---------------------------------------------------------------- operand generators
def rnd_fp(rng):
    return rng.randrange(P)


def rnd(rng, n):
    return [rng.randrange(P) for _ in range(n)]


EDGE = [0, ONE_W, P - 1]


def edge_operands(rng, n, j):
    """n Fp images from 0, the Montgomery one and p - 1.  j = 0, 1, 2: all equal (j = 2: every
    Fp2 element has c0 = c1 = p - 1, the lazy Karatsuba sum is 2p - 2); j = 3: every c0 = 0,
    c1 random; j = 4: every c1 = 0; j = 5: c0 = c1 = p - 1 against random; else a random mixture."""
    if j < 3:
        return [EDGE[j]] * n
    if j == 3:
        return [0 if i % 2 == 0 else rnd_fp(rng) for i in range(n)]
    if j == 4:
        return [0 if i % 2 == 1 else rnd_fp(rng) for i in range(n)]
    if j == 5:
        return [P - 1 if (i // 2) % 2 == 0 else rnd_fp(rng) for i in range(n)]
    return [rng.choice(EDGE) if rng.random() < 0.75 else rnd_fp(rng) for _ in range(n)]


class Points:
    """Seeded pools of on-curve affine points (values): G1 multiples of the generator, G2 multiples
    of the generator, and G2 points on the curve outside the subgroup (y solved with f2_sqrt)."""

    def __init__(self, seed, n=24):
        rng = random.Random(seed)
        self.g1, self.g2, self.off = [], [], []
        p1, d1 = O.g1_mul(O.G1_GEN, rng.randrange(1, O.R)), O.g1_mul(O.G1_GEN, rng.randrange(1, O.R))
        p2, d2 = O.g2_mul(O.G2_GEN, rng.randrange(1, O.R)), O.g2_mul(O.G2_GEN, rng.randrange(1, O.R))
        for _ in range(n):
            self.g1.append(p1)
            self.g2.append(p2)
            p1, p2 = O.g1_add(p1, d1), O.g2_add(p2, d2)
        while len(self.off) < n:
            x = (rng.randrange(P), rng.randrange(P))
            y = O.f2_sqrt(O.f2_add(O.f2_mul(O.f2_sqr(x), x), O.B2))
            if y is not None:
                self.off.append((x, y if rng.random() < 0.5 else O.f2_neg(y)))

    def pick(self, F, j):
        """Point j of the field's pool: G1 multiples; G2 alternately in and outside the subgroup."""
        if F is Fp1:
            return self.g1[j % len(self.g1)], "gen"
        pool, cls = ((self.g2, "gen"), (self.off, "offsub"))[j % 2]
        return pool[(j // 2) % len(pool)], cls


def rnd_elem(F, rng, nonzero=True):
    while True:
        v = rng.randrange(P) if F is Fp1 else (rng.randrange(P), rng.randrange(P))
        if not nonzero or v != F.zero:
            return v


def jac_of(F, pt, z):
    """The Jacobian image (X, Y, Z) = (x z^2, y z^3, z) of an affine point."""
    z2 = F.mul(z, z)
    return enc_all(F, [F.mul(pt[0], z2), F.mul(pt[1], F.mul(z2, z)), z])


def hom_of(pt, z):
    return enc_all(Fp2, [Fp2.mul(pt[0], z), Fp2.mul(pt[1], z), z])


def rescale(F, pw, lam, neg=False):
    """The same point (or its negative) in another representation: (l^2 X, +-l^3 Y, l Z)."""
    X, Y, Z = dec_n(F, pw, 3)
    l2 = F.mul(lam, lam)
    Y = F.mul(Y, F.mul(l2, lam))
    return enc_all(F, [F.mul(X, l2), f_neg(F, Y) if neg else Y, F.mul(Z, lam)])


def arbitrary_words(F, rng, j):
    """X and Y images of an infinite point: any words at all (all ones, above p, random)."""
    return [(R384 - 1) if j % 3 == 0 else (P + rng.randrange(R384 - P)) if j % 3 == 1 else rng.randrange(R384)
            for _ in range(2 * F.N)]


DEGENERATE = {"dbl": ("a=b", "a=b scaled", "a=b scaled, off curve"),
              "inf": ("a=-b", "a=-b scaled", "H=0 R!=0, off curve"),
              "copy": ("a inf", "b inf", "both inf")}


def degenerate_add(fam, outcome, j, rng, pts):
    """Case j of an addition that leaves the generic formula: fam 'q' (gang_add), 'q1' (gang1_add)
    or 'r' (row_add); the class cycles through DEGENERATE[outcome], the form through r fresh /
    r aliasing a."""
    F = Fp1 if fam == "q1" else Fp2
    op = {"q": "q_add", "q1": "q1_add", "r": "r_add"}[fam] + ("_ra" if (j // 3) % 2 else "")
    cls = DEGENERATE[outcome][j % 3]
    pt, _ = pts.pick(F, j)
    a = jac_of(F, pt, rnd_elem(F, rng))
    if cls.endswith("off curve"):
        a = rnd(rng, 3 * F.N)
    if cls == "a=b":
        b = list(a)
    elif cls.startswith("a=b scaled"):
        b = rescale(F, a, rnd_elem(F, rng))
    elif cls == "a=-b":
        b = rescale(F, a, F.one, neg=True)
    elif cls == "a=-b scaled":
        b = rescale(F, a, rnd_elem(F, rng), neg=True)
    elif cls.startswith("H=0"):
        X1, _, Z1 = dec_n(F, a, 3)
        z2 = rnd_elem(F, rng)
        zz = F.mul(F.mul(z2, z2), F.inv(F.mul(Z1, Z1)))
        b = enc_all(F, [F.mul(X1, zz), rnd_elem(F, rng), z2])  # U2 = U1, S2 random
    elif cls == "a inf":
        b = jac_of(F, pts.pick(F, j + 1)[0], rnd_elem(F, rng))
        a = arbitrary_words(F, rng, j // 6) + [0] * F.N
    elif cls == "b inf":
        b = arbitrary_words(F, rng, j // 6) + [0] * F.N
    else:
        a = arbitrary_words(F, rng, j // 6) + [0] * F.N
        b = arbitrary_words(F, rng, j // 6 + 1) + [0] * F.N
    c = Case(op, cls, a + b)
    assert c.outcome == outcome, (cls, c.outcome)
    return c


def point_cases(fn, F, pts, seed, two):
    """The cases of a doubling (two = False) or addition over the forms of `fn`: 32 random field
    triples (off the curve), 16 on-curve points with random Z, 12 edge-coordinate operands; a
    doubling also gets Y = 0 (Z3 = 0) and infinite points."""
    rng = random.Random(seed)
    forms = FUNCS[fn]
    out = []
    n = 3 * F.N * (2 if two else 1)
    for j in range(32):
        out.append(Case(forms[j % 2], "random", rnd(rng, n)))
    shift = 2 * (seed % 11)
    for j in range(16):
        # G2: both forms (j % 2) meet points in and outside the subgroup ((j // 2) % 2)
        jj = shift + (j if F is Fp1 else (j // 2) % 2 + 2 * (j // 4))
        pt, cls = pts.pick(F, jj)
        ws = jac_of(F, pt, rnd_elem(F, rng))
        if two:
            ws += jac_of(F, pts.pick(F, jj + 10)[0], rnd_elem(F, rng))  # another point of that pool
        out.append(Case(forms[j % 2], cls, ws))
    for j in range(12):
        ws = edge_operands(rng, n, j // 2)
        out.append(Case(forms[j % 2], "edge", ws))
    if not two:
        for j in range(2):
            ws = rnd(rng, 3 * F.N)
            ws[F.N:2 * F.N] = [0] * F.N
            out.append(Case(forms[j], "Y=0", ws))
            out.append(Case(forms[j], "infinite", rnd(rng, 2 * F.N) + [0] * F.N))
    return out


def build_required(pts):
    """Every case the checks need, op by op (the interleaved order adds further degenerate
    additions as wave fillers)."""
    cs = []
    rng = random.Random(2301)
    # Fp2 products: 16 random + 8 edge per form
    for form in FUNCS["gang_fp2_mul"]:
        for j in range(16):
            cs.append(Case(form, "random", rnd(rng, 4)))
        for j in range(8):
            cs.append(Case(form, "edge", edge_operands(rng, 4, j)))
    for form in FUNCS["row_mul4"]:
        n = 4 if form == "r_mul4_txxx" else 16
        for j in range(16):
            cs.append(Case(form, "random", rnd(rng, n)))
        for j in range(8):
            cs.append(Case(form, "edge", edge_operands(rng, n, j)))
    cs += point_cases("gang_dbl", Fp2, pts, 2302, False)
    cs += point_cases("row_dbl", Fp2, pts, 2303, False)
    cs += point_cases("gang1_dbl", Fp1, pts, 2304, False)
    cs += point_cases("gang_add", Fp2, pts, 2305, True)
    cs += point_cases("row_add", Fp2, pts, 2306, True)
    cs += point_cases("gang1_add", Fp1, pts, 2307, True)
    rng = random.Random(2308)
    for fam in ("q", "r", "q1"):
        for outcome in ("dbl", "inf", "copy"):
            for j in range(6):  # every class in both forms
                cs.append(degenerate_add(fam, outcome, j, rng, pts))
    # line steps
    rng = random.Random(2309)
    for pre in ("q", "r"):
        for j in range(32):
            cs.append(Case(pre + "_line_dbl", "random", rnd(rng, 6)))
            cs.append(Case(pre + "_line_add", "random", rnd(rng, 10)))
        for j in range(16):
            T, cls = pts.pick(Fp2, j)
            Q = pts.pick(Fp2, j + 10)[0]  # another point of the same pool
            z = Fp2.one if j >= 12 else rnd_elem(Fp2, rng)
            cls += ", Z=1" if j >= 12 else ""
            cs.append(Case(pre + "_line_dbl", cls, hom_of(T, z)))
            cs.append(Case(pre + "_line_add", cls, hom_of(T, z) + enc_all(Fp2, Q)))
        for j in range(8):
            cs.append(Case(pre + "_line_dbl", "edge", edge_operands(rng, 6, j)))
            cs.append(Case(pre + "_line_add", "edge", edge_operands(rng, 10, j)))
        for j in range(4):  # T = Q projectively: theta = lambda = 0, every output zero
            Q = (rnd_elem(Fp2, rng), rnd_elem(Fp2, rng)) if j < 2 else pts.pick(Fp2, j)[0]
            cs.append(Case(pre + "_line_add", "theta=lambda=0", hom_of(Q, rnd_elem(Fp2, rng)) + enc_all(Fp2, Q)))
        for j in range(2):  # T = -Q: lambda = 0 alone
            Q = pts.pick(Fp2, j + 3)[0]
            cs.append(Case(pre + "_line_add", "lambda=0", hom_of(O.g2_neg(Q), rnd_elem(Fp2, rng)) + enc_all(Fp2, Q)))
    # [|x|]P and the 68-event loops: 4 points per form
    rng = random.Random(2310)
    for pre in ("q", "r"):
        cs.append(Case(pre + "_xabs", "gen", jac_of(Fp2, pts.g2[3], rnd_elem(Fp2, rng))))
        cs.append(Case(pre + "_xabs", "gen, Z=1", jac_of(Fp2, pts.g2[4], Fp2.one)))
        cs.append(Case(pre + "_xabs", "offsub", jac_of(Fp2, pts.off[3], rnd_elem(Fp2, rng))))
        cs.append(Case(pre + "_xabs", "random", rnd(rng, 6)))
        cs.append(Case(pre + "_lines", "gen", enc_all(Fp2, pts.g2[5])))
        cs.append(Case(pre + "_lines", "gen", enc_all(Fp2, pts.g2[6])))
        cs.append(Case(pre + "_lines", "offsub", enc_all(Fp2, pts.off[5])))
        cs.append(Case(pre + "_lines", "random", rnd(rng, 4)))
    # scalar chains: the fixed scalars and 8 random ones on on-curve bases, again on random pairs
    rng = random.Random(2311)
    ks = SCALARS + [rng.randrange(1, 1 << 64) for _ in range(8)]
    for j, k in enumerate(ks):
        cs.append(Case("q_g1mul", "gen k=%#x" % k, enc_all(Fp1, pts.g1[j]), k=k))
        for half in (0, 1):
            pt, cls = pts.pick(Fp2, j)
            cs.append(Case("q_g2mul", "%s k=%#x half %d" % (cls, k, half), enc_all(Fp2, pt), k=k, aux=half))
    for j, k in enumerate(ks[2:8]):
        cs.append(Case("q_g1mul", "random k=%#x" % k, rnd(rng, 2), k=k))
        cs.append(Case("q_g2mul", "random k=%#x half %d" % (k, j % 2), rnd(rng, 4), k=k, aux=j % 2))
    cs.append(Case("q_g1mul", "k=0", enc_all(Fp1, pts.g1[0]), k=0))
    cs.append(Case("q_g1mul", "infinite base", [0, 0], k=ks[7]))
    cs.append(Case("q_g2mul", "infinite base", [0, 0, 0, 0], k=ks[7]))
    return cs


def interleave(required, pts, seed=2320):
    """File order: waves of 16 quad cases / 4 row cases, each with at least one case of every
    outcome, the ops dealt round-robin; further degenerate additions fill the waves."""
    rng = random.Random(seed)
    waves = {}
    for row in (False, True):
        mine = [c for c in required if is_row(c.op) == row]
        by_op = {}
        for c in mine:
            if c.outcome == "generic":
                by_op.setdefault(c.op, []).append(c)
        generic = []  # dealt round-robin over the ops
        while any(by_op.values()):
            for op in sorted(by_op, key=lambda o: OPS[o]):
                if by_op[op]:
                    generic.append(by_op[op].pop(0))
        deg = {o: [c for c in mine if c.outcome == o] for o in OUTCOMES[1:]}
        size = 4 if row else 16
        nw = max(-(-len(generic) // (size - 3)), max(len(v) for v in deg.values()))
        made = {}
        ws = []
        for w in range(nw):
            wave = generic[w * (size - 3):(w + 1) * (size - 3)]
            if not wave:
                wave = [Case("r_add" if row else "q_add", "random", rnd(rng, 12))]
            for o in OUTCOMES[1:]:
                if deg[o]:
                    wave.append(deg[o].pop(0))
                else:
                    fam = "r" if row else ("q", "q1")[w % 2]
                    j = made.get((fam, o), 6)  # the required cases end at j = 5
                    made[(fam, o)] = j + 1
                    wave.append(degenerate_add(fam, o, j, rng, pts))
            rng.shuffle(wave)
            ws.append(wave)
        waves[row] = ws
    order = []
    q, r = waves[False], waves[True]
    for i in range(max(len(q), len(r))):  # quad and row waves alternate in the file
        order += (q[i] if i < len(q) else []) + (r[i] if i < len(r) else [])
    return order


def build_orders(seed=2300):
    """(interleaved, sorted, ragged): the same cases in file order and sorted by op and outcome
    (uniform waves), and a short list with 21 quad and 5 row cases (both 5 mod 16: the last wave of
    each kernel is partly filled, whole quads / rows return early)."""
    pts = Points(seed)
    inter = interleave(build_required(pts), pts)
    srt = sorted(inter, key=lambda c: (OPS[c.op], OUTCOMES.index(c.outcome), c.cls, c.id))
    ragged = [c for c in inter if not is_row(c.op)][:21] + [c for c in inter if is_row(c.op)][:5]
    return inter, srt, ragged


def write_cases(path, cases):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for c in cases:
            fh.write(struct.pack("<%dI" % IN_WORDS, *c.record()))


def read_cases(path):
    """The records of a case file: (op name, aux, k, operand images as 16 integers)."""
    raw = open(path, "rb").read()
    (n,) = struct.unpack_from("<I", raw)
    assert len(raw) == 4 + 4 * IN_WORDS * n
    out = []
    for i in range(n):
        w = struct.unpack_from("<%dI" % IN_WORDS, raw, 4 + 4 * IN_WORDS * i)
        out.append((OP_NAMES[w[0]], w[1], w[2] | (w[3] << 32), [int_of_words(w[4 + 12 * j:16 + 12 * j]) for j in range(16)]))
    return out


def model_output(cases):
    """The OUT file a correct checker writes."""
    return b"".join(c.pre + c.per * lanes(c.op) for c in cases)


# ---------------------------------------------------------------- comparator
class Report:
    def __init__(self):
        self.compared = {}    # op -> cases compared
        self.mismatch = {}    # (op, class) -> case ids whose words differ from the reference
        self.lanes = {}       # (op, class) -> case ids whose lanes do not hold the same words
        self.words = {}       # case id -> the case's result bytes

    @property
    def ok(self):
        return not self.mismatch and not self.lanes

    def total(self):
        return sum(self.compared.values())

    def ops_failed(self):
        return sorted({op for op, _ in list(self.mismatch) + list(self.lanes)})

    def text(self):
        fmt = lambda d: "none" if not d else "; ".join("%s[%s]: %d (ids %s)" % (op, cls, len(v), v[:4])
                                                     for (op, cls), v in sorted(d.items()))
        return "compared %d cases\nmismatches by op: %s\nlanes of a gang disagree: %s" % (
            self.total(), fmt(self.mismatch), fmt(self.lanes))


def compare(cases, out, ops=None):
    """Every output word of every lane of every case (of `ops`, default all) against the
    reference.  `out` is the checker's whole OUT file; its length must be the cases' exactly."""
    assert len(out) == sum(c.out_bytes() for c in cases), "OUT is %d bytes, the cases need %d" % (
        len(out), sum(c.out_bytes() for c in cases))
    rep, o = Report(), 0
    for c in cases:
        got = out[o:o + c.out_bytes()]
        o += c.out_bytes()
        if ops is not None and c.op not in ops:
            continue
        rep.compared[c.op] = rep.compared.get(c.op, 0) + 1
        rep.words[c.id] = got
        n, m = len(c.pre), len(c.per)
        blocks = [got[n + m * l:n + m * (l + 1)] for l in range(lanes(c.op))]
        if any(b != blocks[0] for b in blocks):
            rep.lanes.setdefault((c.op, c.cls), []).append(c.id)
        if got[:n] != c.pre or any(b != c.per for b in blocks):
            rep.mismatch.setdefault((c.op, c.cls), []).append(c.id)
    return rep


# ---------------------------------------------------------------- the oracle's group law
def _jac_affine(F, ws):
    X, Y, Z = dec_n(F, ws, 3)
    if Z == F.zero:
        return None
    zi = F.inv(Z)
    zi2 = F.mul(zi, zi)
    return (F.mul(X, zi2), F.mul(Y, F.mul(zi2, zi)))


def _hom_affine(ws):
    X, Y, Z = dec_n(Fp2, ws, 3)
    if Z == Fp2.zero:
        return None
    zi = Fp2.inv(Z)
    return (Fp2.mul(X, zi), Fp2.mul(Y, zi))


def _on_curve(F, pt):
    return pt is not None and f_sqr(F, pt[1]) == F.add(F.mul(f_sqr(F, pt[0]), pt[0]), F.b)


def _unpack(b):
    return [int.from_bytes(b[i:i + 48], "little") for i in range(0, len(b), 48)]


def _line_ok(L, T, lam):
    """(L0, L2, L3) is proportional to (lam x_T - y_T, -lam, 1)."""
    L0, L2, L3 = dec_n(Fp2, L, 3)
    if L3 == Fp2.zero:
        return False
    i3 = Fp2.inv(L3)
    return Fp2.mul(L2, i3) == f_neg(Fp2, lam) and Fp2.mul(L0, i3) == Fp2.sub(Fp2.mul(lam, T[0]), T[1])


def _tangent(T):
    return Fp2.mul(f_small(Fp2, f_sqr(Fp2, T[0]), 3), Fp2.inv(f_small(Fp2, T[1], 2)))


def _chord(T, Q):
    return Fp2.mul(Fp2.sub(T[1], Q[1]), Fp2.inv(Fp2.sub(T[0], Q[0])))


def oracle_check(c):
    """None when the case's operands are not curve points; else a list of disagreements between
    the integer reference's expectation and oracle/bls12_381.py (empty: they agree)."""
    op, ws = c.op, c.ws
    F = Fp1 if op.startswith("q1_") or op == "q_g1mul" else Fp2
    base = op[2:] if op[1] == "_" else op[3:]
    n3 = 3 * F.N
    per = _unpack(c.per)
    errs = []
    if base in ("dbl", "dbl_rp", "xabs"):
        p = _jac_affine(F, ws[:n3]) if all(w < P for w in ws[:n3]) else None
        if not _on_curve(F, p):
            return None
        want = F.oadd(p, p) if base != "xabs" else F.omul(p, O.X_ABS)
        if _jac_affine(F, per[:n3]) != want:
            errs.append("result is not the oracle's")
        return errs
    if base in ("add", "add_ra"):
        if not all(w < P for w in ws[:2 * n3]):
            return None
        a, b = _jac_affine(F, ws[:n3]), _jac_affine(F, ws[n3:2 * n3])
        if not (_on_curve(F, a) and _on_curve(F, b)):
            return None
        return [] if _jac_affine(F, per) == F.oadd(a, b) else ["sum is not the oracle's"]
    if base in ("line_dbl", "line_add"):
        T = _hom_affine(ws[:6])
        if not _on_curve(Fp2, T):
            return None
        if base == "line_dbl":
            want, lam = O.g2_add(T, T), _tangent(T)
        else:
            Q = tuple(dec_n(Fp2, ws[6:10], 2))
            if not _on_curve(Fp2, Q) or Q[0] == T[0]:
                return None
            want, lam = O.g2_add(T, Q), _chord(T, Q)
        if _hom_affine(per[:6]) != want:
            errs.append("new T is not the oracle's sum")
        if not _line_ok(per[6:12], T, lam):
            errs.append("line is not proportional to (lam x - y, -lam, 1)")
        return errs
    if op in ("q_g1mul", "q_g2mul"):
        k = c.k if op == "q_g1mul" else ((c.k >> 32) if c.aux else (c.k & M32))
        p = tuple(dec_n(F, ws[:2 * F.N], 2))
        if not any(ws[:2 * F.N]) or not _on_curve(F, p):
            return None
        want = F.omul(p, k) if k else None
        if _jac_affine(F, per[:n3]) != want:
            errs.append("[k]P is not the oracle's")
        if op == "q_g1mul":
            x, y, cc = dec_n(Fp1, per[3:6], 3)
            got = None if cc == 0 else (x * pow(cc, -1, P) % P, y * pow(cc, -1, P) % P)
            if got != want:
                errs.append("g1s_from_jac is not the oracle's point")
        return errs
    if base == "lines":
        Q = tuple(dec_n(Fp2, ws[:4], 2))
        if not _on_curve(Fp2, Q):
            return None
        T = Q
        for e, d in enumerate(EVENTS):
            lam = _tangent(T) if d else _chord(T, Q)
            if not _line_ok(per[6 * e:6 * e + 6], T, lam):
                errs.append("event %d: line is not the oracle's" % e)
            T = O.g2_add(T, T if d else Q)
        if _hom_affine(per[6 * ML_EVENTS:]) != T or T != O.g2_mul(Q, O.X_ABS):
            errs.append("final T is not [|x|]Q")
        return errs
    return None


def main(argv):
    """gang_vectors.py write DIR: the three case files; gang_vectors.py check ORDER OUT: compare."""
    inter, srt, ragged = build_orders()
    orders = {"interleaved": inter, "sorted": srt, "ragged": ragged}
    if len(argv) == 3 and argv[1] == "write":
        for name, cases in orders.items():
            write_cases(os.path.join(argv[2], name + ".bin"), cases)
        return 0
    if len(argv) == 4 and argv[1] == "check" and argv[2] in orders:
        rep = compare(orders[argv[2]], open(argv[3], "rb").read())
        print(rep.text())
        return 0 if rep.ok else 1
    print(main.__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv))
