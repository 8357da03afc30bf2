"""Cases, integer reference and comparator for tools/ubench/curve28_check
(tests/test_gpu_curve28.py, tests/test_curve28_vectors.py).

The checker runs the radix-2^28 curve layer (grandine_amd/csrc/bls_curve28.h) on the GPU, one
case per lane, on RAW limb images (14 words per fe, 12 per engine-form fp; nothing converted).
Everything it returns is recomputed here with Python integers.  The header's formulas are restated
on plain field values -- dbl-2009-l, add-2007-bl, madd-2007-bl with their degenerate branches, the
homogeneous line steps, the complete addition of Renes-Costello-Batina (algorithm 7), psi and the
Budroni-Pintore sequences -- and nothing is imported from the engine; the limb and bound models are
field28_vectors.py's, the curve points come from oracle/bls12_381.py and tests/golden.

An fe with integer X stands for X 2^-392 mod p; an engine-form word W for W 2^-384 mod p.  A
result coordinate is checked in one of two ways:
  exact   every word: canonical outputs (to_fp / g2j_out, g1s_from_jac28, g1h28_store), single
          products (from_fp / g2j_in), the repacked words (store12 / load12), half, booleans, and
          every coordinate the header COPIES (r = a, the constants of jac_set_inf and f_one);
  residue mod p against the restated formula, coordinate by coordinate, with every limb < 2^28
          and the value below the bound the header states for that output.
Bounds, in hundredths of p: 103 for every product, sub_r, lin_r / sub2_r / subk_r, mulk_r and
add + wred result ("every f_ operation returns a normalized, weakly reduced value (< 1.03 p)");
203 for the Z of jac_dbl28 ("Z3 normalized and < 2.03 p"); 102 for fe2_mul_fe and from_fp
(field28_vectors.BOUND).  A chain's bound is that of its last step.

UNDEFINED lists the outputs the header leaves open; the comparator skips them."""
import json
import os
import random
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import field28_vectors as F28  # noqa: E402
from oracle import bls12_381 as O  # noqa: E402

P = F28.P
N = 14
M28 = F28.M28
R, RINV, R384 = F28.R, F28.RINV, F28.R384
R384INV = pow(R384, -1, P)
limbs_of, int_of, words12, int12, pack_words = F28.limbs_of, F28.int_of, F28.words12, F28.int12, F28.pack_words
X_ABS = 0xD201000000010000
EVENTS = 68
ZERO_L = [0] * N
ONE_L = limbs_of(R % P)  # K28_ONE
# every output of every op is defined by the header (an infinite g1h28 sum returns the formula's
# x and y with c = 0; the chain on a (0, 0) base ends in jac_set_inf)
UNDEFINED = ()

B_F, B_Z2, B_FE = 103, 203, 102   # hundredths of p (module docstring)
IN_POINT = 21 * P // 10           # "input coordinates normalized and < 2.1 p"
IN_LINE_T = 103 * P // 100        # T of the line steps, g1h28 coordinates, half
IN_3B = 4 * P                     # fe2_mul_3b


# ---------------------------------------------------------------- the two coordinate fields
class K1:
    n, zero, one = 1, 0, 1
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    mul = staticmethod(lambda a, b: a * b % P)
    neg = staticmethod(lambda a: -a % P)
    muls = staticmethod(lambda a, k: a * k % P)
    inv = staticmethod(lambda a: pow(a, -1, P) if a % P else 0)
    comps = staticmethod(lambda a: [a])
    make = staticmethod(lambda c: c[0] % P)
    is_zero = staticmethod(lambda a: a % P == 0)


class K2:
    n, zero, one = 2, (0, 0), (1, 0)
    add = staticmethod(lambda a, b: ((a[0] + b[0]) % P, (a[1] + b[1]) % P))
    sub = staticmethod(lambda a, b: ((a[0] - b[0]) % P, (a[1] - b[1]) % P))
    mul = staticmethod(lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P))
    neg = staticmethod(lambda a: (-a[0] % P, -a[1] % P))
    muls = staticmethod(lambda a, k: (a[0] * k % P, a[1] * k % P))
    comps = staticmethod(lambda a: [a[0], a[1]])
    make = staticmethod(lambda c: (c[0] % P, c[1] % P))
    is_zero = staticmethod(lambda a: a[0] % P == 0 and a[1] % P == 0)

    @staticmethod
    def inv(a):  # conj(a) / N(a), 0 -> 0
        n = K1.inv((a[0] * a[0] + a[1] * a[1]) % P)
        return (a[0] * n % P, -a[1] * n % P)


def k2_pow(a, e):
    r = K2.one
    while e:
        if e & 1:
            r = K2.mul(r, a)
        a = K2.mul(a, a)
        e >>= 1
    return r


conj = lambda a: (a[0], -a[1] % P)
XI = (1, 1)
PSI_CX = K2.inv(k2_pow(XI, (P - 1) // 3))   # psi(x, y) = (conj(x) PSI_CX, conj(y) PSI_CY)
PSI_CY = K2.inv(k2_pow(XI, (P - 1) // 2))
PSI2_CX = K2.mul(PSI_CX, conj(PSI_CX))[0]   # psi^2(x, y) = (x N(PSI_CX), y N(PSI_CY)), both in Fp
PSI2_CY = K2.mul(PSI_CY, conj(PSI_CY))[0]
INV2 = pow(2, -1, P)


# ---------------------------------------------------------------- coordinates of the model
class Co:
    """A coordinate: its field value, the header's bound on the raw value (hundredths of p) and,
    for each Fp component the header copies from an input or a constant, the raw limbs."""
    __slots__ = ("v", "b", "raw")

    def __init__(self, v, b, raw=None):
        self.v, self.b, self.raw = v, b, raw


def co_in(K, raws):
    return Co(K.make([int_of(l) * RINV % P for l in raws]), None, [list(l) for l in raws])


def co_one(K):
    return Co(K.one, 100, [ONE_L] + [ZERO_L] * (K.n - 1))


def co_zero(K):
    return Co(K.zero, 100, [ZERO_L] * K.n)


def p_inf(K):  # jac_set_inf
    return (co_one(K), co_one(K), co_zero(K))


def f(v):
    return Co(v, B_F)


# ---------------------------------------------------------------- the restated point formulas
def m_dbl(K, p):
    """dbl-2009-l (a = 0)."""
    X, Y, Z = p[0].v, p[1].v, p[2].v
    A, B = K.mul(X, X), K.mul(Y, Y)
    C = K.mul(B, B)
    t = K.add(X, B)
    D = K.muls(K.sub(K.sub(K.mul(t, t), A), C), 2)
    E = K.muls(A, 3)
    X3 = K.sub(K.mul(E, E), K.muls(D, 2))
    Y3 = K.sub(K.mul(E, K.sub(D, X3)), K.muls(C, 8))
    return (f(X3), f(Y3), Co(K.muls(K.mul(Y, Z), 2), B_Z2))


def m_add(K, a, b):
    """add-2007-bl with the header's branches: b infinite -> a, a infinite -> b (copies),
    H = 0 -> the doubling of b or jac_set_inf."""
    if K.is_zero(b[2].v):
        return a
    if K.is_zero(a[2].v):
        return b
    X1, Y1, Z1, X2, Y2, Z2 = a[0].v, a[1].v, a[2].v, b[0].v, b[1].v, b[2].v
    Z1Z1, Z2Z2 = K.mul(Z1, Z1), K.mul(Z2, Z2)
    U1, U2 = K.mul(X1, Z2Z2), K.mul(X2, Z1Z1)
    S1, S2 = K.mul(K.mul(Y1, Z2), Z2Z2), K.mul(K.mul(Y2, Z1), Z1Z1)
    H = K.sub(U2, U1)
    r = K.muls(K.sub(S2, S1), 2)
    if K.is_zero(H):
        return m_dbl(K, b) if K.is_zero(r) else p_inf(K)
    t = K.add(Z1, Z2)
    ZZ = K.sub(K.sub(K.mul(t, t), Z1Z1), Z2Z2)
    t = K.muls(H, 2)
    I = K.mul(t, t)
    J, V = K.mul(H, I), K.mul(U1, I)
    X3 = K.sub(K.sub(K.mul(r, r), J), K.muls(V, 2))
    Y3 = K.sub(K.mul(r, K.sub(V, X3)), K.muls(K.mul(S1, J), 2))
    return (f(X3), f(Y3), f(K.mul(ZZ, H)))


def aff_is_inf(K, b):
    return K.is_zero(b[0].v) and K.is_zero(b[1].v)


def m_madd(K, a, b, check_b):
    """madd-2007-bl; check_b: the affine (0, 0) is infinity (jac_add_aff28<true>)."""
    if check_b and aff_is_inf(K, b):
        return a
    if K.is_zero(a[2].v):
        return (b[0], b[1], co_one(K))
    X1, Y1, Z1, X2, Y2 = a[0].v, a[1].v, a[2].v, b[0].v, b[1].v
    Z1Z1 = K.mul(Z1, Z1)
    H = K.sub(K.mul(X2, Z1Z1), X1)
    r = K.muls(K.sub(K.mul(K.mul(Y2, Z1), Z1Z1), Y1), 2)
    if K.is_zero(H):
        return m_dbl(K, (b[0], b[1], co_one(K))) if K.is_zero(r) else p_inf(K)
    HH = K.mul(H, H)
    I = K.muls(HH, 4)
    J, V = K.mul(H, I), K.mul(X1, I)
    t = K.add(Z1, H)
    Z3 = K.sub(K.sub(K.mul(t, t), Z1Z1), HH)
    X3 = K.sub(K.sub(K.mul(r, r), J), K.muls(V, 2))
    Y3 = K.sub(K.mul(r, K.sub(V, X3)), K.muls(K.mul(Y1, J), 2))
    return (f(X3), f(Y3), f(Z3))


def m_neg(K, p):
    return (p[0], f(K.neg(p[1].v)), p[2])


def m_eq(K, p, q):
    pi, qi = K.is_zero(p[2].v), K.is_zero(q[2].v)
    if pi or qi:
        return pi and qi
    z1, z2 = K.mul(p[2].v, p[2].v), K.mul(q[2].v, q[2].v)
    if K.mul(p[0].v, z2) != K.mul(q[0].v, z1):
        return False
    return K.mul(K.mul(p[1].v, q[2].v), z2) == K.mul(K.mul(q[1].v, p[2].v), z1)


def m_psi(p):
    z = p[2]
    return (f(K2.mul(conj(p[0].v), PSI_CX)), f(K2.mul(conj(p[1].v), PSI_CY)),
            Co(conj(z.v), max(B_F, z.b or B_F), [z.raw[0] if z.raw else None, None]))  # z.c0 is copied


def m_psi2(p):
    return (Co(K2.muls(p[0].v, PSI2_CX), B_FE), Co(K2.muls(p[1].v, PSI2_CY), B_FE), p[2])


def m_of_aff(a):
    return p_inf(K2) if aff_is_inf(K2, a) else (a[0], a[1], co_one(K2))


def m_to_aff(p):
    zi = K2.inv(p[2].v)
    zi2 = K2.mul(zi, zi)
    return (f(K2.mul(p[0].v, zi2)), f(K2.mul(p[1].v, K2.mul(zi2, zi))))


def m_xabs(b):
    """[|x|] b on an affine base: 63 doublings, a mixed addition (b known finite) where the bit
    of |x| is set; the (0, 0) base ends in jac_set_inf."""
    if aff_is_inf(K2, b):
        return p_inf(K2)
    acc = (b[0], b[1], co_one(K2))
    for i in range(62, -1, -1):
        acc = m_dbl(K2, acc)
        if (X_ABS >> i) & 1:
            acc = m_madd(K2, acc, b, False)
    return acc


def m_xabs_jac(p):  # mul_by_xabs: Jacobian base, full additions
    acc = p
    for i in range(62, -1, -1):
        acc = m_dbl(K2, acc)
        if (X_ABS >> i) & 1:
            acc = m_add(K2, acc, p)
    return acc


def m_in_group(b):  # psi(P) == [x]P, x < 0
    return m_eq(K2, m_psi(m_of_aff(b)), m_neg(K2, m_xabs(b)))


def m_clear_mid(pa, x1):
    p = m_of_aff(pa)
    t2 = m_add(K2, m_psi(p), m_neg(K2, x1))
    T = m_add(K2, x1, m_neg(K2, p))
    T = m_add(K2, T, m_psi2(m_dbl(K2, p)))
    T = m_add(K2, T, m_neg(K2, m_psi(p)))
    return m_to_aff(t2), T


def m_clear_post(x2, T):
    return m_add(K2, m_neg(K2, x2), T)


def m_clear_staged(p):
    pa = m_to_aff(p)
    t2a, T = m_clear_mid(pa, m_xabs(pa))
    return m_clear_post(m_xabs(t2a), T)


def m_clear_full(p):
    """Budroni-Pintore: [x^2 - x - 1]P + [x - 1]psi(P) + psi^2(2P), in clear_cofactor28's order."""
    t1 = m_neg(K2, m_xabs_jac(p))
    t2 = m_add(K2, m_psi(p), t1)
    t3 = m_neg(K2, m_xabs_jac(t2))
    t3 = m_add(K2, t3, m_neg(K2, t1))
    t3 = m_add(K2, t3, m_psi2(m_dbl(K2, p)))
    t3 = m_add(K2, t3, m_neg(K2, m_psi(p)))
    return m_add(K2, t3, m_neg(K2, p))


def signed_digits(k):
    """k = sum d_i 8^i, d_i in [-3, 4] for i < 21, d_21 in [0, 2]."""
    d, carry = [], 0
    for i in range(21):
        v = ((k >> (3 * i)) & 7) + carry
        carry = 1 if v > 4 else 0
        d.append(v - 8 * carry)
    return d + [(k >> 63) + carry]


def m_g1mul(base, k):
    """g1_mul_u64_w3_28: the table {P, 2P, 3P, 4P}, the top digit selected, then three
    doublings and one addition per window (a zero digit keeps the accumulator)."""
    t0 = (base[0], base[1], co_zero(K1) if aff_is_inf(K1, base) else co_one(K1))
    t1 = m_dbl(K1, t0)
    tab = [None, t0, t1, m_add(K1, t1, t0), m_dbl(K1, t1)]
    d = signed_digits(k)
    acc = p_inf(K1) if d[21] == 0 else tab[d[21]]
    for i in range(20, -1, -1):
        for _ in range(3):
            acc = m_dbl(K1, acc)
        if d[i]:
            q = tab[abs(d[i])]
            acc = m_add(K1, acc, m_neg(K1, q) if d[i] < 0 else q)
    return acc


def m_g1h_add(a, b):
    """Renes-Costello-Batina algorithm 7 (a = 0, b3 = 12) on (x : y : c); c = 0 is infinity."""
    K = K1
    ai, bi = K.is_zero(a[2].v), K.is_zero(b[2].v)
    if ai:
        return b
    if bi:
        return a
    X1, Y1, Z1, X2, Y2, Z2 = a[0].v, a[1].v, a[2].v, b[0].v, b[1].v, b[2].v
    t0, t1, t2 = K.mul(X1, X2), K.mul(Y1, Y2), K.mul(Z1, Z2)
    t3 = K.add(K.mul(X1, Y2), K.mul(X2, Y1))
    t4 = K.add(K.mul(Y1, Z2), K.mul(Y2, Z1))
    y3 = K.muls(K.add(K.mul(X1, Z2), K.mul(X2, Z1)), 12)
    t0, t2 = K.muls(t0, 3), K.muls(t2, 12)
    z3, t1 = K.add(t1, t2), K.sub(t1, t2)
    return (f(K.sub(K.mul(t3, t1), K.mul(t4, y3))), f(K.add(K.mul(y3, t0), K.mul(t1, z3))),
            f(K.add(K.mul(z3, t4), K.mul(t0, t3))))


def m_mul_3b(a):  # 3 b' a, b' = 4 (1 + u)
    return K2.muls(K2.mul(a, XI), 12)


def m_line_dbl(T):
    """The doubling step on a homogeneous T = (X : Y : Z) of the twist y^2 = x^3 + 4 (1 + u)
    -> (L0, L2, L3), T'."""
    K = K2
    X, Y, Z = T
    B, C = K.mul(Y, Y), K.mul(Z, Z)
    E = m_mul_3b(C)
    H = K.muls(K.mul(Y, Z), 2)
    A = K.muls(K.mul(X, Y), INV2)
    L3, L0, L2 = K.neg(H), K.sub(E, B), K.muls(K.mul(X, X), 3)
    Fv = K.muls(E, 3)
    G = K.muls(K.add(B, Fv), INV2)
    T2 = (K.mul(A, K.sub(B, Fv)), K.sub(K.mul(G, G), K.muls(K.mul(E, E), 3)), K.mul(B, H))
    return (L0, L2, L3), T2


def m_line_add(T, q):
    """The mixed addition step: theta = Y1 - y2 Z1, lambda = X1 - x2 Z1."""
    K = K2
    X, Y, Z = T
    x2, y2 = q
    th, la = K.sub(Y, K.mul(y2, Z)), K.sub(X, K.mul(x2, Z))
    L = (K.sub(K.mul(th, x2), K.mul(la, y2)), K.neg(th), la)
    uu, vv = K.mul(th, th), K.mul(la, la)
    vvv = K.neg(K.mul(vv, la))
    Rr = K.mul(vv, X)
    A = K.sub(K.sub(K.sub(K.mul(uu, Z), vvv), Rr), Rr)
    T2 = (K.neg(K.mul(la, A)), K.sub(K.neg(K.mul(th, K.sub(Rr, A))), K.mul(vvv, Y)), K.mul(vvv, Z))
    return L, T2


def ev_is_dbl():
    """The 68 events: a doubling per bit of |x| below the top, an addition where it is set."""
    ev = []
    for i in range(62, -1, -1):
        ev.append(True)
        if (X_ABS >> i) & 1:
            ev.append(False)
    assert len(ev) == EVENTS
    return ev


EV_DBL = ev_is_dbl()


def m_line_chain(q):
    T = (q[0], q[1], K2.one)
    out = []
    for dbl in EV_DBL:
        L, T = m_line_dbl(T) if dbl else m_line_add(T, q)
        out.append(L)
    return out, T


# ---------------------------------------------------------------- ops
OP_LIST = ["g2_dbl", "g2_dbl_rp", "g2_add", "g2_add_ra", "g2_madd_t", "g2_madd_t_ra", "g2_madd_f", "g2_madd_f_ra",
           "g2_neg", "g2_eq", "g1_dbl", "g1_dbl_rp", "g1_add", "g1_add_ra", "g1_neg", "g1_eq", "psi", "psi2",
           "of_aff", "to_aff", "fe2_inv", "inv", "half", "fe2_half", "mul_3b", "store12", "load12", "g2j_rt",
           "g2a_rt", "g2j_in", "g2j_out", "line_dbl", "line_add", "g1h_load", "g1h_add", "g1h_add_ra",
           "g1h_add_rb", "g1h_store", "line_chain", "xabs", "in_group", "clear_mid", "clear_post", "clear_staged",
           "clear_full", "g1mul"]
OPS = {n: i for i, n in enumerate(OP_LIST)}
IN_WORDS = 4 + 168
# the header's functions and the forms they are called in
FUNCS = {"jac_dbl28": ("g2_dbl", "g2_dbl_rp", "g1_dbl", "g1_dbl_rp"),
         "jac_add28": ("g2_add", "g2_add_ra", "g1_add", "g1_add_ra"),
         "jac_add_aff28": ("g2_madd_t", "g2_madd_t_ra", "g2_madd_f", "g2_madd_f_ra"),
         "jac_neg": ("g2_neg", "g1_neg"), "jac_eq": ("g2_eq", "g1_eq"),
         "g2_psi28": ("psi",), "g2_psi2_28": ("psi2",), "g2j_of_aff28": ("of_aff",), "jac_to_aff28": ("to_aff",),
         "fe2_inv": ("fe2_inv",), "inv": ("inv",), "half": ("half", "fe2_half"), "fe2_mul_3b": ("mul_3b",),
         "store12": ("store12", "load12", "g2j_rt", "g2a_rt"), "g2j_in": ("g2j_in",), "g2j_out": ("g2j_out",),
         "line_dbl28": ("line_dbl",), "line_add28": ("line_add",), "line_chain": ("line_chain",),
         "g2_xabs_aff28": ("xabs",), "g2_in_group28": ("in_group",),
         "clear_mid28": ("clear_mid",), "clear_post28": ("clear_post",),
         "clear_cofactor28_staged": ("clear_staged",), "clear_cofactor28": ("clear_full",),
         "g1_mul_u64_w3_28": ("g1mul",), "g1h28_load": ("g1h_load",),
         "g1h28_add": ("g1h_add", "g1h_add_ra", "g1h_add_rb"), "g1h28_store": ("g1h_store",)}
FUNC_OF = {op: fn for fn, ops in FUNCS.items() for op in ops}
# the test groups of tests/test_gpu_curve28.py
GROUPS = {"point formulas": ("jac_dbl28", "jac_add28", "jac_add_aff28", "jac_neg", "jac_eq"),
          "maps and conversions": ("g2_psi28", "g2_psi2_28", "g2j_of_aff28", "jac_to_aff28", "fe2_inv", "inv", "half",
                                   "fe2_mul_3b", "store12", "g2j_in", "g2j_out"),
          "lines": ("line_dbl28", "line_add28", "line_chain"),
          "xabs": ("g2_xabs_aff28", "g2_in_group28"),
          "clearing": ("clear_mid28", "clear_post28", "clear_cofactor28_staged", "clear_cofactor28"),
          "g1mul": ("g1_mul_u64_w3_28",),
          "g1h28": ("g1h28_load", "g1h28_add", "g1h28_store")}
DEGENERATE = ("dbl branch", "neg branch", "a inf Z=0", "a inf Z=p", "a inf Z=2p", "b inf Z=0", "b inf Z=p",
              "b inf Z=2p", "both inf", "b aff00", "b aff00 p", "a inf b aff00")


def items_of(K, co):
    out = []
    for i, c in enumerate(K.comps(co.v)):
        if co.raw is not None and co.raw[i] is not None:
            out.append(("exact", list(co.raw[i])))
        else:
            out.append(("res", c * R % P, co.b * P // 100))
    return out


def items_pt(K, pt):
    return [it for co in pt for it in items_of(K, co)]


def items_vals(K, vals, b=B_F):
    return [it for v in vals for it in items_of(K, Co(v, b))]


class Case:
    """op, class label, operand words (raw), the scalar; items: the expected result in order,
    ("exact", words) or ("res", residue, exclusive value bound) per 14-word coefficient.
    oracle: for on-curve cases, what the result is as a point ((kind, operands...), K, model
    point), for tests/test_curve28_vectors.py."""
    _next = 0

    def __init__(self, op, cls, words, items, scalar=0, group=None, oracle=None):
        assert op in OPS and len(words) <= IN_WORDS - 4 and all(0 <= w <= F28.M32 for w in words), (op, cls)
        self.op, self.cls, self.words, self.scalar, self.group = op, cls, list(words), scalar, group
        self.items, self.oracle = items, oracle
        self.id = Case._next
        Case._next += 1

    def record(self):
        w = [OPS[self.op], 0, self.scalar & F28.M32, self.scalar >> 32] + self.words
        return w + [0] * (IN_WORDS - len(w))

    def out_words(self):
        return sum(len(it[1]) if it[0] == "exact" else N for it in self.items)

    def out_bytes(self):
        return 4 * self.out_words()


# ---------------------------------------------------------------- operands
def raw_of(v, k=0):
    """The raw limbs of an Fp value: its canonical image plus k p."""
    return limbs_of(v * R % P + k * P)


def top_k(v, bound):
    """The largest k with v R mod p + k p below the bound."""
    return (bound - 1 - v * R % P) // P


def raws(K, v, mode, rng, bound=IN_POINT):
    """Raw limbs per component: 'canon', 'top' (each component at its largest representative
    below the bound with probability 1/2) or 'topall'."""
    out = []
    for c in K.comps(v):
        k = top_k(c, bound) if mode == "topall" or (mode == "top" and rng.random() < 0.5) else 0
        out.append(raw_of(c, k))
    return out


def full_pattern(bound):
    """Every limb below the top full, the top limb the largest the bound allows."""
    return F28.top_pattern((M28, bound))


def flat(ls):
    return [w for l in ls for w in l]


def jac_of(K, aff, lam):
    """The Jacobian representative (x l^2, y l^3, l) of an affine point (None: (1, 1, 0) l-scaled)."""
    if aff is None:
        return (K.mul(lam, lam), K.mul(K.mul(lam, lam), lam), K.zero)
    l2 = K.mul(lam, lam)
    return (K.mul(aff[0], l2), K.mul(aff[1], K.mul(l2, lam)), lam)


def rnd_k(K, rng):
    while True:
        v = K.make([rng.randrange(P) for _ in range(K.n)])
        if not K.is_zero(v):
            return v


def pt_in(K, vals, mode, rng, bound=IN_POINT):
    """(the model point with its raw limbs, the operand words)"""
    rs = [raws(K, v, mode, rng, bound) for v in vals]
    return tuple(co_in(K, r) for r in rs), flat(flat(rs))


def pt_raw(K, rs):
    return tuple(co_in(K, r) for r in rs), flat(flat(rs))


def aff_of(K, pt):
    """The affine point of a model Jacobian point (None: infinity)."""
    if K.is_zero(pt[2].v):
        return None
    zi = K.inv(pt[2].v)
    zi2 = K.mul(zi, zi)
    return (K.mul(pt[0].v, zi2), K.mul(pt[1].v, K.mul(zi2, zi)))


def gold(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))


def g2_rec(rec):
    return tuple((int(c[0], 16), int(c[1], 16)) for c in (rec["x"], rec["y"]))


def g1_rec(rec):
    return (int(rec["x"], 16), int(rec["y"], 16))


def map_outputs(n, seed):
    """n seeded outputs of the oracle's map_to_g2 (SSWU and the 3-isogeny: on the curve, outside
    the subgroup)."""
    out = []
    for i in range(n):
        for u in O.hash_to_field_fp2(b"curve28 %d %d" % (seed, i), O.DST_POP, 2):
            out.append(O.iso_map_g2(O.map_to_curve_sswu(u)))
    return out[:n]


G1MUL_FIXED = [0, 1, 2, 3, 4, 5, 7, 8, 1 << 63, (1 << 64) - 1]
K_ALL4 = sum(4 << (3 * i) for i in range(21))
K_ALL5 = sum(5 << (3 * i) for i in range(21)) | 1 << 63


def digit_scalars(rng):
    """One scalar per signed digit value and window: -3 ... 4 in windows 0 ... 20, and 0, 1, 2
    in window 21 (the top digit is bit 63 plus a carry: it takes no other value)."""
    out = []
    for i in range(22):
        for d in (range(-3, 5) if i < 21 else range(3)):
            while True:
                ds = [rng.randrange(-3, 5) for _ in range(21)] + [rng.randrange(3)]
                ds[i] = d
                k = sum(x << (3 * j) if x >= 0 else -((-x) << (3 * j)) for j, x in enumerate(ds))
                if 0 <= k < 1 << 64 and signed_digits(k) == ds:
                    break
            out.append((i, d, k))
    return out


# ---------------------------------------------------------------- case lists
def build_cases(seed=2828):
    rng = random.Random(seed)
    cs = []
    gid = [0]

    def add(ops, cls, words, items, scalar=0, oracle=None):
        gid[0] += 1
        for op in ops:
            cs.append(Case(op, cls, words, items, scalar=scalar, group=gid[0] if len(ops) > 1 else None,
                           oracle=oracle))

    so = gold("small_order")
    g2_small = []
    for e in so["e2"]:
        for name in ("T", "negT", "T_plus_gen"):
            g2_small.append((e["order"], name, g2_rec(e[name])))
    t11 = g1_rec(next(e for e in so["e1"] if e["order"] == 11)["T"])
    g2_pts = [O.g2_mul(O.G2_GEN, rng.randrange(1, 1 << 64)) for _ in range(12)] + map_outputs(6, seed)
    g1_pts = [O.g1_mul(O.G1_GEN, rng.randrange(1, 1 << 64)) for _ in range(8)] + [t11, O.g1_mul(t11, 4)]
    pts = {K1: g1_pts, K2: g2_pts}
    pick = lambda K: rng.choice(pts[K])

    # ---- jac_dbl28, jac_neg, psi, psi2, the conversions: random / top / all at the top / full limbs
    for K, pre in ((K2, "g2"), (K1, "g1")):
        for mode, cnt in (("canon", 8), ("top", 8), ("topall", 1)):
            cls = {"canon": "random", "top": "top", "topall": "top all"}[mode]
            for _ in range(cnt):
                a = pick(K)
                p, w = pt_in(K, jac_of(K, a, rnd_k(K, rng)), mode, rng)
                add((pre + "_dbl", pre + "_dbl_rp"), cls, w, items_pt(K, m_dbl(K, p)), oracle=(("dbl", a), K, m_dbl(K, p)))
                add((pre + "_neg",), cls, w, items_pt(K, m_neg(K, p)), oracle=(("neg", a), K, m_neg(K, p)))
                if K is K2:
                    add(("psi",), cls, w, items_pt(K, m_psi(p)), oracle=(("psi", a), K, m_psi(p)))
                    add(("psi2",), cls, w, items_pt(K, m_psi2(p)), oracle=(("psi2", a), K, m_psi2(p)))
                    ta = m_to_aff(p)
                    add(("to_aff",), cls, w, items_pt(K, ta), oracle=(("id", a), K, (ta[0], ta[1], co_one(K))))
                    add(("g2j_rt",), cls, w, [("exact", words12(int_of(l))) for l in _fes(w)] +
                        [("exact", l) for l in _fes(w)])
                    add(("g2j_out",), cls, w, [("exact", words12(int_of(l) * RINV % P * R384 % P)) for l in _fes(w)])
        fullp = [[full_pattern(IN_POINT)] * K.n] * 3
        p, w = pt_raw(K, fullp)
        add((pre + "_dbl", pre + "_dbl_rp"), "top full", w, items_pt(K, m_dbl(K, p)))
        add((pre + "_neg",), "top full", w, items_pt(K, m_neg(K, p)))
        if K is K2:
            add(("psi",), "top full", w, items_pt(K, m_psi(p)))
            add(("psi2",), "top full", w, items_pt(K, m_psi2(p)))
            add(("to_aff",), "top full", w, items_pt(K, m_to_aff(p)))
        # the doubling of an infinite point (Z = 0, p, 2p): Z3 = 0 mod p
        for k in (0, 1, 2):
            rs = [raws(K, rnd_k(K, rng), "canon", rng), raws(K, rnd_k(K, rng), "canon", rng), [raw_of(0, k)] * K.n]
            p, w = pt_raw(K, rs)
            add((pre + "_dbl", pre + "_dbl_rp"), "inf Z=%s" % ("0", "p", "2p")[k], w, items_pt(K, m_dbl(K, p)))
            if K is K2:
                ta = m_to_aff(p)
                add(("to_aff",), "inf Z=%s" % ("0", "p", "2p")[k], w, items_pt(K, ta))
                add(("psi",), "inf Z=%s" % ("0", "p", "2p")[k], w, items_pt(K, m_psi(p)))

    # ---- jac_add28 (G2, G1) and jac_add_aff28 (G2): generic and every degenerate branch
    infz = {"Z=0": 0, "Z=p": 1, "Z=2p": 2}

    def inf_rs(K, k):  # an infinite point: any X, Y, and Z = k p in raw limbs
        return [raws(K, rnd_k(K, rng), "canon", rng), raws(K, rnd_k(K, rng), "canon", rng), [raw_of(0, k)] * K.n]

    for K, pre in ((K2, "g2"), (K1, "g1")):
        ops = (pre + "_add", pre + "_add_ra")

        def add_case(cls, pa, wa, pb, wb, oa, ob):
            r = m_add(K, pa, pb)
            add(ops, cls, wa + wb, items_pt(K, r), oracle=(("add", oa, ob), K, r))

        for mode, cnt in (("canon", 8), ("top", 8), ("topall", 1)):
            cls = {"canon": "random", "top": "top", "topall": "top all"}[mode]
            for _ in range(cnt):
                a, b = pick(K), pick(K)
                while a == b:
                    b = pick(K)
                pa, wa = pt_in(K, jac_of(K, a, rnd_k(K, rng)), mode, rng)
                pb, wb = pt_in(K, jac_of(K, b, rnd_k(K, rng)), mode, rng)
                add_case(cls, pa, wa, pb, wb, a, b)
        pa, wa = pt_raw(K, [[full_pattern(IN_POINT)] * K.n] * 3)
        pb, wb = pt_raw(K, [[limbs_of(int_of(full_pattern(IN_POINT)) - 1 - j)] * K.n for j in range(3)])
        add(ops, "top full", wa + wb, items_pt(K, m_add(K, pa, pb)))
        for j in range(6):
            mode = ("canon", "top", "topall")[j % 3]
            a = pick(K) if j < 4 else (g2_small[3 * (j - 4)][2] if K is K2 else t11)
            pa, wa = pt_in(K, jac_of(K, a, rnd_k(K, rng)), mode, rng)
            pb, wb = pt_in(K, jac_of(K, a, rnd_k(K, rng)), mode, rng)
            add_case("dbl branch", pa, wa, pb, wb, a, a)
            na = (a[0], K.neg(a[1]))
            pb, wb = pt_in(K, jac_of(K, na, rnd_k(K, rng)), mode, rng)
            add_case("neg branch", pa, wa, pb, wb, a, na)
        for name, k in infz.items():
            a = pick(K)
            pf, wf = pt_in(K, jac_of(K, a, rnd_k(K, rng)), "top", rng)
            pi, wi = pt_raw(K, inf_rs(K, k))
            add_case("a inf " + name, pi, wi, pf, wf, None, a)
            add_case("b inf " + name, pf, wf, pi, wi, a, None)
            pj, wj = pt_raw(K, inf_rs(K, (k + 1) % 3))
            add_case("both inf", pi, wi, pj, wj, None, None)
    K = K2
    mops_t, mops_f = ("g2_madd_t", "g2_madd_t_ra"), ("g2_madd_f", "g2_madd_f_ra")

    def madd_case(cls, pa, wa, pb, wb, oa, ob, finite_b=True):
        r = m_madd(K, pa, pb, True)
        add(mops_t, cls, wa + wb, items_pt(K, r), oracle=(("add", oa, ob), K, r))
        if finite_b:
            r = m_madd(K, pa, pb, False)
            add(mops_f, cls, wa + wb, items_pt(K, r), oracle=(("add", oa, ob), K, r))

    for mode, cnt in (("canon", 8), ("top", 8), ("topall", 1)):
        cls = {"canon": "random", "top": "top", "topall": "top all"}[mode]
        for _ in range(cnt):
            a, b = pick(K), pick(K)
            while a == b:
                b = pick(K)
            pa, wa = pt_in(K, jac_of(K, a, rnd_k(K, rng)), mode, rng)
            pb, wb = pt_in(K, b, mode, rng)
            madd_case(cls, pa, wa, pb, wb, a, b)
    pa, wa = pt_raw(K, [[full_pattern(IN_POINT)] * 2] * 3)
    pb, wb = pt_raw(K, [[limbs_of(int_of(full_pattern(IN_POINT)) - 1 - j)] * 2 for j in range(2)])
    r = m_madd(K, pa, pb, True)
    add(mops_t + mops_f, "top full", wa + wb, items_pt(K, r))
    for j in range(6):
        mode = ("canon", "top", "topall")[j % 3]
        a = pick(K) if j < 4 else g2_small[3 * (j - 4)][2]
        pa, wa = pt_in(K, jac_of(K, a, rnd_k(K, rng)), mode, rng)
        pb, wb = pt_in(K, a, mode, rng)
        madd_case("dbl branch", pa, wa, pb, wb, a, a)
        na = (a[0], K.neg(a[1]))
        pb, wb = pt_in(K, na, mode, rng)
        madd_case("neg branch", pa, wa, pb, wb, a, na)
    for name, k in infz.items():
        a = pick(K)
        pi, wi = pt_raw(K, inf_rs(K, k))
        pb, wb = pt_in(K, a, "top", rng)
        madd_case("a inf " + name, pi, wi, pb, wb, None, a)
        pf, wf = pt_in(K, jac_of(K, a, rnd_k(K, rng)), "top", rng)
        z, wz = pt_raw(K, [[raw_of(0, k)] * 2] * 2)   # the affine (0, 0) as 0, p, 2p
        madd_case("b aff00" if k == 0 else "b aff00 p", pf, wf, z, wz, a, None, finite_b=False)
        madd_case("a inf b aff00", pi, wi, z, wz, None, None, finite_b=False)

    # ---- jac_eq
    for K, op in ((K2, "g2_eq"), (K1, "g1_eq")):
        def eq_case(cls, rs_a, rs_b):
            pa, wa = pt_raw(K, rs_a)
            pb, wb = pt_raw(K, rs_b)
            add((op,), cls, wa + wb, [("exact", [1 if m_eq(K, pa, pb) else 0])])

        rep = lambda a, mode: [raws(K, v, mode, rng) for v in jac_of(K, a, rnd_k(K, rng))]
        for j in range(6):
            a, b = pick(K), pick(K)
            while a == b:
                b = pick(K)
            mode = ("canon", "top", "topall")[j % 3]
            eq_case("equal", rep(a, mode), rep(a, mode))
            eq_case("different", rep(a, mode), rep(b, mode))
            eq_case("negated", rep(a, mode), rep((a[0], K.neg(a[1])), mode))
        zero3 = lambda k: [[raw_of(0, k)] * K.n] * 3
        for name, k in infz.items():
            a = pick(K)
            eq_case("inf finite", inf_rs(K, k), rep(a, "canon"))
            eq_case("finite inf", rep(a, "canon"), inf_rs(K, k))
            eq_case("inf inf", inf_rs(K, k), inf_rs(K, (k + 2) % 3))
            # X = Y = Z = 0 mod p is infinity too (Z = 0): not equal to a finite point
            eq_case("zero finite", zero3(k), rep(a, "canon"))
            eq_case("finite zero", rep(a, "canon"), zero3(k))

    # ---- g2j_of_aff28, g2a round trip, g2j_in, fe2_inv, inv, fe2_mul_3b, store12 / load12, half
    K = K2
    for mode, cnt in (("canon", 4), ("top", 4), ("topall", 1)):
        for _ in range(cnt):
            cls = {"canon": "random", "top": "top", "topall": "top all"}[mode]
            a = pick(K)
            p, w = pt_in(K, a, mode, rng)
            add(("of_aff",), cls, w, items_pt(K, m_of_aff(p)))
            add(("g2a_rt",), cls, w, [("exact", words12(int_of(l))) for l in _fes(w)] + [("exact", l) for l in _fes(w)])
    for k in (0, 1, 2):
        p, w = pt_raw(K, [[raw_of(0, k)] * 2] * 2)
        add(("of_aff",), "aff00" if k == 0 else "aff00 p", w, items_pt(K, m_of_aff(p)))
    p, w = pt_raw(K, [[raw_of(0, 1), raw_of(0, 0)], [raw_of(0, 2), raw_of(1, 0)]])  # x = 0, y = u: finite
    add(("of_aff",), "aff x=0", w, items_pt(K, m_of_aff(p)))
    for j in range(8):
        eng = [rng.randrange(P) if j < 6 else rng.choice([0, P - 1, P, R384 - 1]) for _ in range(6)]
        add(("g2j_in",), "random" if j < 6 else "edge", flat(words12(e) for e in eng),
            [("exact", F28.redc(e * F28.CIN)) for e in eng])
    fe_edges = [0, 1, P - 1]
    for j in range(12):
        if j < 9:
            v = K.make([rng.randrange(P), rng.randrange(P)])
            rs = raws(K, v, ("canon", "top", "topall")[j % 3], rng)
            cls = ("random", "top", "top all")[j % 3]
        elif j < 11:
            rs, cls = [raw_of(0, j - 9), raw_of(0, 2 * (j - 9))], "zero"
        else:
            rs, cls = [full_pattern(IN_POINT)] * 2, "top full"
        a = co_in(K, rs)
        iv = K.inv(a.v)
        add(("fe2_inv",), cls, flat(rs), items_vals(K, [iv]))
        iv1 = K1.inv(a.v[0])
        add(("inv",), cls, rs[0], items_vals(K1, [iv1], B_FE))
    add(("inv",), "top full", full_pattern(16 * P), items_vals(K1, [K1.inv(int_of(full_pattern(16 * P)) * RINV % P)], B_FE))
    for j in range(10):
        if j < 8:
            rs = [limbs_of(rng.randrange(IN_3B if j % 2 else P)) for _ in range(2)]
            cls = "top" if j % 2 else "random"
        else:
            rs = [full_pattern(IN_3B)] * 2 if j == 8 else [limbs_of(0), full_pattern(IN_3B)]
            cls = "top full"
        add(("mul_3b",), cls, flat(rs), items_vals(K, [m_mul_3b(co_in(K, rs).v)]))
    for j in range(12):
        x = [0, 1, P - 1, P, R384 - 1, (1 << 383) + 5][j] if j < 6 else rng.randrange(R384)
        add(("store12",), "edge" if j < 6 else "random", limbs_of(x), [("exact", words12(x))])
        add(("load12",), "edge" if j < 6 else "random", words12(x), [("exact", limbs_of(x))])
    halves = [("0", 0), ("1", 1), ("p-1", P - 1), ("p", P), ("top", IN_LINE_T - 1), ("top even", IN_LINE_T - 2)]
    halves += [("odd", rng.randrange(P) | 1) for _ in range(5)] + [("even", rng.randrange(P) & ~1) for _ in range(5)]
    halves += [("full limbs", int_of(full_pattern(IN_LINE_T))), ("full limbs even", int_of(full_pattern(IN_LINE_T)) - 1)]
    for cls, x in halves:
        assert x < IN_LINE_T
        h = (x + (P if x & 1 else 0)) >> 1
        add(("half",), cls, limbs_of(x), [("exact", limbs_of(h))])
    for (c0, x0), (c1, x1) in zip(halves, halves[1:] + halves[:1]):
        add(("fe2_half",), c0 + " / " + c1, limbs_of(x0) + limbs_of(x1),
            [("exact", limbs_of((x + (P if x & 1 else 0)) >> 1)) for x in (x0, x1)])

    # ---- the line steps: T homogeneous (x l : y l : l), coordinates < 1.03 p
    def line_items(L, T2):
        return items_vals(K2, list(L) + list(T2))

    for mode, cnt in (("canon", 8), ("top", 8), ("topall", 2)):
        cls = {"canon": "random", "top": "top", "topall": "top all"}[mode]
        for _ in range(cnt):
            a, q = rng.sample(g2_pts[:12], 2)
            lam = rnd_k(K2, rng)
            if mode != "canon":  # a small Z, so that Z + p is inside T's bound
                lam = (rng.randrange(IN_LINE_T - P) * RINV % P, rng.randrange(IN_LINE_T - P) * RINV % P)
            T = (K2.mul(a[0], lam), K2.mul(a[1], lam), lam)
            rs = [raws(K2, v, mode, rng, IN_LINE_T) for v in T]
            rq = [raws(K2, v, "canon", rng) for v in q]
            w = flat(flat(rs)) + flat(flat(rq))
            Tv = tuple(co_in(K2, r).v for r in rs)
            add(("line_dbl",), cls, w, line_items(*m_line_dbl(Tv)), oracle=(("hdbl", a), K2, m_line_dbl(Tv)[1]))
            add(("line_add",), cls, w, line_items(*m_line_add(Tv, q)), oracle=(("hadd", a, q), K2, m_line_add(Tv, q)[1]))
    rs = [[full_pattern(IN_LINE_T)] * 2] * 3
    rq = [[limbs_of(int_of(full_pattern(IN_LINE_T)) - 7)] * 2] * 2
    Tv = tuple(co_in(K2, r).v for r in rs)
    qv = tuple(co_in(K2, r).v for r in rq)
    add(("line_dbl",), "top full", flat(flat(rs)) + flat(flat(rq)), line_items(*m_line_dbl(Tv)))
    add(("line_add",), "top full", flat(flat(rs)) + flat(flat(rq)), line_items(*m_line_add(Tv, qv)))
    for j in range(8):
        q = g2_pts[j]
        rq = [raws(K2, v, "canon" if j < 6 else "topall", rng, IN_LINE_T) for v in q]
        Ls, T = m_line_chain(q)
        add(("line_chain",), "random" if j < 6 else "top all", flat(flat(rq)),
            items_vals(K2, [c for L in Ls for c in L] + list(T)), oracle=(("chain", q), K2, (Ls, T)))

    # ---- [|x|] chain and membership
    def xabs_cases(cls, a, mode):
        p, w = pt_in(K2, a, mode, rng)
        r = m_xabs(p)
        add(("xabs",), cls, w, items_pt(K2, r) * 2, oracle=(("mul", a, X_ABS), K2, r))
        add(("in_group",), cls, w, [("exact", [1 if m_in_group(p) else 0])], oracle=(("in_group", a), K2, None))

    for j in range(8):
        xabs_cases("in group", g2_pts[j], ("canon", "top", "topall")[j % 3])
    for j in range(6):
        xabs_cases("map output", g2_pts[12 + j], ("canon", "top", "topall")[j % 3])
    for j, (order, name, a) in enumerate(g2_small):
        xabs_cases("small order %d" % order, a, ("canon", "topall", "top")[j % 3])
    for k in (0, 1, 2):
        p, w = pt_raw(K2, [[raw_of(0, k)] * 2] * 2)
        add(("xabs",), "aff00" if k == 0 else "aff00 p", w, items_pt(K2, m_xabs(p)) * 2)

    # ---- clearing: P = Q0 + Q1 of seeded map outputs; Q0 = Q1; Q0 = -Q1 (P infinite); one Q infinite
    maps = map_outputs(16, seed + 1)
    pairs = [("Q0 + Q1", maps[2 * j], maps[2 * j + 1]) for j in range(6)]
    pairs += [("Q0 = Q1", maps[12], maps[12]), ("Q0 = -Q1", maps[13], (maps[13][0], K2.neg(maps[13][1]))),
              ("Q0 inf", None, maps[14]), ("Q1 inf", maps[15], None)]
    for j, (cls, q0, q1) in enumerate(pairs):
        mode = ("canon", "top", "topall")[j % 3]
        p0, w0 = pt_in(K2, jac_of(K2, q0, rnd_k(K2, rng)), mode, rng)
        p1, w1 = pt_in(K2, jac_of(K2, q1, rnd_k(K2, rng)), mode, rng)
        pj = m_add(K2, p0, p1)   # the pre stage: jac_add, jac_to_aff28
        add(("g2_add", "g2_add_ra"), "clear pre " + cls, w0 + w1, items_pt(K2, pj), oracle=(("add", q0, q1), K2, pj))
        # the stages take canonical images of the values the previous stage returns
        canon = lambda pt: pt_in(K2, [c.v for c in pt], "canon", rng)
        pjc, wj = canon(pj)
        ta = m_to_aff(pjc)
        add(("to_aff",), "clear pre " + cls, wj, items_pt(K2, ta))
        pa, wa = canon(ta)
        x1, wx1 = canon(m_xabs(pa))
        psum = O.g2_add(q0, q1)
        add(("xabs",), "clear " + cls, wa, items_pt(K2, m_xabs(pa)) * 2, oracle=(("mul", psum, X_ABS), K2, m_xabs(pa)))
        t2a, T = m_clear_mid(pa, x1)
        add(("clear_mid",), cls, wa + wx1, items_pt(K2, t2a) + items_pt(K2, T), oracle=(("mid", psum), K2, (t2a, T)))
        t2c, wt2 = canon(t2a)
        x2, wx2 = canon(m_xabs(t2c))
        Tc, wT = canon(T)
        h = m_clear_post(x2, Tc)
        add(("clear_post",), cls, wx2 + wT, items_pt(K2, h), oracle=(("clear", psum), K2, h))
        pm, wm = pt_in(K2, [c.v for c in pj], mode, rng)
        h = m_clear_staged(pm)
        add(("clear_staged",), cls, wm, items_pt(K2, h), oracle=(("clear", psum), K2, h))
        h = m_clear_full(pm)
        add(("clear_full",), cls, wm, items_pt(K2, h), oracle=(("clear", psum), K2, h))

    # ---- g1_mul_u64_w3_28 then g1s_from_jac28 (engine form, canonical: exact)
    def g1mul_case(cls, base, k):
        w = flat(words12(c * R384 % P) for c in base)
        bco = tuple(Co(c, None) for c in base)
        r = m_g1mul(bco, k)
        if K1.is_zero(r[2].v):
            vals = [0, 0, 0]
        else:
            z = r[2].v
            vals = [r[0].v * z % P, r[1].v, z * z * z % P]
        add(("g1mul",), cls, w, [("exact", words12(v * R384 % P)) for v in vals], scalar=k,
            oracle=(("mul", None if base == (0, 0) else base, k), K1, r))

    gen_pt = g1_pts[0]
    for base, bn in ((t11, "order 11"), (gen_pt, "in group")):
        for k in G1MUL_FIXED:
            g1mul_case("fixed " + bn, base, k)
        g1mul_case("all 4 " + bn, base, K_ALL4)
        g1mul_case("all 5 " + bn, base, K_ALL5)
    for j, (i, d, k) in enumerate(digit_scalars(rng)):
        g1mul_case("digit", t11 if j % 2 else gen_pt, k)
    for j in range(64):
        g1mul_case("random", t11 if j % 2 else g1_pts[1 + j % 7], rng.randrange(1 << 64))
    for k in (0, 1, 5, (1 << 64) - 1):
        g1mul_case("base 00", (0, 0), k)

    # ---- g1h28: (x : y : c), coordinates < 1.03 p
    def hpt(a, mode):
        """(x l : y l : l) raw; top: one coordinate small enough for its + p image"""
        lam = rng.randrange(1, P)
        if a is None:
            vals = [rng.randrange(P), rng.randrange(1, P), 0]
        else:
            if mode != "canon":
                j = rng.randrange(3)
                small = rng.randrange(1, IN_LINE_T - P) * RINV % P
                lam = small * pow((a[0], a[1], 1)[j], -1, P) % P
            vals = [a[0] * lam % P, a[1] * lam % P, lam]
        return [raws(K1, v, mode, rng, IN_LINE_T) for v in vals]

    hops = ("g1h_add", "g1h_add_ra", "g1h_add_rb")

    def hadd(cls, ra, rb, oa, ob):
        pa, wa = pt_raw(K1, ra)
        pb, wb = pt_raw(K1, rb)
        r = m_g1h_add(pa, pb)
        add(hops, cls, wa + wb, items_pt(K1, r), oracle=(("hadd1", oa, ob), K1, r))

    for mode, cnt in (("canon", 8), ("topall", 8)):
        for _ in range(cnt):
            a, b = rng.choice(g1_pts), rng.choice(g1_pts)
            hadd("random" if mode == "canon" else "top", hpt(a, mode), hpt(b, mode), a, b)
    pa, wa = pt_raw(K1, [[full_pattern(IN_LINE_T)]] * 3)
    pb, wb = pt_raw(K1, [[limbs_of(int_of(full_pattern(IN_LINE_T)) - 1 - j)] for j in range(3)])
    add(hops, "top full", wa + wb, items_pt(K1, m_g1h_add(pa, pb)))
    for j in range(4):
        a = rng.choice(g1_pts) if j < 3 else t11
        mode = "canon" if j % 2 else "topall"
        hadd("dbl branch", hpt(a, mode), hpt(a, mode), a, a)
        hadd("neg branch", hpt(a, mode), hpt((a[0], -a[1] % P), mode), a, (a[0], -a[1] % P))
    for name, k in infz.items():
        a = rng.choice(g1_pts)
        ri = lambda kk: [raws(K1, rng.randrange(P), "canon", rng), raws(K1, rng.randrange(1, P), "canon", rng), [raw_of(0, kk)]]
        hadd("a inf " + name, ri(k), hpt(a, "canon"), None, a)
        hadd("b inf " + name, hpt(a, "canon"), ri(k), a, None)
        hadd("both inf", ri(k), ri((k + 1) % 3), None, None)
        z = [[raw_of(0, k)]] * 3
        hadd("a zero", z, hpt(a, "canon"), None, a)
    for j in range(8):
        eng = [rng.randrange(P) if j < 6 else rng.choice([0, P - 1, P, R384 - 1]) for _ in range(3)]
        add(("g1h_load",), "random" if j < 6 else "edge", flat(words12(e) for e in eng),
            [("exact", limbs_of(e)) for e in eng])
    for j in range(12):
        if j < 8:
            rs = hpt(rng.choice(g1_pts), "canon" if j % 2 else "topall")
            cls = "random" if j % 2 else "top"
        elif j < 11:
            rs, cls = [raws(K1, rng.randrange(P), "canon", rng), raws(K1, rng.randrange(P), "canon", rng),
                       [raw_of(0, j - 8)]], "inf " + ("Z=0", "Z=p", "Z=2p")[j - 8]
        else:
            rs, cls = [[full_pattern(IN_LINE_T)]] * 3, "top full"
        vals = [int_of(r[0]) * RINV % P for r in rs]
        if vals[2] == 0:
            vals = [0, 0, 0]
        add(("g1h_store",), cls, flat(flat(rs)), [("exact", words12(v * R384 % P)) for v in vals])
    return cs


def _fes(words):
    return [words[N * i:N * i + N] for i in range(len(words) // N)]


RAGGED = 64 + 37


def build_orders(seed=2828):
    """(interleaved, sorted, ragged): every 64-lane wave of the interleaved file mixes ops, the
    generic case and the degenerate branches; the same cases sorted by op and class (uniform
    waves); and 101 of them in interleaved order, the first case of every op among them (the
    last wave holds 37 lanes)."""
    cs = build_cases(seed)
    by_op = {}
    for c in cs:
        by_op.setdefault(c.op, {}).setdefault(c.cls, []).append(c)
    inter = F28.spread([F28.spread(list(by_cls.values())) for _, by_cls in sorted(by_op.items(), key=lambda t: OPS[t[0]])])
    # a stride walk over the spread list: every wave samples the whole list, so the small classes
    # (the degenerate branches sit in the middle of their op's spread) reach every wave
    n = len(inter)
    assert n % 61
    inter = [inter[(i * 61) % n] for i in range(n)]
    srt = sorted(inter, key=lambda c: (OPS[c.op], c.cls, c.id))
    pick, seen = set(), set()
    for c in inter:
        if c.op not in seen:
            seen.add(c.op)
            pick.add(c.id)
    for c in inter:
        if len(pick) < RAGGED:
            pick.add(c.id)
    return inter, srt, [c for c in inter if c.id in pick]


def write_cases(path, cases):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for c in cases:
            fh.write(pack_words(c.record()))


def model_output(cases):
    """An OUT file that passes: the exact words, and the canonical image of every residue."""
    out = []
    for c in cases:
        for it in c.items:
            out.append(pack_words(it[1] if it[0] == "exact" else limbs_of(it[1])))
    return b"".join(out)


# ---------------------------------------------------------------- comparator
class Report(F28.Report):
    pass


def check_case(c, got):
    """None, or what is wrong with the case's result bytes."""
    w = struct.unpack("<%dI" % (len(got) // 4), got)
    o = 0
    for k, it in enumerate(c.items):
        if it[0] == "exact":
            e = it[1]
            g = w[o:o + len(e)]
            o += len(e)
            if list(g) != list(e):
                bad = [i for i in range(len(e)) if g[i] != e[i]]
                return "item %d: %d words differ, first word %d: %#x, expected %#x" % (k, len(bad), bad[0], g[bad[0]], e[bad[0]])
            continue
        l = w[o:o + N]
        o += N
        if max(l) > M28:
            return "item %d: a limb >= 2^28" % k
        x = int_of(l)
        if x >= it[2]:
            return "item %d: value %.4f p, bound %.2f p" % (k, x / P, it[2] / P)
        if x % P != it[1]:
            return "item %d: wrong residue" % k
    return None


def compare(cases, out, ops=None):
    """Every result of every case (of `ops`, default all).  `out` is the checker's whole OUT
    file; its length must be the cases' exactly."""
    need = sum(c.out_bytes() for c in cases)
    assert len(out) == need, "OUT is %d bytes, the cases need %d" % (len(out), need)
    rep, o = Report(), 0
    for c in cases:
        got = out[o:o + c.out_bytes()]
        o += c.out_bytes()
        if ops is not None and c.op not in ops:
            continue
        rep.compared[c.op] = rep.compared.get(c.op, 0) + 1
        rep.words[c.id] = got
        what = check_case(c, got)
        if what:
            rep.mismatch.setdefault((c.op, c.cls), []).append((c.id, what))
    return rep


def group_disagreements(cases, rep):
    """Cases built on the same operands (r fresh and r aliased) whose result words differ."""
    by = {}
    for c in cases:
        if c.group is not None and c.id in rep.words:
            by.setdefault(c.group, []).append(c)
    return by, [(g, sorted(c.op for c in cs)) for g, cs in by.items() if len({rep.words[c.id] for c in cs}) > 1]


def main(argv):
    """curve28_vectors.py write DIR: the three case files; check ORDER OUT: compare;
    stats: case counts per op and class."""
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
    if len(argv) == 2 and argv[1] == "stats":
        n = {}
        for c in inter:
            n.setdefault(c.op, {}).setdefault(c.cls, 0)
            n[c.op][c.cls] += 1
        print("%d cases" % len(inter))
        for op in OP_LIST:
            print(op, sum(n[op].values()), n[op])
        return 0
    print(main.__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv))
