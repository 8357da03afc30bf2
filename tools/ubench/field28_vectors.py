"""Cases, integer reference and comparator for tools/ubench/field28_check
(tests/test_gpu_field28.py, tests/test_field28_vectors.py).

The checker runs the radix-2^28 field layer (grandine_amd/csrc/bls_field28.h) on the GPU, one case
per lane, on RAW limb images (14 words per fe, nothing converted), through the public r28::
functions, so that the device branch (the generated v_mad_u64_u32 products of bls_fpmul28_gen.h)
is what runs.  Everything it returns is recomputed here with Python integers; nothing is imported
from the engine.

Primitives (mul, sqr, mul2, mul4, mul6, fe2_mul3k): EXACT.  Product-scanning REDC returns the
unique integer (T + m p) / 2^392 with m = -T p^-1 mod 2^392, T the sum of the operand products
read as integers (fe2_mul3k: T0 = A - B + 17 p^2, T1 = C - A - B).  Output limbs 0..12 are that
integer's 28-bit digits, limb 13 the rest; every word must match.  The module also runs an
integer model of the column loop (mul_n of the header, the signed two-accumulator loop of
tools/gen_fpmul28.py emit_kara3) and records the peak of every 64-bit accumulator.

Composites (fe2_mul ... fe12_mul_034_kara_st and the Miller chains): the representative depends
on the internal sequence, so each output coefficient is checked for its residue mod p against the
plain Fp / Fp2 / Fp12 formula (Fp12 = Fp2[w] / (w^6 - xi) as a polynomial product), the limb
contract (every limb < 2^28) and the value bound the header states.  sp_from_engine, from_fp,
to_fp, fe12_to_engine_scaled and fp_pow_pm3d4 are single products or canonical: exact words.

An fe with integer X stands for X 2^-392 mod p, so a product formula's expectation is the formula
on the operand integers times 2^-392."""
import os
import random
import struct
import sys
from operator import mul as _mul

P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
N = 14
M28 = (1 << 28) - 1
M32 = (1 << 32) - 1
R = 1 << 392
RINV = pow(R, -1, P)
R384 = 1 << 384
NPINV = (-pow(P, -1, R)) % R          # -p^-1 mod 2^392
PINV28 = NPINV & M28                  # the header's kPinv
CIN = (1 << 400) % P                  # GBLS_R28_CIN
COUT = R384 % P                       # GBLS_R28_COUT
BIAS_KARA = 17 * P * P
PM3D4 = (P - 3) // 4
IN_WORDS = 4 + 252
CHAIN_STEPS = 30
TOP_SHIFT = 28 * 13


def limbs_of(v):
    """28-bit digits, the rest in limb 13 (a normalized image)."""
    assert 0 <= v < 1 << (TOP_SHIFT + 32)
    return [(v >> (28 * i)) & M28 for i in range(13)] + [v >> TOP_SHIFT]


def int_of(l):
    return sum(int(x) << (28 * i) for i, x in enumerate(l))


def words12(v):
    assert 0 <= v < R384
    return [(v >> (32 * i)) & M32 for i in range(12)]


def int12(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


P_L = limbs_of(P)


def make_bias(m, b):
    """m p with every limb but the top raised by b 2^28 (the header's make_bias)."""
    r = limbs_of(m * P)
    for i in range(13):
        r[i] += b << 28
        r[i + 1] -= b
    return r


BIAS4P = make_bias(4, 1)


def add_lazy(a, b):
    return [x + y for x, y in zip(a, b)]


def neg_lazy(a):
    r = [x - y for x, y in zip(BIAS4P, a)]
    assert min(r) >= 0
    return r


# ---------------------------------------------------------------- the exact value
def redc(T):
    """(T + m p) / 2^392, m = -T p^-1 mod 2^392, as limbs (13 digits and the rest)."""
    m = (T * NPINV) % R
    q, rem = divmod(T + m * P, R)
    assert rem == 0 and q >= 0
    return limbs_of(q)


def exact_product(pairs):
    return redc(sum(int_of(x) * int_of(y) for x, y in pairs))


def exact_mul3k(xs, us):
    """xs, us: three (c0, c1) limb pairs each -> (r0 limbs, r1 limbs)."""
    A = sum(int_of(x[0]) * int_of(u[0]) for x, u in zip(xs, us))
    B = sum(int_of(x[1]) * int_of(u[1]) for x, u in zip(xs, us))
    C = sum((int_of(x[0]) + int_of(x[1])) * (int_of(u[0]) + int_of(u[1])) for x, u in zip(xs, us))
    return redc(A - B + BIAS_KARA), redc(C - A - B)


# ---------------------------------------------------------------- the column loops
def _col(x, yr, k):
    """sum over i + j = k of x[i] y[j]; yr is y reversed."""
    lo, hi = max(0, k - 13), min(k, 13)
    return sum(map(_mul, x[lo:hi + 1], yr[13 - k + lo:14 - k + hi]))


def model_mul_n(pairs):
    """The header's mul_n<NP> with an unbounded accumulator -> (limbs, peak accumulator).  The
    device products (fe_mul_dev ... fe_mul6_dev) add the same terms in the same column order, and
    fe_sqr_dev adds the same column sums (the cross terms once, doubled)."""
    prs = [(x, y[::-1]) for x, y in pairs]
    m, t = [0] * N, [0] * N
    mr = None
    acc = peak = 0
    PR = P_L[::-1]
    for k in range(27):
        for x, yr in prs:
            acc += _col(x, yr, k)
        # m[i] P[k - i] for i < k: m[k] is still zero here, so the full column sum is the same
        acc += _col(m, PR, k)
        if k < N:
            m[k] = (((acc & M32) * PINV28) & M32) & M28
            acc += m[k] * P_L[0]
        else:
            t[k - N] = acc & M28
        peak = max(peak, acc)
        acc >>= 28
    assert acc <= M32
    t[13] = acc
    return t, peak


def model_mul3k(xs, us):
    """fe2_mul3k_dev's loop: a, b formed apart, C into acc1, acc0 += a - b + bias_k (signed),
    acc1 -= a + b, the two reductions, an arithmetic shift of acc0
    -> (r0, r1, peaks {a, b, acc1, acc0: max |acc0|}, the columns where acc0 went negative)."""
    bias = [(BIAS_KARA >> (28 * k)) & M28 for k in range(28)]
    assert BIAS_KARA >> (28 * 28) == 0
    xa = [x[0] for x in xs]
    xb = [x[1] for x in xs]
    xs_ = [add_lazy(x[0], x[1]) for x in xs]
    ua = [u[0][::-1] for u in us]
    ub = [u[1][::-1] for u in us]
    us_ = [add_lazy(u[0], u[1])[::-1] for u in us]
    PR = P_L[::-1]
    m0, m1, t0, t1 = [0] * N, [0] * N, [0] * N, [0] * N
    acc0 = acc1 = 0
    peaks = {"a": 0, "b": 0, "acc1": 0, "acc0": 0}
    neg = []
    for k in range(27):
        a = sum(_col(xa[q], ua[q], k) for q in range(3))
        b = sum(_col(xb[q], ub[q], k) for q in range(3))
        acc1 += sum(_col(xs_[q], us_[q], k) for q in range(3))
        peaks["a"], peaks["b"], peaks["acc1"] = max(peaks["a"], a), max(peaks["b"], b), max(peaks["acc1"], acc1)
        acc0 += a - b + bias[k]
        was_neg = acc0 < 0
        peaks["acc0"] = max(peaks["acc0"], abs(acc0))
        acc1 -= a + b
        assert acc1 >= 0
        acc0 += _col(m0, PR, k)
        acc1 += _col(m1, PR, k)
        if k < N:
            m0[k] = (((acc0 & M32) * PINV28) & M32) & M28
            acc0 += m0[k] * P_L[0]
            m1[k] = (((acc1 & M32) * PINV28) & M32) & M28
            acc1 += m1[k] * P_L[0]
        else:
            t0[k - N] = acc0 & M28
            t1[k - N] = acc1 & M28
        peaks["acc0"], peaks["acc1"] = max(peaks["acc0"], abs(acc0)), max(peaks["acc1"], acc1)
        if was_neg or acc0 < 0:
            neg.append(k)
        acc0 >>= 28  # arithmetic
        acc1 >>= 28
    t0[13] = (acc0 + bias[27]) & M32
    assert 0 <= acc0 + bias[27] <= M32 and acc1 <= M32
    t1[13] = acc1
    return t0, t1, peaks, neg


# ---------------------------------------------------------------- ops
OP_LIST = ["mul", "mul_ra", "mul_rb", "mul_aa", "sqr", "sqr_ra", "mul2", "mul2_rc", "mul4", "mul6", "mul3k",
           "fe2_mul", "fe2_mul_ra", "fe2_sqr", "fe2_mul_fe", "sp_from_engine", "sp_mul_sp_lazy", "sp_mul_sp",
           "m034", "m034_st", "m034_lazy", "m034_lazy_st", "m034_kara_st", "to_engine_scaled",
           "from_fp", "to_fp", "pow_pm3d4", "chain"]
OPS = {n: i for i, n in enumerate(OP_LIST)}
FORMS = ["m034", "m034_st", "m034_lazy", "m034_lazy_st", "m034_kara_st"]  # a chain's aux
CHAIN_FORMS = ("m034_st", "m034_lazy_st", "m034_kara_st")
# the header's functions and the forms they are called in
FUNCS = {"mul": ("mul", "mul_ra", "mul_rb", "mul_aa"), "sqr": ("sqr", "sqr_ra"), "mul2": ("mul2", "mul2_rc"),
         "mul4": ("mul4",), "mul6": ("mul6",), "fe2_mul3k": ("mul3k",),
         "fe2_mul": ("fe2_mul", "fe2_mul_ra"), "fe2_sqr": ("fe2_sqr",), "fe2_mul_fe": ("fe2_mul_fe",),
         "sp_from_engine": ("sp_from_engine",), "sp_mul_sp_lazy": ("sp_mul_sp_lazy",), "sp_mul_sp": ("sp_mul_sp",),
         "fe12_mul_034": ("m034",), "fe12_mul_034_st": ("m034_st",), "fe12_mul_034_lazy": ("m034_lazy",),
         "fe12_mul_034_lazy_st": ("m034_lazy_st",), "fe12_mul_034_kara_st": ("m034_kara_st",),
         "fe12_to_engine_scaled": ("to_engine_scaled",), "from_fp": ("from_fp",), "to_fp": ("to_fp",),
         "fp_pow_pm3d4": ("pow_pm3d4",), "miller_chain": ("chain",)}
FUNC_OF = {op: fn for fn, ops in FUNCS.items() for op in ops}
PRIMITIVES = ("mul", "sqr", "mul2", "mul4", "mul6", "fe2_mul3k")
# operand words read and result words written
IN_FE = {"mul": 2, "mul_ra": 2, "mul_rb": 2, "mul_aa": 1, "sqr": 1, "sqr_ra": 1, "mul2": 4, "mul2_rc": 4,
         "mul4": 8, "mul6": 12, "mul3k": 12, "fe2_mul": 4, "fe2_mul_ra": 4, "fe2_sqr": 2, "fe2_mul_fe": 3,
         "sp_mul_sp_lazy": 12, "sp_mul_sp": 12, "m034": 18, "m034_st": 18, "m034_lazy": 18, "m034_lazy_st": 18,
         "m034_kara_st": 18, "to_engine_scaled": 12, "to_fp": 1, "chain": 18}
OUT_WORDS = {"mul": 14, "mul_ra": 14, "mul_rb": 14, "mul_aa": 14, "sqr": 14, "sqr_ra": 14, "mul2": 14,
             "mul2_rc": 14, "mul4": 14, "mul6": 14, "mul3k": 28, "fe2_mul": 28, "fe2_mul_ra": 28, "fe2_sqr": 28,
             "fe2_mul_fe": 28, "sp_from_engine": 84, "sp_mul_sp_lazy": 168, "sp_mul_sp": 168, "m034": 168,
             "m034_st": 168, "m034_lazy": 168, "m034_lazy_st": 168, "m034_kara_st": 168, "to_engine_scaled": 144,
             "from_fp": 14, "to_fp": 12, "pow_pm3d4": 12, "chain": (CHAIN_STEPS + 1) * 168}
# value bounds of the outputs, in hundredths of p (header comments; fe2_sqr and fe2_mul_fe state
# none: a single reduction of T < 32 p^2 is < p (1 + 32 p / 2^392) < 1.02 p)
BOUND = {"fe2_mul": 103, "fe2_mul_ra": 103, "fe2_sqr": 102, "fe2_mul_fe": 102, "sp_mul_sp_lazy": 101,
         "sp_mul_sp": 110, "m034": 110, "m034_st": 110, "m034_lazy": 102, "m034_lazy_st": 102,
         "m034_kara_st": 103}

# operand roles of the primitives: (limb limit, value bound, exclusive)
L32 = ((1 << 29) - 1, 32 * P)                # mul, sqr, mul2: lazy limbs, values < 32 p
N11 = (M28, 11 * P // 10)                    # normalized, < 1.1 p
L51 = ((1 << 29) - 1, 51 * P // 10)          # lazy limbs, < 5.1 p
N51 = (M28, 51 * P // 10)                    # normalized, < 5.1 p
ROLES = {"mul": [L32, L32], "sqr": [L32], "mul2": [L32] * 4, "mul4": [N11, L51] * 4, "mul6": [N11, L51] * 6,
         "fe2_mul3k": [N11, N11, N51, N51] * 3}
T_LIMIT = {"mul4": 34 * P * P, "mul6": 34 * P * P}


def top_pattern(role):
    """Limbs 0..12 at the role's limit, the top limb the largest the value bound allows."""
    lim, bound = role
    low = sum(lim << (28 * i) for i in range(13))
    top = (bound - 1 - low) >> TOP_SHIFT
    assert 0 <= top <= lim
    return [lim] * 13 + [top]


def limb_limit(role, i):
    lim, bound = role
    return lim if i < 13 else min(lim, (bound - 1) >> TOP_SHIFT)


def one_hot(role, i):
    r = [0] * N
    r[i] = limb_limit(role, i)
    return r


def band(role, lo, hi):
    """Limbs lo..hi-1 at the role's limit (the top limb as far as the bound allows), the rest 0."""
    r = [0] * N
    for i in range(lo, min(hi, 13)):
        r[i] = role[0]
    if hi == N:
        r[13] = (role[1] - 1 - int_of(r)) >> TOP_SHIFT
        assert 0 <= r[13] <= role[0]
    return r


SPECIALS = {"0": 0, "raw1": 1, "mont1": R % P, "p-1": P - 1, "p": P, "2p-1": 2 * P - 1}


def rnd_role(rng, role, kind):
    """kind 'canon': a canonical element; 'lazy': for a lazy role the limbwise sum of two
    normalized elements or a 4p - a image, for a normalized role any value below its bound."""
    lim, bound = role
    if kind == "canon":
        return limbs_of(rng.randrange(P))
    if lim == M28:
        return limbs_of(rng.randrange(bound))
    if rng.random() < 0.5:
        return neg_lazy(limbs_of(rng.randrange(2 * P)))
    half = bound // 2
    return add_lazy(limbs_of(rng.randrange(half)), limbs_of(rng.randrange(half)))


def in_role(l, role):
    return all(0 <= x <= role[0] for x in l) and int_of(l) < role[1]


# ---------------------------------------------------------------- Fp2 / Fp12 on integers mod p
def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_scale(a, s):
    return (a[0] * s % P, a[1] * s % P)


XI = (1, 1)
Z2 = (0, 0)
W_OF_MEM = (0, 2, 4, 1, 3, 5)  # fe12 memory order c0.c0 c0.c1 c0.c2 c1.c0 c1.c1 c1.c2 -> power of w


def w_from_mem(c):
    w = [None] * 6
    for m in range(6):
        w[W_OF_MEM[m]] = c[m]
    return w


def mem_from_w(w):
    return [w[W_OF_MEM[m]] for m in range(6)]


def sp_w(s):
    """a0 + a2 w^2 + a3 w^3"""
    return [s[0], Z2, s[1], s[2], Z2, Z2]


def f12_mul(a, b):
    """Fp2[w] / (w^6 - xi): the polynomial product."""
    t = [Z2] * 11
    for i in range(6):
        for j in range(6):
            t[i + j] = f2_add(t[i + j], f2_mul(a[i], b[j]))
    return [f2_add(t[k], f2_mul(t[k + 6], XI)) if k < 5 else t[k] for k in range(6)]


def f12_scaled(a, s):
    return [f2_scale(c, s) for c in a]


# ---------------------------------------------------------------- cases
class Case:
    """op, class label, operand words (raw), aux; exact: the result bytes, or res: the residue
    of every output coefficient (14 words each) with bound: the value bound (exclusive)."""
    _next = 0

    def __init__(self, op, cls, words, aux=0, group=None):
        assert op in OPS and len(words) <= IN_WORDS - 4 and all(0 <= w <= M32 for w in words)
        self.op, self.cls, self.words, self.aux, self.group = op, cls, list(words), aux, group
        self.id = Case._next
        Case._next += 1
        self.exact = self.res = self.bound = self.peak = self.neg = None
        expect(self)

    def record(self):
        w = [OPS[self.op], self.aux, 0, 0] + self.words
        return w + [0] * (IN_WORDS - len(w))

    def fes(self, n=None):
        n = IN_FE[self.op] if n is None else n
        return [self.words[N * i:N * i + N] for i in range(n)]

    def out_bytes(self):
        return 4 * OUT_WORDS[self.op]


def pack_words(ws):
    return struct.pack("<%dI" % len(ws), *ws)


def _fe2s(fes):
    return [(int_of(fes[2 * i]) % P, int_of(fes[2 * i + 1]) % P) for i in range(len(fes) // 2)]


def _res_of_f2(vals):
    return [c for v in vals for c in v]


def dense_step(f_mem, s):
    """f (memory order, integers mod p) times the sparse s, over 2^392: memory order."""
    return mem_from_w(f12_scaled(f12_mul(w_from_mem(f_mem), sp_w(s)), RINV))


def expect(c):
    op = c.op
    if FUNC_OF[op] in PRIMITIVES:
        f = c.fes()
        if op in ("mul", "mul_ra", "mul_rb"):
            pairs = [(f[0], f[1])]
        elif op in ("mul_aa", "sqr", "sqr_ra"):
            pairs = [(f[0], f[0])]
        elif op == "mul3k":
            xs = [(f[4 * q], f[4 * q + 1]) for q in range(3)]
            us = [(f[4 * q + 2], f[4 * q + 3]) for q in range(3)]
            r0, r1 = exact_mul3k(xs, us)
            c.exact = pack_words(r0 + r1)
            return
        else:
            pairs = [(f[2 * q], f[2 * q + 1]) for q in range(len(f) // 2)]
        c.exact = pack_words(exact_product(pairs))
        return
    if op == "sp_from_engine":
        w = [int12(c.words[12 * i:12 * i + 12]) for i in range(9)]  # L0 L2 L3 (c0, c1), Px Py Pc
        q = {0: w[8], 1: w[6], 2: w[7]}
        out = []
        for j in range(3):
            out += redc(w[2 * j] * q[j]) + redc(w[2 * j + 1] * q[j])
        c.exact = pack_words(out)
        return
    if op == "to_engine_scaled":
        out = []
        for l in c.fes():
            x = int_of(l)
            assert x < 2 * P
            out += words12(x - P if x >= P else x)
        c.exact = pack_words(out)
        return
    if op == "from_fp":
        c.exact = pack_words(redc(int12(c.words[:12]) * CIN))
        return
    if op == "to_fp":
        c.exact = pack_words(words12(int_of(redc(int_of(c.words[:N]) * COUT)) % P))
        return
    if op == "pow_pm3d4":
        v = int12(c.words[:12]) * pow(R384, -1, P) % P
        c.exact = pack_words(words12(pow(v, PM3D4, P) * R384 % P))
        return
    c.bound = BOUND[FORMS[c.aux] if op == "chain" else op] * P // 100
    f = c.fes()
    if op in ("fe2_mul", "fe2_mul_ra"):
        a, b = _fe2s(f)
        c.res = _res_of_f2([f2_scale(f2_mul(a, b), RINV)])
    elif op == "fe2_sqr":
        (a,) = _fe2s(f)
        c.res = _res_of_f2([f2_scale(f2_mul(a, a), RINV)])
    elif op == "fe2_mul_fe":
        (a,) = _fe2s(f[:2])
        c.res = _res_of_f2([f2_scale(a, int_of(f[2]) * RINV % P)])
    elif op in ("sp_mul_sp_lazy", "sp_mul_sp"):
        v = _fe2s(f)
        c.res = _res_of_f2(mem_from_w(f12_scaled(f12_mul(sp_w(v[:3]), sp_w(v[3:])), RINV)))
    elif op in FORMS:
        v = _fe2s(f)
        c.res = _res_of_f2(dense_step(v[:6], v[6:]))
    elif op == "chain":
        v = _fe2s(f)
        s = [v[0:3], v[3:6], v[6:9]]
        acc = mem_from_w(f12_scaled(f12_mul(sp_w(s[0]), sp_w(s[1])), RINV))
        c.res = _res_of_f2(acc)
        for j in range(CHAIN_STEPS):
            acc = dense_step(acc, s[(j + 2) % 3])
            c.res += _res_of_f2(acc)
    else:
        raise KeyError(op)
    assert len(c.res) * N == OUT_WORDS[op]


def primitive_pairs(c):
    """The (x, y) limb pairs of a primitive case (not mul3k)."""
    f = c.fes()
    if c.op in ("mul_aa", "sqr", "sqr_ra"):
        return [(f[0], f[0])]
    return [(f[2 * q], f[2 * q + 1]) for q in range(len(f) // 2)]


def model(c):
    """A primitive case through the column loop -> (result words, {accumulator: peak}, columns
    where the signed accumulator was negative)."""
    if c.op == "mul3k":
        f = c.fes()
        xs = [(f[4 * q], f[4 * q + 1]) for q in range(3)]
        us = [(f[4 * q + 2], f[4 * q + 3]) for q in range(3)]
        r0, r1, peaks, neg = model_mul3k(xs, us)
        return r0 + r1, peaks, neg
    t, peak = model_mul_n(primitive_pairs(c))
    return t, {"acc": peak}, []


def in_contract(c):
    """The header contract of a primitive case's operands."""
    fn = FUNC_OF[c.op]
    f = c.fes()
    roles = ROLES[fn]
    if c.op in ("mul_aa",):
        roles = [L32]
    if not all(in_role(l, r) for l, r in zip(f, roles)) or len(f) != len(roles):
        return False
    if fn in T_LIMIT:
        return sum(int_of(x) * int_of(y) for x, y in primitive_pairs(c)) < T_LIMIT[fn]
    if fn == "fe2_mul3k":
        return sum(int_of(f[4 * q + 1]) * int_of(f[4 * q + 3]) for q in range(3)) < BIAS_KARA
    return sum(int_of(x) * int_of(y) for x, y in primitive_pairs(c)) < R * P


# ---------------------------------------------------------------- case lists
def _flat(ls):
    return [w for l in ls for w in l]


def _primitive_operand_sets(fn, rng):
    """[(class, operands)] of one primitive, without the one-hot cases."""
    roles = ROLES[fn]
    out = []
    for _ in range(16):
        out.append(("canon", [rnd_role(rng, r, "canon") for r in roles]))
    for _ in range(16):
        out.append(("lazy", [rnd_role(rng, r, "lazy") for r in roles]))
    names = list(SPECIALS)
    allowed = [[n for n in names if in_role(limbs_of(SPECIALS[n]), r)] for r in roles]
    if fn == "mul":
        for a in names:
            for b in names:
                out.append(("special", [limbs_of(SPECIALS[a]), limbs_of(SPECIALS[b])]))
    elif fn == "sqr":
        for a in names:
            out.append(("special", [limbs_of(SPECIALS[a])]))
    else:
        for j in range(12):
            ops = []
            for i, r in enumerate(roles):
                if j < len(names):  # the same value everywhere it is allowed
                    n = names[j] if names[j] in allowed[i] else "p"
                elif rng.random() < 0.7:
                    n = rng.choice(allowed[i])
                else:
                    n = None
                ops.append(limbs_of(SPECIALS[n]) if n else rnd_role(rng, r, "canon"))
            out.append(("special", ops))
    out.append(("top", [top_pattern(r) for r in roles]))
    return out


def build_primitives(seed):
    rng = random.Random(seed)
    cs = []
    g = 0

    def add(ops, cls, operands):
        nonlocal g
        g += 1
        for op in ops:
            n = IN_FE[op]
            cs.append(Case(op, cls, _flat(operands[:n]), group=g))

    for cls, o in _primitive_operand_sets("mul", rng):
        add(("mul", "mul_ra", "mul_rb"), cls, o)
        add(("mul_aa", "sqr", "sqr_ra"), cls, o[:1])
    for i in range(N):
        for j in range(N):
            add(("mul",), "onehot", [one_hot(L32, i), one_hot(L32, j)])
    for i in range(N):
        for j in range(i, N):  # two limbs of one operand: one term of the square
            a = one_hot(L32, i)
            a[j] = limb_limit(L32, j)
            if int_of(a) >= 32 * P:
                a[13] -= 2  # room for the lower limb below 32 p
            add(("sqr", "mul_aa"), "onehot", [a])
    for cls, o in _primitive_operand_sets("mul2", rng):
        add(("mul2", "mul2_rc"), cls, o)
    for fn, op, npair in (("mul2", "mul2", 2), ("mul4", "mul4", 4), ("mul6", "mul6", 6)):
        roles = ROLES[fn]
        if fn != "mul2":
            for cls, o in _primitive_operand_sets(fn, rng):
                add((op,), cls, o)
        for q in range(npair):
            for i in range(N):
                for j in range(N):
                    o = [[0] * N for _ in roles]
                    o[2 * q], o[2 * q + 1] = one_hot(roles[2 * q], i), one_hot(roles[2 * q + 1], j)
                    add((op,), "onehot", o)
    # fe2_mul3k: operands x_q.c0 x_q.c1 u_q.c0 u_q.c1
    roles = ROLES["fe2_mul3k"]
    for cls, o in _primitive_operand_sets("fe2_mul3k", rng):
        add(("mul3k",), cls, o)
    for q in range(3):
        for part in (0, 1):  # the A term and the B term of pair q (each with its C term)
            for i in range(N):
                for j in range(N):
                    o = [[0] * N for _ in roles]
                    o[4 * q + part], o[4 * q + 2 + part] = one_hot(N11, i), one_hot(N51, j)
                    add(("mul3k",), "onehot", o)
    zero = [0] * N
    tx, tu = top_pattern(N11), top_pattern(N51)
    add(("mul3k",), "A=0 B max", [zero, tx, zero, tu] * 3)
    add(("mul3k",), "B=0 A max", [tx, zero, tu, zero] * 3)
    add(("mul3k",), "A high B low", [band(N11, 7, 14), band(N11, 0, 7), band(N51, 7, 14), band(N51, 0, 7)] * 3)
    add(("mul3k",), "A low B high", [band(N11, 0, 7), band(N11, 7, 14), band(N51, 0, 7), band(N51, 7, 14)] * 3)
    add(("mul3k",), "A=0 B high", [zero, band(N11, 7, 14), zero, band(N51, 7, 14)] * 3)
    return cs


def s_elem(rng, kind):
    """A normalized coefficient < 1.1 p ("S" of the header)."""
    if kind == "canon":
        return limbs_of(rng.randrange(P))
    if kind == "s11":
        return limbs_of(rng.randrange(P, 11 * P // 10))
    if kind == "top":
        return top_pattern(N11)
    return limbs_of(rng.choice([0, 1, R % P, P - 1, P, 11 * P // 10 - 1, rng.randrange(P)]))


S_KINDS = ("canon", "canon", "s11", "top", "edge", "canon", "s11", "edge")


def build_composites(seed):
    rng = random.Random(seed)
    cs = []
    for j in range(16):
        kind = S_KINDS[j % 8]
        # fe2_mul: a limbs < 2^29 (a lazy sum), < 5p; b normalized, < 5p
        if kind == "top":
            a = [top_pattern(((1 << 29) - 1, 5 * P))] * 2
            b = [top_pattern((M28, 5 * P))] * 2
        elif kind == "canon":
            a = [limbs_of(rng.randrange(P)) for _ in range(2)]
            b = [limbs_of(rng.randrange(P)) for _ in range(2)]
        else:
            a = [add_lazy(limbs_of(rng.randrange(5 * P // 2)), limbs_of(rng.randrange(5 * P // 2))) for _ in range(2)]
            b = [limbs_of(rng.randrange(5 * P)) for _ in range(2)]
        cs.append(Case("fe2_mul", kind, _flat(a + b)))
        cs.append(Case("fe2_mul_ra", kind, _flat(a + b)))
        cs.append(Case("fe2_sqr", kind, _flat([s_elem(rng, kind) for _ in range(2)])))
        cs.append(Case("fe2_mul_fe", kind, _flat([s_elem(rng, kind) for _ in range(3)])))
        for op in ("sp_mul_sp_lazy", "sp_mul_sp"):
            cs.append(Case(op, kind, _flat([s_elem(rng, kind) for _ in range(12)])))
        fs = [s_elem(rng, kind) for _ in range(18)]
        for op in FORMS:
            cs.append(Case(op, kind, _flat(fs)))
        cs.append(Case("to_engine_scaled", kind, _flat([s_elem(rng, kind) for _ in range(12)])))
        # engine-form words: canonical images, and any word below 2^384
        eng = lambda: rng.randrange(P) if kind in ("canon", "s11") else rng.choice(
            [0, R384 % P, P - 1, P, R384 - 1, rng.randrange(R384)])
        cs.append(Case("sp_from_engine", kind, _flat([words12(eng()) for _ in range(9)])))
        cs.append(Case("from_fp", kind, words12(eng())))
        cs.append(Case("to_fp", kind, top_pattern(L32) if kind == "top" else rnd_role(rng, L32, "lazy")))
    pw = [0, R384 % P, P - 1, 2 * R384 % P, P, R384 - 1] + [rng.randrange(P) for _ in range(16)] + \
         [rng.randrange(P, R384) for _ in range(2)]
    for j, a in enumerate(pw):
        cs.append(Case("pow_pm3d4", "edge" if j < 6 else "canon" if j < 22 else "above p", words12(a)))
    for form in CHAIN_FORMS:
        for j, kind in enumerate(("canon", "s11", "top", "edge")):
            cs.append(Case("chain", kind, _flat([s_elem(rng, kind) for _ in range(18)]), aux=FORMS.index(form)))
    return cs


def spread(groups):
    """One list out of several, each spread evenly over it (every stretch holds its share of
    every group)."""
    keyed = []
    for gi, g in enumerate(groups):
        for i, c in enumerate(g):
            keyed.append(((i + 0.5) / len(g), gi, c))
    keyed.sort(key=lambda t: (t[0], t[1]))
    return [t[2] for t in keyed]


RAGGED = 64 + 37


def build_orders(seed=2800):
    """(interleaved, sorted, ragged): every 64-lane wave of the interleaved file mixes ops and
    case classes; the same cases sorted by op and class (uniform waves); and 101 of them in
    interleaved order, the first case of every op and chain form among them (the last wave
    holds 37 lanes)."""
    cs = build_primitives(seed) + build_composites(seed + 1)
    by_op = {}
    for c in cs:
        by_op.setdefault(c.op, {}).setdefault(c.cls, []).append(c)
    inter = spread([spread(list(by_cls.values())) for _, by_cls in sorted(by_op.items(), key=lambda t: OPS[t[0]])])
    srt = sorted(inter, key=lambda c: (OPS[c.op], c.aux, c.cls, c.id))
    pick, seen = set(), set()
    for c in inter:
        if (c.op, c.aux) not in seen:
            seen.add((c.op, c.aux))
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
    """An OUT file that passes: the exact words, and for the composites the canonical
    representative of every residue."""
    out = []
    for c in cases:
        out.append(c.exact if c.exact is not None else pack_words(_flat(limbs_of(r) for r in c.res)))
    return b"".join(out)


# ---------------------------------------------------------------- comparator
class Report:
    def __init__(self):
        self.compared = {}   # op -> cases compared
        self.mismatch = {}   # (op, class) -> [(case id, what)]
        self.words = {}      # case id -> result bytes

    @property
    def ok(self):
        return not self.mismatch

    def total(self):
        return sum(self.compared.values())

    def ops_failed(self):
        return sorted({op for op, _ in self.mismatch})

    def text(self):
        if not self.mismatch:
            return "compared %d cases, no mismatch" % self.total()
        return "compared %d cases; mismatches: %s" % (self.total(), "; ".join(
            "%s[%s]: %d (first: id %d, %s)" % (op, cls, len(v), v[0][0], v[0][1])
            for (op, cls), v in sorted(self.mismatch.items())))


def check_case(c, got):
    """None, or what is wrong with the case's result bytes."""
    if c.exact is not None:
        if got == c.exact:
            return None
        w = struct.unpack("<%dI" % (len(got) // 4), got)
        e = struct.unpack("<%dI" % (len(got) // 4), c.exact)
        bad = [i for i in range(len(w)) if w[i] != e[i]]
        return "%d words differ, first word %d: %#x, expected %#x" % (len(bad), bad[0], w[bad[0]], e[bad[0]])
    w = struct.unpack("<%dI" % (len(got) // 4), got)
    for k, r in enumerate(c.res):
        l = w[N * k:N * k + N]
        if max(l) > M28:
            return "coefficient %d: a limb >= 2^28" % k
        x = int_of(l)
        if x >= c.bound:
            return "coefficient %d: value %.4f p, bound %.2f p" % (k, x / P, c.bound / P)
        if x % P != r:
            return "coefficient %d: wrong residue" % k
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
    """Cases built on the same operands (the aliasing forms of a product; sqr(a) and mul(a, a))
    whose result words differ: [(group, {op: bytes})]."""
    by = {}
    for c in cases:
        if c.group is not None and c.id in rep.words:
            by.setdefault(c.group, []).append(c)
    bad = []
    for g, cs in by.items():
        if len({rep.words[c.id] for c in cs}) > 1:
            bad.append((g, sorted(c.op for c in cs)))
    return by, bad


def peaks(cases):
    """{function: {accumulator: (peak, class of the case that reached it)}} and the columns where
    fe2_mul3k's signed accumulator was negative, over the primitive cases."""
    pk, neg = {}, set()
    for c in cases:
        fn = FUNC_OF[c.op]
        if fn not in PRIMITIVES:
            continue
        _, p, ng = model(c)
        neg.update(ng)
        for name, v in p.items():
            if v > pk.setdefault(fn, {}).get(name, (0, ""))[0]:
                pk[fn][name] = (v, c.cls)
    return pk, sorted(neg)


def main(argv):
    """field28_vectors.py write DIR: the three case files; check ORDER OUT: compare;
    stats: case counts per op and the modeled accumulator peaks."""
    import math
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
            n[c.op] = n.get(c.op, 0) + 1
        print("%d cases: %s" % (len(inter), ", ".join("%s %d" % (op, n[op]) for op in OP_LIST)))
        pk, neg = peaks(inter)
        for fn in PRIMITIVES:
            print(fn, ", ".join("%s 2^%.2f (%s)" % (k, math.log2(v), cls) for k, (v, cls) in sorted(pk[fn].items())))
        print("fe2_mul3k acc0 negative in columns", neg)
        return 0
    print(main.__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv))
