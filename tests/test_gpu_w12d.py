"""The row-distributed Fp12 engine (grandine_amd/csrc/bls_w12d.h) bit by bit on the GPU, and the
verdict / Horner kernels built on it through the public ABI.

* tools/ubench/w12d_check runs every operation of the header on raw limb images written by
  tools/ubench/w12d_vectors.py (random, edge, top-of-contract and redundant-limb operands);
  every output coefficient is checked here against Python integers and oracle/bls12_381.py:
  residue, limb contract, and the value bound the header states.  One launch serves all tests.
* gbls_final_verify_partials_device on crafted partials: SUCCESS exactly when the oracle's
  final exponentiation of the product is 1, for both verdict kernels.
* gbls_multi_verify_partials_device: the partial BYTES of the row form equal the one-wave
  form's times an Fp scalar derived from the event schedule, and the C oracle's up to an Fp2
  factor (ten exactly-zero coefficients), not only in a verdict.
"""
import ctypes
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
import w12d_vectors as V  # noqa: E402

O = V.O


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    """(cases, results) of ONE launch of w12d_check over every case."""
    exe = os.path.join(ROOT, "tools", "ubench", "_bin", "w12d_check")
    if not os.path.exists(exe):
        raise AssertionError("%s not built (make -C tools/ubench)" % exe)
    d = tmp_path_factory.mktemp("w12d")
    cases = V.build_cases()
    src, dst = str(d / "cases.bin"), str(d / "results.bin")
    V.write_cases(src, cases)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=90)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return cases, V.read_results(dst, cases)


def _check(checked, want_counts):
    cases, results = checked
    counts, errs = V.check_all(cases, results, ops=set(want_counts))
    assert counts == want_counts  # no case skipped or filtered
    assert not errs, "%d errors, first:\n%s" % (len(errs), "\n".join(errs[:12]))


def test_w12d_mul_and_sqr(checked):
    """mul (c distinct, c aliasing a, c aliasing b, a == b) and sqr (c distinct, c aliasing a):
    80 operands each -- 48 random canonical, 12 edge patterns of 0 / 1 / p - 1, the elements 0,
    1, an Fp scalar, an Fp6 element, 16 top-of-contract images (x + 127 p with limbs at
    2^28 + 2^9 - 1; one with all twelve coefficients at the top, presums of 8 just under
    1024 p).  Outputs < 128 p."""
    _check(checked, {"mul": 80, "mul_ca": 80, "mul_cb": 80, "mul_aa": 80, "sqr": 80, "sqr_ca": 80})


def test_w12d_conj_frobenius_load_store(checked):
    """conj (outputs <= 128 p: the bias minus a zero coefficient is 128 p exactly), frob
    (< p + 2^337), frob2 (< p + 2^336), and load_scaled + store_words with the exact 2^-64."""
    _check(checked, {"conj": 80, "frob": 80, "frob2": 80, "load_scaled": 60})


def test_w12d_cyclotomic(checked):
    """cyc_sqr == f12_sqr (< 40 p) and exp_x_cyc == conj(a^|x|) on oracle-built cyclotomic
    elements f^((p^6-1)(p^2+1)), canonical and with 127 p on every coefficient."""
    _check(checked, {"cyc_sqr": 49, "exp_x_cyc": 49})


def test_w12d_easy_part(checked):
    """c = f^((p^6-1)(p^2+1)), D = F0^2 + F1^2 and its inverse in words[0..24), and the image t
    (easy_part leaves frob2(f^(p^6-1)) there): random, Fp6, F1 = 0, F0 = 0, top-of-contract."""
    _check(checked, {"easy_part": 28})


def test_w12d_inv_wave(checked):
    """out < p and out x = 1 mod p (plain integers), and the batch count of the exact-integer
    iteration (the exit test must see a redundant zero g): edge values, powers of two, 2^60 y
    and 2^90 y (g = 0 mod 2^30 with g != 0: the rare exit-test path), 200 random values; x = 0
    only has to end."""
    _check(checked, {"inv_wave": 237})


def test_w12d_flags(checked):
    """one_flags / zero_flags on 0, p, 2p, 127p, 128p, 1, p + 1, 2^336-sized and one + k p
    representatives: the answer depends on the residue only."""
    _check(checked, {"one_flags": 54, "zero_flags": 40})


def test_w12d_chains(checked):
    """200 self-feeding steps (sqr, mul, frob, conj, frob2; and cyc_sqr, mul from cyclotomic
    seeds), every step's image checked for residue, limb contract and bound."""
    _check(checked, {"chain": 2, "chain_cyc": 2})


# ------------------------------------------------------------------ verdicts through the ABI
@pytest.fixture(scope="module")
def G():
    from grandine_amd import _lib as G
    G.lib()
    return G


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def _f12_add_one(a, i):
    a = [list(c) for c in a]
    a[i // 2][i % 2] = (a[i // 2][i % 2] + 1) % O.P
    return [tuple(c) for c in a]


F12_ZERO = [(0, 0)] * 6


def _accepts(x):
    """blst's PAIRING_FinalVerify on the oracle: final_exp(x) == 1; 0 is rejected."""
    if x == F12_ZERO:
        return False
    return O.f12_is_one(O.final_exp(x))


@pytest.fixture(scope="module")
def pool():
    """16 (element, accepted) pairs; the expectation is the oracle's final exponentiation."""
    rng = random.Random(1210)
    rnd = lambda: V.random_f12(rng)
    fp6 = lambda: [(rng.randrange(O.P), rng.randrange(O.P)) if i % 2 == 0 else (0, 0) for i in range(6)]
    hr = lambda: O.f12_pow(rnd(), O.R)
    scalar = [(rng.randrange(1, O.P), 0)] + [(0, 0)] * 5
    els = [O.f12_one(), scalar, fp6(), hr(), hr(), O.f12_mul(hr(), fp6()), O.f12_mul(hr(), fp6()),
           O.f12_mul(hr(), scalar)]
    els += [rnd(), rnd(), O.f12_mul(hr(), rnd()), O.f12_mul(hr(), rnd()), _f12_add_one(els[3], 0),
            _f12_add_one(els[5], 7), F12_ZERO, _f12_add_one(O.f12_one(), 11)]
    out = [(x, _accepts(x)) for x in els]
    assert [a for _, a in out] == [True] * 8 + [False] * 8  # what the construction intends
    return out


def _run_verdicts(torch_dev, G, parts, errs, nparts, nseg):
    """parts: [part][segment] oracle elements; errs: [part][segment] ints -> verdicts per segment."""
    torch, dev = torch_dev
    L = G.lib()
    raw = b"".join(V.engine_bytes(parts[p][s]) for p in range(nparts) for s in range(nseg))
    d_parts = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    d_errs = torch.tensor([errs[p][s] for p in range(nparts) for s in range(nseg)], dtype=torch.int32, device=dev)
    v = torch.full((nseg,), -1, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.gbls_final_verify_partials_device(d_parts.data_ptr(), d_errs.data_ptr(), nparts, nseg, v.data_ptr(), st)
    assert rc == 0, L.gbls_last_error()
    torch.cuda.synchronize()
    return [int(x) for x in v.cpu()]


def _split(rng, target, nparts):
    """nparts factors whose product is target: random ones, and target over their product."""
    fs = [V.random_f12(rng) for _ in range(nparts - 1)]
    prod = O.f12_one()
    for f in fs:
        prod = O.f12_mul(prod, f)
    last = O.f12_mul(target, O.f12_inv(prod)) if fs else target
    chk = last
    for f in fs:
        chk = O.f12_mul(chk, f)
    assert chk == [tuple(c) for c in target]
    return fs + [last]


@pytest.mark.parametrize("nseg", [5, 70])
def test_verdict_kernels_match_oracle_final_exp(torch_dev, G, pool, nseg):
    """nseg = 5 takes k_final_verdict_d (easy part with an inversion, Granger-Scott squarings,
    == 1), nseg = 70 k_final_verdict (inversion-free, Fp6-image test): both must say SUCCESS
    exactly where the oracle's final exponentiation of the segment's value is 1.  Every launch
    mixes accepting and rejecting segments."""
    order = list(range(16))
    random.Random(1211).shuffle(order)
    launches = [order[i:i + 5] + order[:max(0, i + 5 - 16)] for i in range(0, 16, 5)] if nseg == 5 else \
        [[order[i % 16] for i in range(70)]]
    for idx in launches:
        assert len(idx) == nseg
        got = _run_verdicts(torch_dev, G, [[pool[i][0] for i in idx]], [[0] * nseg], 1, nseg)
        want = [G.SUCCESS if pool[i][1] else G.VERIFY_FAIL for i in idx]
        assert got == want, (idx, got, want)


@pytest.mark.parametrize("nseg", [5, 70])
@pytest.mark.parametrize("nparts", [2, 3])
def test_verdict_of_product_of_parts(torch_dev, G, pool, nseg, nparts):
    """Partials laid out [part][segment] with f_1 (f_2) random and the last part target over
    their product: only the product decides, and a transposed index is seen because every
    segment has its own factors and its own expectation.  One accepting segment gets a
    non-zero seg_err in one part: that segment alone turns to VERIFY_FAIL."""
    rng = random.Random(1212 + 10 * nseg + nparts)
    idx = [rng.randrange(16) for _ in range(nseg)]
    idx[:6] = [0, 8, 3, 14, 5, 10][:min(6, nseg)]
    cols = [_split(rng, pool[i][0], nparts) for i in idx]
    parts = [[cols[s][p] for s in range(nseg)] for p in range(nparts)]
    errs = [[0] * nseg for _ in range(nparts)]
    want = [G.SUCCESS if pool[i][1] else G.VERIFY_FAIL for i in idx]
    assert _run_verdicts(torch_dev, G, parts, errs, nparts, nseg) == want
    flagged = 2  # pool[3]: accepted
    assert want[flagged] == G.SUCCESS
    errs[nparts - 1][flagged] = 7
    want[flagged] = G.VERIFY_FAIL
    assert _run_verdicts(torch_dev, G, parts, errs, nparts, nseg) == want


# ------------------------------------------------------------------ partial bytes
def _in_fp2(x):
    """x (oracle form) lies in Fp2: the coefficients of w^1..w^5 are exactly zero."""
    return all(c == (0, 0) for c in x[1:])


def _partials(torch_dev, G, msgs, sigs, pks, rands, offsets):
    torch, dev = torch_dev
    L = G.lib()
    nseg = len(offsets) - 1
    n = offsets[-1]
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    m, s, p = up(msgs[:32 * n]), up(sigs[:192 * n]), up(pks[:96 * n])
    r = torch.tensor([x - (1 << 64) if x >= 1 << 63 else x for x in rands[:n]], dtype=torch.int64, device=dev)
    parts = torch.zeros(nseg * 576, dtype=torch.uint8, device=dev)
    errs = torch.full((nseg,), -1, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.gbls_multi_verify_partials_device(m.data_ptr(), s.data_ptr(), p.data_ptr(), r.data_ptr(), n,
                                             G.u32_array(offsets), nseg, parts.data_ptr(), errs.data_ptr(), st)
    assert rc == 0, L.gbls_last_error()
    torch.cuda.synchronize()
    assert [int(x) for x in errs.cpu()] == [0] * nseg
    raw = bytes(parts.cpu().numpy())
    return [V.f12_from_engine_bytes(raw[576 * i:576 * i + 576]) for i in range(nseg)]


def _row_form_scale():
    """The Fp scalar of the row form against the one-wave form.  The Miller loop's 68 events
    (for each bit of |x| below the top one a doubling, then an addition if the bit is set) are
    combined as f = prod_k V_k^(2^(D_k)), D_k = doublings after event k.  The row form reads
    every event value and each of its 4 part values as repacked limbs, 2^-64 times the value
    (dfp::from_words_scaled); its other steps are exact.  So it returns f times
    2^(-64 (4 + sum_k 2^(D_k)))."""
    ev = []
    for i in range(62, -1, -1):
        ev.append(True)
        if (O.X_ABS >> i) & 1:
            ev.append(False)
    assert len(ev) == 68
    e = 4 + sum(1 << sum(ev[k + 1:]) for k in range(68))
    return pow(pow(1 << 64, -1, O.P), e, O.P)


def test_partial_bytes_row_form_vs_one_wave_form(torch_dev, G):
    """The same 3 segments x 2 sets as a 3-segment call (row form: k_ml_horner_d +
    k_ml_combine_d) and as segments 0..2 of a 70-segment call (one-wave form: k_ml_horner).

    Both calls are far below the line kernels' regime threshold (kW4Max = 1024 points), so both
    feed their Horner kernels the same event values V_k: the two partials differ only by the Fp*
    scalars of load_scaled / from_words_scaled.  Hence a b^-1 lies in Fp -- eleven of its twelve
    coefficients are exactly zero -- and it is the scalar _row_form_scale() derives from the
    event schedule, the same for every segment.  A one-bit verdict can hide an error here;
    eleven zero coefficients and an exact scalar cannot."""
    from grandine_amd import factory as F
    msgs, sigs, pks, rands = F.c2_batch(140, seed=1213)
    row = _partials(torch_dev, G, msgs, sigs, pks, rands, [0, 2, 4, 6])
    wave = _partials(torch_dev, G, msgs, sigs, pks, rands, list(range(0, 141, 2)))
    assert len(row) == 3 and len(wave) == 70
    want = [(_row_form_scale(), 0)] + [(0, 0)] * 5
    for s in range(3):
        assert O.f12_mul(row[s], O.f12_inv(wave[s])) == want, s
    # and the segments are not each other's: a transposed index would pass a per-call check
    assert not _in_fp2(O.f12_mul(row[0], O.f12_inv(wave[1])))


def test_partial_bytes_vs_c_oracle(torch_dev, G):
    """One segment of 32 sets against ref_multi_verify_partial of the C oracle (oracle/bls_ref.c).
    Both run the Miller loop over the same pairs (P_i, Q_i), but the oracle's lines are affine
    and the engine's projective (Jacobian S and H(m), bls_w4.h): a line is defined up to a factor
    of the field of its coefficients, Fp2, and the points' coordinates up to Fp.  So the ratio
    lies in Fp2 -- the ten coefficients of w^1..w^5 are exactly zero -- and nothing smaller is
    justified."""
    from grandine_amd import factory as F
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
    C = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libbls_ref.so"))
    C.ref_multi_verify_partial.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                           ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_char_p]
    n = 32
    msgs, sigs, pks, rands = F.c2_batch(n, seed=1214)
    cpart = ctypes.create_string_buffer(576)
    assert C.ref_multi_verify_partial(msgs, sigs, pks, (ctypes.c_uint64 * n)(*rands), n, cpart) == 0
    gpu = _partials(torch_dev, G, msgs, sigs, pks, rands, [0, n])[0]
    ratio = O.f12_mul(gpu, O.f12_inv(V.f12_from_engine_bytes(cpart.raw)))
    assert ratio[0] != (0, 0) and _in_fp2(ratio), ratio
