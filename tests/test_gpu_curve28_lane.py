"""The radix-2^28 lane kernels themselves (k_h2c_clear_lane_a28 / _b28, the staged
k_h2c_clear_pre28 / k_h2c_chain28 / _mid28 / _post28, k_lines_lane28, k_mv_g1mul_lane28, the MSM's
k_msm_chunk28 / k_msm_fold28) through the public ABI at the smallest shape that reaches them: 1100
sets in one segment (tests/edges_cases.py PAD_TO: above kW4Max = 1024, 17 full waves and 12 lanes)
under GBLS_LANE_MIN=1025, in BYTES and not only in a verdict.  Each engine configuration runs in a
fresh child process (tests/gpu_curve28_child.py)."""
import ctypes
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import edges_cases as E  # noqa: E402
import gpu_curve28_child as CH  # noqa: E402
import w12d_vectors as W12  # noqa: E402
from oracle import bls12_381 as O  # noqa: E402

LANE = "GBLS_LANE_MIN=1025"


def child(d, tag, *args):
    """One fresh engine process: {task: bytes} and its JSON line."""
    files = {t: str(d / ("%s_%s.bin" % (tag, t))) for t in args if not t.startswith("GBLS_")}
    argv = [a if a.startswith("GBLS_") else "%s=%s" % (a, files[a]) for a in args]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_curve28_child.py")] + argv,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    return {t: open(p, "rb").read() for t, p in files.items()}, res


@pytest.fixture(scope="module")
def C():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libbls_ref.so"))
    lib.ref_multi_verify_partial.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_char_p]
    lib.ref_hash_to_g2.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def lane(tmp_path_factory):
    """{configuration: ({task: bytes}, JSON)}: the lane regime with the one-kernel and the staged
    clearing, and with the engine-form lane kernels."""
    d = tmp_path_factory.mktemp("curve28_lane")
    return {"staged0": child(d, "s0", LANE, "GBLS_CLEAR_STAGED=0", "h2c", "partial"),
            "staged1": child(d, "s1", LANE, "GBLS_CLEAR_STAGED=1", "h2c", "partial"),
            "r28off": child(d, "e", LANE, "GBLS_LANE_R28=0", "partial")}


def _in_fp2(x):
    return all(c == (0, 0) for c in x[1:])


def _ratio(a, b):
    return O.f12_mul(W12.f12_from_engine_bytes(a), O.f12_inv(W12.f12_from_engine_bytes(b)))


def test_lane_hash_bytes_equal_the_oracle_s_in_both_clearing_forms(lane, C):
    """gbls_hash_to_g2 of the 1100 messages through k_h2c_clear_lane_a28 / _b28 and through the
    staged pre / chain / mid / chain / post kernels: every byte the C oracle's."""
    msgs = E.padded_messages()
    assert len(msgs) == E.PAD_TO == CH.N_SETS == 1100 and 1100 == 17 * 64 + 12

    def one(m):
        out = ctypes.create_string_buffer(192)
        C.ref_hash_to_g2(m, len(m), O.DST_POP, len(O.DST_POP), out)
        return out.raw

    with ThreadPoolExecutor(8) as ex:  # ctypes releases the GIL
        want = list(ex.map(one, msgs))
    for cfg in ("staged0", "staged1"):
        files, res = lane[cfg]
        raw = files["h2c"]
        assert res["h2c"] == 1100 and len(raw) == 192 * 1100
        bad = [i for i in range(1100) if raw[192 * i:192 * i + 192] != want[i]]
        assert not bad, (cfg, bad[:8])
        # gbls_hash_to_g2 launches its three kernels outside the stage timers (h2c_affine), so it
        # reports no stage; launch_h2c_clear picks the form from the launch size and the knobs alone,
        # and the same child's 1100-set partial, which does report, went through the clearing stage
        assert not any(res["stages"]["h2c"].values()), res["stages"]["h2c"]
        assert res["stages"]["partial"]["k_h2c_clear"] >= 1 and res["knobs"][:2] == [LANE, "GBLS_CLEAR_STAGED=%s" % cfg[-1]]


def test_lane_partial_bytes_vs_c_oracle(lane, C):
    """One segment of 1100 sets against ref_multi_verify_partial of the C oracle, under
    GBLS_CLEAR_STAGED=0 and =1.  Both sides run the Miller loop over the same pairs; the oracle's
    lines are affine and the engine's projective, so the ratio lies in Fp2: the ten coefficients
    of w^1 ... w^5 are exactly zero (the argument of test_partial_bytes_vs_c_oracle).  The path:
    per-set r pk (k_mv_g1mul), no bucket MSM, the clearing, line and Miller stages."""
    from grandine_amd import factory as F
    n = CH.N_SETS
    msgs, sigs, pks, rands = F.c2_batch(n, seed=CH.SEED)
    cpart = ctypes.create_string_buffer(576)
    assert C.ref_multi_verify_partial(msgs, sigs, pks, (ctypes.c_uint64 * n)(*rands), n, cpart) == 0
    for cfg in ("staged0", "staged1", "r28off"):
        files, res = lane[cfg]
        assert res["partial_err"] == [0] and len(files["partial"]) == 576
        ratio = _ratio(files["partial"], cpart.raw)
        assert ratio[0] != (0, 0) and _in_fp2(ratio), (cfg, ratio)
        st = res["stages"]["partial"]
        assert st["k_mv_g1mul"] >= 1 and st["k_msm"] == 0 and st["k_h2c_clear"] >= 1 and st["k_lines"] >= 1 and \
            st["k_ml_group"] >= 1, (cfg, st)
    # the staged and the one-kernel clearing hand the same affine points on: the same bytes
    assert lane["staged0"][0]["partial"] == lane["staged1"][0]["partial"]


def _lane_form_scale(npairs):
    """The Fp scalar of the default lane form against the GBLS_LANE_R28=0 lane form.  Both run the
    same line formulas on the same points; k_lines_lane28 stores every coefficient as its repacked
    limbs (store12: no conversion product), which the engine-form reader sees as the coefficient
    times 2^8 -- the three coefficients of a line alike, so the line's value times 2^8.  The Miller
    loop combines the 68 event values as f = prod_k V_k^(2^(D_k)), D_k = doublings after event k,
    and V_k is the product over the npairs message pairs (the signature pair's lines come from
    another kernel in both runs).  So the default form returns f times 2^(8 npairs sum_k 2^(D_k))."""
    ev = []
    for i in range(62, -1, -1):
        ev.append(True)
        if (O.X_ABS >> i) & 1:
            ev.append(False)
    assert len(ev) == 68
    e = sum(1 << sum(ev[k + 1:]) for k in range(68))
    return pow(2, 8 * npairs * e, O.P)


def test_lane_form_vs_engine_form_lane_kernels(lane):
    """The default lane form against the GBLS_LANE_R28=0 lane form of the same 1100 sets: the
    ratio lies in Fp -- eleven coefficients exactly zero -- and is the scalar _lane_form_scale()
    derives from the code."""
    ratio = _ratio(lane["staged0"][0]["partial"], lane["r28off"][0]["partial"])
    print("ratio c0:", ratio[0])
    assert ratio[1:] == [(0, 0)] * 5 and ratio[0][1] == 0, ratio
    assert ratio[0] == (_lane_form_scale(CH.N_SETS), 0)


def test_msm_special_segment_radix28_vs_engine_form(tmp_path):
    """The "special" case of tests/gpu_msm_windows.py under GBLS_MSM_MIN=1 (equal points and a
    cancelling pair in one bucket: the doubling and the infinity branch of the bucket additions),
    once with the radix-2^28 chunks and folds (GBLS_MSM_R28=1) and once in engine form (=0): the
    two partials' ratio lies in Fp for every segment, and both runs took the MSM."""
    a, ra = child(tmp_path, "m1", "GBLS_MSM_MIN=1", "GBLS_MSM_R28=1", "special")
    b, rb = child(tmp_path, "m0", "GBLS_MSM_MIN=1", "GBLS_MSM_R28=0", "special")
    for res in (ra, rb):
        # the bucket MSM replaces the per-set signature sum (test_gpu_msm_windows.py: stages [1, 0])
        assert res["special_err"] == [0, 0, 0] and res["stages"]["special"]["k_msm"] == 1 and \
            res["stages"]["special"]["k_g2sum"] == 0, res
    assert len(a["special"]) == len(b["special"]) == 3 * 576
    for s in range(3):
        ratio = _ratio(a["special"][576 * s:576 * s + 576], b["special"][576 * s:576 * s + 576])
        print("segment", s, "ratio c0:", ratio[0])
        assert ratio[0] != (0, 0) and ratio[1:] == [(0, 0)] * 5 and ratio[0][1] == 0, (s, ratio)
