"""The c = 5 bucket MSM's window sums on the wave engine (k_msm_windows_w4,
grandine_amd/csrc/k_msm_w4.hip): S(s, w) = sum_b (b + 1) X(s, w, b), 13 Miller pairs per segment.

tests/gpu_msm_windows.py runs as fresh children (their own engines), once per set of cases, and
every case below reads its per-segment verdicts: gbls_multi_verify_segments against the C
oracle's ref_multi_verify of the same segment, as planned and with one message of every nonempty
segment corrupted.  A submission takes the MSM only when every segment holds GBLS_MSM_MIN sets,
so the cases with an empty segment run with GBLS_MSM_MIN=0 and the others with 1, and every call
is checked to have run the MSM stage once and the per-set signature sum never (the engine's
stage timers).  The shapes are the smallest at which the kernel can go wrong:

* grid: 207 one-set segments, r = (b + 1) 2^(5 w) for every window and bucket that fits 64 bits
  -- exactly one bucket of one window populated, so a wrong weight, window constant or index is
  a wrong verdict of that segment alone; once more with GBLS_MSM_R28=0 (engine-form partials);
* signed: r = 17 * 2^(5 w) (digit -15 and a carry), 2^64 - 1 (every digit -1, top digit 16),
  2^63, 1;
* full: all 16 buckets of window 0 in one segment, buckets 0..14 of window 12 in another;
* special: the addition's special cases inside the fold -- two equal points, a bucket sum that
  is infinity beside a third set, a segment whose S is infinity altogether;
* runs: 40 sets in one bucket (K = 4: 10 chunks, two runs) and 300 random 64-bit scalars;
* an infinite signature and a zero scalar (the engine's flag: VERIFY_FAIL) on offsets
  [0, 1, 18, 58, 358], and again on [0, 1, 1, 18, 58, 358];
* segments: offsets [0, 1, 1, 18, 58, 358] -- an empty segment under both conventions (an error
  through gbls_multi_verify_segments, the identity through the Miller partials);
* 80 segments: 1040 windows, more than k_lines_w4j takes, so the sums are stored affine.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TAIL = ["infinite signature", "zero scalar"]
SETS = {
    "main": ["grid", "signed", "full", "special", "runs"] + TAIL + ["80 segments"],
    "empty": ["segments", "segments / partials"] + TAIL,
    "engine": ["grid"],
}
CASES = [(k, c) for k, v in SETS.items() for c in v]
_children = {}


def _child(which):
    """The child's rows.  After a child that failed (a fault, an abort, a time limit) no further child
    is started on the GPU: the remaining sets fail without running."""
    failed = [k for k, v in _children.items() if isinstance(v, str)]
    if which not in _children:
        assert not failed, "not started: the child of set %r failed before" % failed[0]
        _children[which] = "failed"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_msm_windows.py"), "--set", which],
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        res = json.loads(out.stdout.strip().splitlines()[-1])
        assert res["set"] == which
        _children[which] = {c["name"]: c for c in res["cases"]}
    assert not isinstance(_children[which], str), "the child of set %r failed" % which
    return _children[which]


def _twin(name):
    base, _, tail = name.partition(" / ")
    return base + " / twin" + (" / " + tail if tail else "")


@pytest.mark.parametrize("which,name", CASES)
def test_window_sums_match_oracle(which, name):
    row = _child(which)[name]
    print(which, name, "ref", row["ref"], "gpu", row["gpu"], "stages", row["stages"])
    assert row["stages"] == [1, 0], "the call did not take the bucket MSM"
    assert row["gpu"] == row["ref"], name
    assert 0 in row["ref"], name  # the plan has something to accept


@pytest.mark.parametrize("which,name", CASES)
def test_corrupted_twin_fails(which, name):
    row = _child(which)[_twin(name)]
    print(which, name, "ref", row["ref"], "gpu", row["gpu"], "stages", row["stages"])
    assert row["stages"] == [1, 0], "the call did not take the bucket MSM"
    assert row["gpu"] == row["ref"], name
    # every segment fails; through the Miller partials the empty one (segment 1) is the identity
    want = [5] * len(row["ref"])
    if name.endswith("partials"):
        want[1] = 0
    assert row["ref"] == want, name


@pytest.mark.parametrize("which", sorted(SETS))
def test_plan_is_complete(which):
    assert sorted(_child(which)) == sorted(SETS[which] + [_twin(c) for c in SETS[which]])
