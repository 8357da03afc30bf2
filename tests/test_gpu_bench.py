"""bench.py's command line: a plain run carries the headline figure only and --dump-outputs
writes the last timed step's verdicts; --full adds the legs that take runs of their own.
Small shapes (2 batches of 256 sets) in fresh child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batches", "2", "--sets", "256"]


def _bench(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SHAPE + extra, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


def test_plain_run_is_lean_and_dumps_the_last_steps_verdicts(tmp_path):
    out = tmp_path / "dump"
    line = _bench(["--dump-outputs", str(out)])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0, line
    assert line["unit"] == "sets/s" and line["higher_is_better"] is True, line
    # value and ms_per_step describe the same 3 timed steps of 2 x 256 sets
    assert abs(line["value"] - 512 / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"], line
    assert line["roofline"] is None and line["cpu_baseline"] is None and "single_batch" not in line, line
    assert sorted(os.listdir(out)) == ["verdicts.npy"]
    v = np.load(out / "verdicts.npy")
    # one row per batch: verified, status GBLS_SUCCESS
    assert v.dtype == np.float64 and v.tolist() == [[1.0, 0.0], [1.0, 0.0]], v


def test_full_run_adds_the_other_legs():
    line = _bench(["--full", "--no-cpu"])
    assert line["single_batch"]["sets_per_step"] == 256 and line["single_batch"]["value"] > 0, line
    assert line["roofline"]["peak"] > 0 and line["roofline"]["stage_ms_per_step"], line
