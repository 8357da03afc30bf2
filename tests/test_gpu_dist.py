"""The N-rank flow as fresh child processes: torch.distributed.run with 2
ranks on the one GPU of the box (gloo, GBLS_BENCH_ONE_DEVICE), each started before it touches
the GPU.  (1) tests/dist_flow.py: per-rank GPU partials, all-gather, final exponentiation on
every rank; clean batch accepted, a corrupted shard rejected by every rank.  (2) bench.py's
own 2-rank C2 leg (2 batches of 4096 sets per rank, all verdicts checked by the bench)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(args, timeout):
    env = dict(os.environ, GBLS_BENCH_ONE_DEVICE="1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", "--master-port=%d" % _port()] + args
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


def test_two_rank_partials_flow_rejects_corrupt_shard():
    r = _run([os.path.join(ROOT, "tests", "dist_flow.py")], 300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
    res = json.loads(line)
    assert res["world"] == 2
    for x in res["ranks"]:
        assert x["clean"] == 0 and x["corrupt"] == 5, res


def test_bench_two_rank_c2_leg():
    r = _run([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu",
              "--batches", "2"], 400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0, line


def test_bench_two_rank_c4_epoch_strong_scaling():
    """VERDICT r03 "next 6": C4 as BASELINE.json configs[3] names it -- ONE mainnet epoch (2048
    committees over a 2^20-key registry) split into whole committees per rank (1024 each), the
    ranks' Miller partials all-gathered into one final exponentiation, strong scaling; the bench
    then checks every committee's own verdict on its rank and sums them over the ranks."""
    args = [os.path.join(ROOT, "bench.py"), "--config", "C4", "--full", "--gpus", "2", "--steps", "2", "--warmup", "1",
            "--no-cpu"]
    r = _run(args, 600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0, line
    assert line["epoch"]["committees"] == 2048 and line["epoch"]["keys"] == (1 << 20) - 576, line
    assert line["epoch"]["per_committee_check"] == {"committees_verified": 2048, "committees": 2048}, line
    assert line["config"]["units_per_gpu_per_step"] == 1024, line
