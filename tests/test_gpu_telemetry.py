"""Engine telemetry on the GPU (include/grandine_bls_gpu_telemetry.h).

The level is process-wide and sticky, so every case runs tests/gpu_telemetry_child.py in a fresh
process; the children that share a call sequence run once per level and are shared by the tests.
The environment is the 600-key registry and the committee table of tests/test_gpu_spans.py (its
constants are imported, as tests/test_gpu_fold.py imports them; the children load the same shapes
through tests/gpu_each_child.py).

Counts are exact: they follow from the calls made, never from what the engine reports.  The phase
inequalities are exact too: every phase is a difference of steady-clock readings nested inside the
next one (total >= hold + window + queue + run, run >= enqueue + sync, enqueue >= staging).

Neither a wait for a staging slot nor a wait for a context lease can be provoked deterministically
on the GPU (both need the device to lag behind the host by four calls of one context, or 64 calls in
flight).  Both are measured by host-only hooks (tel::timed_acquire, tel::timed_wait in
gbls_telemetry.h) that tests/native/telemetry_main.cpp drives with a pool of stub contexts and a stub
wait, beside the scheduler's phases; nothing here loops until one happens."""
import json
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_spans as S  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = S.ROOT
CALLER = ["hold", "window", "queue", "run", "total"]
SHARD = ["reglock", "lease", "staging", "growth", "enqueue", "sync", "device", "lag"]
# the sequence of the child, in order: (class, kind, sets)
CALLS = [("normal", "batch", 3)] * 4 + [("normal", "checks", 5)] * 2 + [("block", "batch", 1), ("normal", "span_checks", 3),
                                                                       ("normal", "direct", 2)]


def child(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_telemetry_child.py")] + [str(a) for a in args],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def runs():
    return {level: child("sequence", level) for level in (0, 1, 2)}


def expected_cells():
    want = {}
    for cls, kind, sets in CALLS:
        c = want.setdefault("%s/%s" % (cls, kind), {"calls": 0, "sets": 0, "rejected": 0})
        c["calls"] += 1
        c["sets"] += sets
    want["normal/checks"]["rejected"] = 1
    return want


def test_off_by_default(runs):
    off = runs[0]
    assert off["cells"] == {} and off["trace"] == [] and off["dropped"] == 0
    assert off["rejected"] == [5, 102]
    # 4 good batches, check 2 of 5 fails twice, the block verifies, the spans pass, both keys decode
    v = off["verdicts"]
    assert v[:4] == [0, 0, 0, 0] and v[4] == v[5] == [0, [0] * 5, [0, 0, 5, 0, 0]]
    assert v[6] == 0 and v[7] == [0, [0, 0, 0]] and v[8] == [0, [0, 0], True]
    for level in (1, 2):
        assert runs[level]["verdicts"] == v and runs[level]["rejected"] == off["rejected"]


def check_counts(cells, level):
    want = expected_cells()
    assert sorted(cells) == sorted(want)
    for name, w in want.items():
        c = cells[name]
        assert (c["calls"], c["sets"], c["rejected"], c["engine_errors"]) == (w["calls"], w["sets"], w["rejected"], 0), name
        assert c["submissions"] == c["calls"] == c["callers"] and c["submitted_sets"] == c["sets"], name
        assert c["shards"] == c["calls"], name            # nothing here is large enough to be sharded
        assert c["callers_bin"][0] == c["submissions"] and sum(c["callers_bin"]) == c["submissions"], name
        assert sum(c["sets_bin"]) == c["submissions"], name
        ph = c["phases"]
        for p in CALLER:
            assert ph[p]["count"] == c["calls"], (name, p)
        for p in SHARD:
            assert ph[p]["count"] == c["shards"], (name, p)
        for p, h in ph.items():
            assert sum(h["buckets"]) == h["count"], (name, p)
            assert h["max_ns"] <= h["sum_ns"], (name, p)
        s = {p: ph[p]["sum_ns"] for p in ph}
        assert s["total"] >= s["hold"] + s["window"] + s["queue"] + s["run"], name
        assert s["run"] >= s["enqueue"] + s["sync"], name
        assert s["enqueue"] >= s["staging"], name
        assert s["total"] > 0 and s["run"] > 0 and s["enqueue"] > 0 and s["sync"] > 0, name
        if level == 1:
            assert s["device"] == 0 and s["lag"] == 0, name
        else:
            assert s["device"] > 0, name
    assert cells["normal/batch"]["sets_bin"][2] == 4      # 3 sets: the bin of 3..4
    assert cells["normal/direct"]["sets_bin"][1] == 1     # 2 sets
    assert cells["block/batch"]["sets_bin"][0] == 1       # 1 set


def test_exact_counts_at_level_1(runs):
    check_counts(runs[1]["cells"], 1)


def check_trace(trace, level):
    assert len(trace) == len(CALLS)                       # one record per shard
    assert [(r["cls"], r["kind"], r["sets"]) for r in trace] == CALLS
    for a, b in zip(trace, trace[1:]):
        assert b["id"] == a["id"] + 1 and b["submission"] >= a["submission"]
    for r in trace:
        assert r["first_arrival_ns"] <= r["lead_ns"] <= r["lease_ns"] <= r["enqueued_ns"] <= r["synced_ns"], r
        assert r["callers"] == 1 and r["shard_sets"] == r["sets"] and r["engine"] == 0 and r["context"] != 0
        if level == 1:
            assert r["device_ns"] == 0 and r["lag_ns"] == 0 and r["first_event_ns"] == 0
        else:
            assert r["lease_ns"] <= r["first_event_ns"] <= r["enqueued_ns"]
            assert 0 < r["device_ns"] <= r["synced_ns"] - r["first_event_ns"], r
            assert r["lag_ns"] == r["synced_ns"] - r["first_event_ns"] - r["device_ns"], r


def test_trace_at_level_1(runs):
    check_trace(runs[1]["trace"], 1)
    assert runs[1]["dropped"] == 0


def test_trace_and_device_time_at_level_2(runs):
    two = runs[2]
    check_counts(two["cells"], 2)
    check_trace(two["trace"], 2)
    flood = two["flood"]
    # 1030 more shards: the ring keeps the 1024 most recent, in order, and counts the rest
    assert flood["n"] == 1024 and flood["dropped"] == 6 and flood["consecutive"] and flood["kinds"] == ["direct"]
    assert flood["ids"][1] == two["trace"][-1]["id"] + 1030
    assert flood["ids"] == [flood["written"] - 1024, flood["written"] - 1]
    assert flood["snapshot_dropped"] == 6


def test_conservation_under_merging():
    """160 callers in, 160 callers out, however they were merged.  (Whether they were merged depends
    on timing and is not asserted.)"""
    for mode in ("merge", "nomerge"):
        res = child(mode)
        assert res["good"] == [20] * 8
        assert list(res["cells"]) == ["normal/batch"]
        c = res["cells"]["normal/batch"]
        assert (c["calls"], c["sets"], c["rejected"], c["engine_errors"]) == (160, 480, 0, 0)
        assert c["callers"] == 160 and c["submitted_sets"] == 480 and c["submissions"] <= 160
        assert c["shards"] == c["submissions"] == sum(c["callers_bin"]) == sum(c["sets_bin"])
        for p in CALLER:
            assert c["phases"][p]["count"] == 160
        s = {p: h["sum_ns"] for p, h in c["phases"].items()}
        assert s["total"] >= s["hold"] + s["window"] + s["queue"] + s["run"]
        if mode == "nomerge":
            assert c["submissions"] == 160 and c["callers_bin"][0] == 160
            assert s["window"] == 0 and s["hold"] == 0


def test_memory_gauges():
    res = child("memory")
    assert res["before_init"] == [] and res["before_init_zero"]
    txt = open(os.path.join(ROOT, "grandine_amd", "csrc", "gbls_msgcache.h")).read()
    a, b = re.search(r"constexpr size_t kSlotWords = (\d+) \* (\d+);", txt).groups()
    slot_bytes = int(a) * int(b) * 4
    for stage in ("registry", "configured", "served", "unconfigured", "larger"):
        assert len(res[stage]) == 1
        m = res[stage][0]
        assert m["registry_bytes"] >= S.NREG * 96
        assert m["pinned_live_bytes"] >= 1 << 20          # a context has uploaded: the smallest staging slot
        held = (sum(m["workspace_bytes"].values()) + m["registry_bytes"] + m["committee_bytes"] + m["member_bytes"] +
                m["linecache_bytes"])
        assert held + m["device_free_bytes"] <= m["device_total_bytes"] and m["device_total_bytes"] > 0
        assert sum(m["contexts_idle"].values()) >= 2 and sum(m["contexts_leased"].values()) == 0
    line = [res[s][0]["linecache_bytes"] for s in ("registry", "configured", "served", "unconfigured", "larger")]
    assert line == [0, 0, (256 + 64) * slot_bytes, 0, 0]   # allocated by the first served call: 256 slots and the spare quarter
    ws = [sum(res[s][0]["workspace_bytes"].values()) for s in ("registry", "served", "unconfigured", "larger")]
    assert ws[0] > 0 and ws[0] <= ws[1] <= ws[2] <= ws[3]


def test_device_kind_records_its_enqueue_only():
    res = child("device", 1)
    assert (res["rc"], res["verdict"]) == (0, 0) and res["corrupted"] == [0, 5]
    assert list(res["cells"]) == ["normal/device"]
    c = res["cells"]["normal/device"]
    assert (c["calls"], c["sets"], c["submissions"], c["shards"]) == (1, 3, 1, 1)
    ph = c["phases"]
    assert ph["enqueue"]["count"] == 1 and ph["enqueue"]["sum_ns"] > 0
    assert ph["sync"]["count"] == 0 and ph["device"]["count"] == 0 and ph["lag"]["count"] == 0
    assert ph["total"]["count"] == 1
    (r,) = res["trace"]
    assert r["kind"] == "device" and r["synced_ns"] == r["enqueued_ns"] and r["device_ns"] == 0


def test_two_engines_share_a_submission_id():
    res = child("replicas")
    assert res["engines"] == 2 and res["rc"] == [0, 0, 0]
    c = res["cells"]["normal/span_checks"]
    assert (c["calls"], c["sets"], c["submissions"], c["shards"], c["callers"]) == (1, 2100, 1, 2, 1)
    assert len(res["trace"]) == 2
    a, b = res["trace"]
    assert a["submission"] == b["submission"] and {a["engine"], b["engine"]} == {0, 1}
    assert a["shard_sets"] + b["shard_sets"] == 2100 and a["sets"] == b["sets"] == 2100
    assert len(res["memory"]) == 2
    s = {p: h["sum_ns"] for p, h in c["phases"].items()}
    assert s["run"] >= s["enqueue"] + s["sync"]
