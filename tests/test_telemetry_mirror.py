"""CPU: the Python module grandine_amd/telemetry.py with the engine stubbed.

* read(), trace() and memory() turn the library's structs into dicts keyed by the names the library
  itself reports (a stub library fills the structs);
* prometheus_text: per (class, kind) and phase the `_bucket` lines are cumulative and non-decreasing,
  the `le` values are the bucket edges in seconds (2^(k+10) ns), `+Inf` equals `_count`, `_sum` is the
  sum in seconds, and the counters are labelled with class and kind."""
import ctypes
import re

import pytest

from grandine_amd import _lib as G
from grandine_amd import telemetry as T

CLASSES = [b"normal", b"block"]
KINDS = [b"batch", b"checks", b"span_items", b"span_checks", b"local_items", b"local_checks", b"fold", b"direct", b"device"]
PHASES = [b"hold", b"window", b"queue", b"run", b"total", b"reglock", b"lease", b"staging", b"growth", b"enqueue", b"sync",
          b"device", b"lag"]


class StubLibrary:
    """Answers the eight entries the way the library does, from Python values."""

    def __init__(self):
        self.level = 0
        self.records = []
        self.engines = []

    @staticmethod
    def _name(names, i):
        return names[i] if 0 <= i < len(names) else None

    def gbls_telemetry_class_name(self, i):
        return self._name(CLASSES, i)

    def gbls_telemetry_kind_name(self, i):
        return self._name(KINDS, i)

    def gbls_telemetry_phase_name(self, i):
        return self._name(PHASES, i)

    def gbls_telemetry_enable(self, level):
        prev, self.level = self.level, max(0, min(2, level))
        return prev

    def gbls_telemetry_reset(self):
        self.records = []

    def gbls_telemetry_read(self, ref, size):
        snap = ref._obj
        assert size == ctypes.sizeof(G.TelemetrySnapshot)
        snap.size, snap.level, snap.trace_written, snap.trace_dropped = size, self.level, 7, 2
        c = snap.cell[0][0]            # normal/batch
        c.calls, c.sets, c.submissions, c.shards, c.callers, c.submitted_sets = 5, 15, 3, 3, 5, 15
        c.callers_bin[0], c.callers_bin[1] = 2, 1
        for p, values in ((4, [900, 1024, 5000, 5000, 3 << 40]), (3, [100] * 5)):   # total, run
            h = c.phase[p]
            for v in values:
                h.count += 1
                h.sum_ns += v
                h.max_ns = max(h.max_ns, v)
                h.bucket[0 if v < 1024 else min(31, v.bit_length() - 10)] += 1
        d = snap.cell[1][7]            # block/direct: only a rejection
        d.rejected = 1
        return 0

    def gbls_telemetry_trace(self, recs, max_records, dropped):
        n = min(max_records, len(self.records))
        for i in range(n):
            for k, v in self.records[i].items():
                setattr(recs[i], k, v)
        dropped._obj.value = 3
        return n

    def gbls_telemetry_memory(self, ref, size):
        info = ref._obj
        info.size, info.engines = size, len(self.engines)
        for e, vals in enumerate(self.engines):
            info.engine[e].hip_device = vals["hip_device"]
            info.engine[e].registry_bytes = vals["registry_bytes"]
            info.engine[e].workspace_bytes[1] = vals["block_ws"]
        return 0


@pytest.fixture
def stub(monkeypatch):
    lib = StubLibrary()
    monkeypatch.setattr(G, "load_library", lambda: lib)
    return lib


def test_enable_read_trace_memory(stub):
    assert T.enable(1) == 0 and T.enable(9) == 1 and stub.level == 2
    assert T.names() == ([n.decode() for n in CLASSES], [n.decode() for n in KINDS], [n.decode() for n in PHASES])
    snap = T.read()
    assert (snap["level"], snap["trace_written"], snap["trace_dropped"]) == (2, 7, 2)
    assert sorted(snap["cells"]) == ["block", "normal"] and list(snap["cells"]["normal"]) == [n.decode() for n in KINDS]
    c = snap["cells"]["normal"]["batch"]
    assert (c["calls"], c["sets"], c["submissions"], c["callers"]) == (5, 15, 3, 5) and c["callers_bin"][:3] == [2, 1, 0]
    assert list(c["phases"]) == [n.decode() for n in PHASES]
    assert c["phases"]["total"]["count"] == 5 and c["phases"]["total"]["max_ns"] == 3 << 40
    assert c["phases"]["total"]["buckets"][0] == 1 and c["phases"]["total"]["buckets"][1] == 1
    assert c["phases"]["total"]["buckets"][3] == 2 and c["phases"]["total"]["buckets"][31] == 1
    assert snap["cells"]["block"]["direct"]["rejected"] == 1 and snap["cells"]["block"]["fold"]["calls"] == 0
    stub.records = [{"id": 4, "submission": 9, "cls": 1, "kind": 8, "sets": 3, "lease_ns": 50, "device_ns": 7},
                    {"id": 5, "submission": 9, "cls": 0, "kind": 3, "sets": 3, "engine": 1}]
    recs, dropped = T.trace()
    assert dropped == 3 and [r["id"] for r in recs] == [4, 5]
    assert (recs[0]["cls"], recs[0]["kind"], recs[0]["device_ns"]) == ("block", "device", 7)
    assert (recs[1]["cls"], recs[1]["kind"], recs[1]["engine"]) == ("normal", "span_checks", 1)
    assert set(recs[0]) == {n for n, _ in G.TelemetryRecord._fields_}
    assert T.trace(1)[0] == recs[:1]
    assert T.memory() == []
    stub.engines = [{"hip_device": 0, "registry_bytes": 57600, "block_ws": 4096}, {"hip_device": 3, "registry_bytes": 1, "block_ws": 0}]
    mem = T.memory()
    assert [m["hip_device"] for m in mem] == [0, 3] and mem[0]["registry_bytes"] == 57600
    assert mem[0]["workspace_bytes"] == {"normal": 0, "block": 4096} and "reserved" not in mem[0]
    T.reset()
    assert stub.records == []


def test_bucket_edges():
    edges = T.bucket_edges_ns()
    assert len(edges) == 31 and edges[0] == 1024 and edges[-1] == 1 << 40
    assert all(b == 2 * a for a, b in zip(edges, edges[1:]))


def test_prometheus_text(stub):
    text = T.prometheus_text(T.read())
    assert text.endswith("\n") and "\n\n" not in text
    lines = text.splitlines()
    label = 'class="normal",kind="batch"'
    # only cells with something in them: normal/batch and the rejection of block/direct
    assert {re.search(r'class="(\w+)",kind="(\w+)"', ln).groups() for ln in lines if "{" in ln} == {("normal", "batch"),
                                                                                                  ("block", "direct")}
    for phase in (n.decode() for n in PHASES):
        fam = "gbls_%s_seconds" % phase
        assert "# TYPE %s histogram" % fam in lines
        rows = [ln for ln in lines if ln.startswith("%s_bucket{%s," % (fam, label))]
        assert len(rows) == 32
        les = [re.search(r'le="([^"]+)"', ln).group(1) for ln in rows]
        counts = [int(ln.rsplit(" ", 1)[1]) for ln in rows]
        assert les[-1] == "+Inf" and [float(x) for x in les[:-1]] == [(1 << (k + 10)) / 1e9 for k in range(31)]
        assert all(b >= a for a, b in zip(counts, counts[1:]))                    # cumulative
        count = int(next(ln for ln in lines if ln.startswith("%s_count{%s}" % (fam, label))).rsplit(" ", 1)[1])
        assert counts[-1] == count
        first = lines.index(rows[0])
        assert lines[first + 32].startswith(fam + "_sum{") and lines[first + 33].startswith(fam + "_count{")   # the order
    rows = [int(ln.rsplit(" ", 1)[1]) for ln in lines if ln.startswith('gbls_total_seconds_bucket{%s,' % label)]
    assert rows[:4] == [1, 2, 2, 4] and rows[30] == 4 and rows[31] == 5            # 900 | 1024 | 5000 5000 | 3 * 2^40
    total_sum = float(next(ln for ln in lines if ln.startswith("gbls_total_seconds_sum{%s}" % label)).rsplit(" ", 1)[1])
    assert total_sum == (900 + 1024 + 5000 + 5000 + (3 << 40)) / 1e9
    assert 'gbls_run_seconds_bucket{%s,le="1.024e-06"} 5' % label in lines
    assert "# TYPE gbls_calls_total counter" in lines and 'gbls_calls_total{%s} 5' % label in lines
    assert 'gbls_rejected_total{class="block",kind="direct"} 1' in lines and 'gbls_callers_total{%s} 5' % label in lines
    assert T.prometheus_text(T.read(), prefix="engine").startswith("# TYPE engine_hold_seconds histogram")
