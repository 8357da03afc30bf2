"""Engine telemetry (include/grandine_bls_gpu_telemetry.h): what the engine did with each call.

``enable(level)`` switches recording on (0 off, 1 counters and host-clock phases, 2 adds device time
per shard); ``read()`` returns the counters and histograms as nested dicts keyed by the engine's own
class, kind and phase names; ``trace()`` drains the ring of the most recent shard records;
``memory()`` returns the memory gauges per engine; ``reset()`` clears the counters.
``prometheus_text(snapshot)`` renders a snapshot as Prometheus exposition text, which a node's
metrics service can append to its own.

None of these needs a device: before the engine is initialised the counters are zero and
``memory()`` lists no engine.
"""

from __future__ import annotations

import ctypes
from typing import Dict, List, Tuple

from . import _lib as G

COUNTERS = ("calls", "sets", "rejected", "engine_errors", "submissions", "shards", "callers", "submitted_sets",
            "fresh_contexts", "staging_waits", "growths")
RECORD_FIELDS = tuple(n for n, _ in G.TelemetryRecord._fields_)
MEMORY_FIELDS = tuple(n for n, _ in G.TelemetryEngineMemory._fields_ if n != "reserved")


def _names(fn) -> List[str]:
    out, i = [], 0
    while True:
        s = fn(i)
        if s is None:
            return out
        out.append(s.decode())
        i += 1


def names() -> Tuple[List[str], List[str], List[str]]:
    """(classes, kinds, phases) as the engine names them."""
    L = G.load_library()
    return (_names(L.gbls_telemetry_class_name), _names(L.gbls_telemetry_kind_name),
            _names(L.gbls_telemetry_phase_name))


def bucket_edges_ns() -> List[int]:
    """Exclusive upper edges of the histogram buckets but the last: bucket 0 holds d < 1024 ns,
    bucket k 2^(k+9) <= d < 2^(k+10) ns, the last bucket everything from 2^40 ns up."""
    return [1 << (k + 10) for k in range(G.TELEMETRY_BUCKETS - 1)]


def enable(level: int) -> int:
    """Set the level (process-wide, sticky); returns the previous one."""
    return G.load_library().gbls_telemetry_enable(int(level))


def reset() -> None:
    G.load_library().gbls_telemetry_reset()


def _hist(h) -> Dict:
    return {"count": h.count, "sum_ns": h.sum_ns, "max_ns": h.max_ns, "buckets": list(h.bucket)}


def read() -> Dict:
    """{"level", "trace_written", "trace_dropped", "cells": {class: {kind: {counter..., "callers_bin",
    "sets_bin", "phases": {phase: {"count", "sum_ns", "max_ns", "buckets"}}}}}}."""
    L = G.load_library()
    snap = G.TelemetrySnapshot()
    if L.gbls_telemetry_read(ctypes.byref(snap), ctypes.sizeof(snap)) != G.SUCCESS:
        raise G.EngineUnavailable("gbls_telemetry_read failed")
    classes, kinds, phases = names()
    cells: Dict = {}
    for a, cname in enumerate(classes):
        cells[cname] = {}
        for k, kname in enumerate(kinds):
            c = snap.cell[a][k]
            cell = {n: getattr(c, n) for n in COUNTERS}
            cell["callers_bin"] = list(c.callers_bin)
            cell["sets_bin"] = list(c.sets_bin)
            cell["phases"] = {p: _hist(c.phase[i]) for i, p in enumerate(phases)}
            cells[cname][kname] = cell
    return {"level": snap.level, "trace_written": snap.trace_written, "trace_dropped": snap.trace_dropped,
            "cells": cells}


def trace(max_records: int = G.TELEMETRY_TRACE_CAPACITY) -> Tuple[List[Dict], int]:
    """(records, dropped): the unread shard records, oldest first, class and kind by name, and the
    number of records lost since the previous drain."""
    L = G.load_library()
    classes, kinds, _ = names()
    recs = (G.TelemetryRecord * max(1, max_records))()
    dropped = ctypes.c_uint64(0)
    n = L.gbls_telemetry_trace(recs, max_records, ctypes.byref(dropped))
    out = []
    for i in range(n):
        d = {f: getattr(recs[i], f) for f in RECORD_FIELDS}
        d["cls"], d["kind"] = classes[d["cls"]], kinds[d["kind"]]
        out.append(d)
    return out, dropped.value


def memory() -> List[Dict]:
    """One dict of gauges per engine device; empty before the engine is initialised."""
    L = G.load_library()
    info = G.TelemetryMemoryInfo()
    if L.gbls_telemetry_memory(ctypes.byref(info), ctypes.sizeof(info)) != G.SUCCESS:
        raise G.EngineUnavailable("gbls_telemetry_memory failed")
    classes = names()[0]
    out = []
    for e in range(info.engines):
        m = info.engine[e]
        d = {}
        for f in MEMORY_FIELDS:
            v = getattr(m, f)
            d[f] = v if isinstance(v, int) else {classes[i]: v[i] for i in range(len(classes))}
        out.append(d)
    return out


def _seconds(ns: int) -> str:
    return repr(ns / 1e9)


def prometheus_text(snapshot: Dict, prefix: str = "gbls") -> str:
    """Prometheus exposition text of a ``read()`` snapshot: one histogram family per phase
    (``<prefix>_<phase>_seconds``: cumulative ``_bucket{le=...}`` lines, then ``_sum`` and
    ``_count``) and one counter family per counter, labelled with class and kind.  Cells without a
    call, a rejection or a shard are left out."""
    edges = bucket_edges_ns()
    lines: List[str] = []
    cells = [(a, k, c) for a, row in snapshot["cells"].items() for k, c in row.items()
             if c["calls"] or c["rejected"] or c["shards"]]
    phases = list(cells[0][2]["phases"]) if cells else []
    for p in phases:
        fam = "%s_%s_seconds" % (prefix, p)
        lines.append("# TYPE %s histogram" % fam)
        for a, k, c in cells:
            h = c["phases"][p]
            label = 'class="%s",kind="%s"' % (a, k)
            run = 0
            for edge, b in zip(edges, h["buckets"]):
                run += b
                lines.append('%s_bucket{%s,le="%s"} %d' % (fam, label, _seconds(edge), run))
            total = run + h["buckets"][len(edges)]  # (not h["count"]: a snapshot taken under load is exact only per counter)
            lines.append('%s_bucket{%s,le="+Inf"} %d' % (fam, label, total))
            lines.append("%s_sum{%s} %s" % (fam, label, _seconds(h["sum_ns"])))
            lines.append("%s_count{%s} %d" % (fam, label, total))
    for n in COUNTERS:
        fam = "%s_%s_total" % (prefix, n)
        lines.append("# TYPE %s counter" % fam)
        for a, k, c in cells:
            lines.append('%s{class="%s",kind="%s"} %d' % (fam, a, k, c[n]))
    return "\n".join(lines) + "\n"
