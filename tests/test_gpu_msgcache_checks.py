"""The message line cache for per-check calls, and prefetch
(include/grandine_bls_gpu_msgcache_checks.h), on the GPU.  Expected verdicts come from the C oracle
(ref_verify / ref_multi_verify), and from the same call with serving off where the issue is that
nothing but the set-side work changes.  Every case restores configure(0) and serve_checks(0).

The helpers and fixtures are those of tests/test_gpu_msgcache.py (and, for the span and local
calls, of tests/test_gpu_each.py and tests/test_gpu_local.py)."""
import contextlib
import ctypes
import json
import os
import subprocess
import sys
import threading

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_each as T  # noqa: E402
import test_gpu_local as Q  # noqa: E402
import test_gpu_msgcache as M  # noqa: E402
import test_gpu_spans as S  # noqa: E402
from test_gpu_each import RV  # noqa: E402,F401  (fixture)
from test_gpu_local import K  # noqa: E402,F401  (fixture)
from test_gpu_msgcache import F, G, L, REF, REF_FAST  # noqa: E402,F401  (fixtures)
from test_gpu_spans import E  # noqa: E402,F401  (fixture)

pytestmark = pytest.mark.gpu

ROOT = M.ROOT
CHILD = os.path.join(ROOT, "tests", "gpu_msgcache_checks_child.py")
ENTERED, PRESENT, SKIPPED = 0, 1, 2
CSTATS = ("prefetched", "check_lookups", "check_hits", "check_published")
SET_SIDE = M.SET_SIDE
stats, delta, cache, stage_calls, batch, sub, corrupt, mv, u64 = (M.stats, M.delta, M.cache, M.stage_calls, M.batch,
                                                                  M.sub, M.corrupt, M.mv, M.u64)


def cstats(L):
    out = (ctypes.c_uint64 * 4)()
    assert L.gbls_msgcache_checks_stats(out) == 0
    return dict(zip(CSTATS, out))


def cdelta(L, before):
    now = cstats(L)
    return {k: now[k] - before[k] for k in CSTATS}


@contextlib.contextmanager
def serving(L, on=True):
    assert L.gbls_msgcache_serve_checks(1 if on else 0) == 0
    try:
        yield
    finally:
        L.gbls_msgcache_serve_checks(0)


def prefetch(G, L, roots, fill=77):
    n = len(roots)
    st = G.i32_array(n)
    for i in range(n):
        st[i] = fill
    rc = L.gbls_msgcache_prefetch(b"".join(roots), n, st)
    return rc, [st[i] for i in range(n)]


def roots_of(b):
    return [b["msgs"][32 * i:32 * i + 32] for i in range(b["n"])]


def verify1(L, b, i, sig_of=None):
    j = i if sig_of is None else sig_of
    return L.gbls_verify(b["sigs"][192 * j:192 * j + 192], b["msgs"][32 * i:32 * i + 32], 32, b["pks"][96 * i:96 * i + 96])


def ref1(C, b, i, sig_of=None):
    j = i if sig_of is None else sig_of
    return bool(C.ref_verify(b["sigs"][192 * j:192 * j + 192], b["msgs"][32 * i:32 * i + 32], 32,
                             b["pks"][96 * i:96 * i + 96]))


# ---------------------------------------------------------------- prefetch
def test_prefetch_cycle(G, L, F, REF):
    b = batch(F, [3, 3, 2], b"mcc/cycle")  # 8 sets on 3 roots
    roots = list(dict.fromkeys(roots_of(b)))
    bad = corrupt(b, 0, 3)
    assert len(roots) == 3 and M.ref_mv(REF, b) and not M.ref_mv(REF, bad)
    assert prefetch(G, L, roots) == (0, [SKIPPED] * 3)  # the cache is off
    assert L.gbls_msgcache_prefetch(None, 0, None) == 0
    assert L.gbls_msgcache_prefetch(None, 2, None) == G.VERIFY_FAIL and L.gbls_last_error() == 102
    with cache(L, 16):
        s0, c0 = stats(L), cstats(L)
        with stage_calls(L) as used:
            assert prefetch(G, L, roots) == (0, [ENTERED] * 3)
        d = delta(L, s0)
        assert (d["lookups"], d["hits"], d["misses"], d["published"], d["bypassed"]) == (3, 0, 3, 3, 0)
        assert stats(L)["entries"] == 3 and cdelta(L, c0)["prefetched"] == 3
        assert [used[k] for k in SET_SIDE] == [1, 1, 1, 1] and used["k_linecache_store"] == 1
        assert (used["k_ml_group"], used["k_final_verdict"], used["k_linecache_load"]) == (0, 0, 0)
        s1 = stats(L)
        with stage_calls(L) as warm:
            assert mv(L, b) and not mv(L, bad)
        d = delta(L, s1)
        assert (d["lookups"], d["hits"], d["misses"]) == (6, 6, 0)
        assert [warm[k] for k in SET_SIDE] == [0, 0, 0, 0] and warm["k_linecache_load"] == 2
        # a repeated root is handled once; every occurrence reports the same
        assert prefetch(G, L, roots + roots[:1]) == (0, [PRESENT] * 4)
        assert L.gbls_msgcache_prefetch(b"".join(roots), 3, None) == 0  # status may be NULL
        assert L.gbls_msgcache_clear() == 0 and stats(L)["entries"] == 0
        assert prefetch(G, L, [roots[1], roots[1], roots[0]]) == (0, [ENTERED] * 3) and stats(L)["entries"] == 2
    with stage_calls(L) as off:
        assert prefetch(G, L, roots) == (0, [SKIPPED] * 3)
    assert sum(off.values()) == 0


def test_prefetch_capacity(G, L, F):
    spare = 64  # spare_for(4)
    roots = [F.messages(spare + 8, b"mcc/cap")[32 * i:32 * i + 32] for i in range(spare + 8)]
    with cache(L, 4):
        s0 = stats(L)
        assert prefetch(G, L, roots[:6]) == (0, [ENTERED] * 6)
        d = delta(L, s0)
        assert (stats(L)["entries"], d["evictions"], d["published"]) == (4, 2, 6)
        assert prefetch(G, L, roots[2:6]) == (0, [PRESENT] * 4)
        assert prefetch(G, L, roots[:2]) == (0, [ENTERED] * 2)
        s1 = stats(L)
        rc, st = prefetch(G, L, roots[6:6 + spare + 1])  # one more missing root than spare slots
        assert rc == 0 and st == [ENTERED] * spare + [SKIPPED]
        d = delta(L, s1)
        assert d["lookups"] == d["hits"] + d["misses"] == spare + 1 and d["bypassed"] == 1 and d["published"] == spare
        assert stats(L)["entries"] == 4


def test_prefetch_generators(G, L, F, REF_FAST):
    """1025 roots in one call: above kW4Max, the row/quad generators; their lines serve small calls."""
    wide = batch(F, [1] * 1025, b"mc/wide")
    four = sub(wide, [0, 511, 1023, 1024])
    bad = corrupt(four, 1, 2)
    assert M.ref_mv(REF_FAST, four) and not M.ref_mv(REF_FAST, bad)
    with cache(L, 4100):  # spare_for(4100) == 1025
        assert prefetch(G, L, roots_of(wide)) == (0, [ENTERED] * 1025)
        s0 = stats(L)
        with stage_calls(L) as used:
            assert mv(L, four) and not mv(L, bad)
        assert (delta(L, s0)["hits"], delta(L, s0)["misses"]) == (8, 0) and used["k_lines"] == 0


# ---------------------------------------------------------------- serving
def test_serving_off_moves_no_counter(G, L, F, REF):
    b = batch(F, [1, 1], b"mcc/off")
    assert ref1(REF, b, 0)
    assert L.gbls_msgcache_serve_checks(0) == 0  # off by default
    with cache(L, 16):
        s0, c0 = stats(L), cstats(L)
        assert verify1(L, b, 0) == 0 and verify1(L, b, 0, sig_of=1) == G.VERIFY_FAIL
        assert set(delta(L, s0).values()) == {0} and set(cdelta(L, c0).values()) == {0} and stats(L)["entries"] == 0


def test_serving_single_checks(G, L, F, REF):
    b = batch(F, [1, 1, 1], b"mcc/one")
    assert ref1(REF, b, 0) and not ref1(REF, b, 0, sig_of=1) and not ref1(REF, b, 2, sig_of=1)
    with cache(L, 16), serving(L):
        assert L.gbls_msgcache_serve_checks(1) == 1  # the previous setting
        s0, c0 = stats(L), cstats(L)
        with stage_calls(L) as cold:
            assert verify1(L, b, 0) == 0
        d = delta(L, s0)
        assert (d["lookups"], d["misses"], d["published"]) == (1, 1, 1)
        assert cdelta(L, c0) == dict(prefetched=0, check_lookups=1, check_hits=0, check_published=1)
        assert [cold[k] for k in SET_SIDE] == [1, 1, 1, 1] and cold["k_linecache_store"] == 1
        s1 = stats(L)
        with stage_calls(L) as warm:
            assert verify1(L, b, 0) == 0 and verify1(L, b, 0, sig_of=1) == G.VERIFY_FAIL
        d = delta(L, s1)
        assert (d["lookups"], d["hits"], d["misses"], d["published"]) == (2, 2, 0, 0)
        assert [warm[k] for k in SET_SIDE] == [0, 0, 0, 0] and warm["k_linecache_load"] == 2
        assert warm["k_final_verdict"] == 2
        s2 = stats(L)
        assert verify1(L, b, 2, sig_of=1) == G.VERIFY_FAIL  # cold and invalid: nothing published
        d = delta(L, s2)
        assert (d["misses"], d["published"]) == (1, 0) and stats(L)["entries"] == 1
        # fast_aggregate_verify over three keys on one root
        agg = batch(F, [3], b"mcc/fav")
        sk = sum(agg["sks"]) % F.R_ORDER
        sig = F.sign([sk], agg["msgs"][:32])
        s3 = stats(L)
        for _ in range(2):
            assert L.gbls_fast_aggregate_verify(sig, agg["msgs"][:32], 32, agg["pks"], 3) == 0
        assert L.gbls_fast_aggregate_verify(sig, agg["msgs"][:32], 32, agg["pks"], 2) == G.VERIFY_FAIL
        d = delta(L, s3)
        assert (d["hits"], d["misses"], d["published"]) == (2, 1, 1)


def test_verify_batch_compressed(G, L, F, REF):
    """5 checks on 3 roots A B C (A B A C B): check 3 (C) carries check 0's signature, check 4's
    signature (B) is undecodable.  A and B have a passing check, C has none."""
    b = batch(F, [2, 2, 1], b"mcc/vbc")
    assert b["of"] == [0, 1, 2, 0, 1]
    b = sub(b, [0, 1, 3, 2, 4])
    assert b["of"] == [0, 1, 0, 2, 1]
    comp = bytearray(M.compress(G, L, b["sigs"], 5))
    comp[96 * 3:96 * 4] = comp[0:96]
    comp[96 * 4] &= 0x7F  # the compression flag
    comp = bytes(comp)
    want = [ref1(REF, b, 0), ref1(REF, b, 1), ref1(REF, b, 2), ref1(REF, b, 3, sig_of=0), False]
    assert want == [True, True, True, False, False]

    def call():
        st, v = G.i32_array(5), G.i32_array(5)
        rc = L.gbls_verify_batch_compressed(b["msgs"], comp, b["pks"], None, 5, st, v)
        return rc, [st[i] for i in range(5)], [v[i] for i in range(5)]

    plain = call()
    assert plain[0] == 0 and [x == 0 for x in plain[2]] == want and plain[1][:4] == [0] * 4 and plain[1][4] != 0
    with cache(L, 16):
        assert call() == plain  # serving off
        with serving(L):
            s0 = stats(L)
            with stage_calls(L) as cold:
                assert call() == plain
            d = delta(L, s0)
            # three messages hashed, not five: the other two pairs copy their lines
            assert (d["lookups"], d["hits"], d["misses"], d["published"]) == (3, 0, 3, 2)
            assert [cold[k] for k in SET_SIDE] == [1, 1, 1, 1]
            assert (cold["k_linecache_store"], cold["k_linecache_load"]) == (1, 1)
            s1 = stats(L)
            with stage_calls(L) as warm:
                assert call() == plain
            d = delta(L, s1)
            assert (d["lookups"], d["hits"], d["misses"], d["published"]) == (3, 2, 1, 0)
            assert stats(L)["entries"] == 2
            # only A and B were published
            assert prefetch(G, L, [b["msgs"][0:32], b["msgs"][32:64], b["msgs"][96:128]]) == (0, [PRESENT, PRESENT, ENTERED])
            with stage_calls(L) as hot:
                assert call() == plain
            assert [hot[k] for k in SET_SIDE] == [0, 0, 0, 0] and hot["k_linecache_load"] == 1


def test_grouped_regime_is_bypassed(G, L, F, REF_FAST):
    b = batch(F, [1025, 1025], b"mcc/grouped")
    n = b["n"]
    bad = corrupt(corrupt(b, 7, 9), 2049, 0)
    assert [ref1(REF_FAST, bad, i) for i in (0, 7, 8, 2048, 2049)] == [True, False, True, True, False]

    def call():
        v = G.i32_array(n)
        rc = L.gbls_aggregate_verify_batch(bad["sigs"], bad["msgs"], G.u32_array(range(0, 32 * n + 1, 32)), bad["pks"], n, v)
        return rc, [v[i] for i in range(n)]

    prev = L.gbls_set_policy(0)
    try:
        L.gbls_set_policy(prev & ~G.INIT_PER_CHECK)  # the grouped regime is the default policy's
        off = call()
        assert off[0] == 0 and [i for i in range(n) if off[1][i] != 0] == [7, 2049]
        with cache(L, 16), serving(L):
            s0 = stats(L)
            assert call() == off
            d = delta(L, s0)
            assert d["bypassed"] == n and d["lookups"] == 0 and stats(L)["entries"] == 0
            # GBLS_INIT_PER_CHECK: no grouped regime, the same checks are served
            L.gbls_set_policy(prev | G.INIT_PER_CHECK)
            s1 = stats(L)
            assert call() == off
            d = delta(L, s1)
            assert (d["bypassed"], d["lookups"], d["misses"], d["published"]) == (0, 2, 2, 2)
    finally:
        L.gbls_set_policy(prev)


# ---------------------------------------------------------------- the span and local calls
def test_each_spans(G, L, F, RV, E):
    """16 sets of the spans suite (the non-signer, the malformed set, the set without participants
    among them) on 4 roots, one signature undecodable: all outputs identical off, cold and warm."""
    sets, signing, planted = T.each_sets(E)
    order = list(range(44, 60))
    assert planted["malformed"] in order
    chunk, sign = [sets[i] for i in order], [signing[i] for i in order]
    um = F.messages(4, b"mcc/spans")
    msgs = b"".join(um[32 * (k % 4):32 * (k % 4) + 32] for k in range(16))
    comp = S.compress(G, L, F.sign([sum(E.sks[v] for v in s.part) % F.R_ORDER or 1 for s in sign], msgs))
    comp = T.clear_flag(comp, 3)
    off = T.each(G, L, msgs, comp, chunk)
    sst, pts = T.decode(G, L, comp)
    want = [G.SUCCESS if off[2][k] == 0 and off[3][k] == 0 and
            RV.ref_verify(pts[k], msgs[32 * k:32 * k + 32], 32, S.oracle_key(RV, E, F, chunk[k].part)) else G.VERIFY_FAIL
            for k in range(16)]
    assert off[:2] == (0, 0) and off[2] == sst and off[4] == want and 0 < sum(x == 0 for x in want) < 16
    assert all(any(want[k] == 0 for k in range(r, 16, 4)) for r in range(4))  # every root has a passing check
    with cache(L, 16), serving(L):
        s0 = stats(L)
        assert T.each(G, L, msgs, comp, chunk) == off  # cold
        d = delta(L, s0)
        assert (d["lookups"], d["misses"], d["published"]) == (4, 4, 4)
        s1 = stats(L)
        assert T.each(G, L, msgs, comp, chunk) == off  # warm
        assert (delta(L, s1)["hits"], delta(L, s1)["misses"]) == (4, 0)


def test_each_local(G, L, F, RV, E, K):
    """The first 40 sets of the local suite's environment (distinct roots; valid and undecodable
    local keys, swapped and undecodable signatures among them): all outputs identical off, cold and warm."""
    sets, planted, table, key_sk, msgs, comp = Q.each_env(G, L, F, RV, E, K)
    lo = list(range(40))
    args = (b"".join(msgs[32 * i:32 * i + 32] for i in lo), b"".join(comp[96 * i:96 * i + 96] for i in lo),
            [sets[i] for i in lo], table)
    off = Q.each_local(G, L, *args)
    npass = sum(x == 0 for x in off[4])
    assert off[:2] == (0, 0) and 0 < npass < 40
    sst, pts = T.decode(G, L, args[1])
    for k, i in enumerate(lo):  # the oracle on the local sets that have a key and a signature
        if Q.is_local(sets[i]) and key_sk[i] is not None and sst[k] == 0:
            ok = RV.ref_verify(pts[k], msgs[32 * i:32 * i + 32], 32, Q.ref_pk(RV, F, key_sk[i]))
            assert (off[4][k] == 0) == bool(ok), i
    with cache(L, 64), serving(L):
        s0 = stats(L)
        assert Q.each_local(G, L, *args) == off  # cold
        d = delta(L, s0)
        assert (d["misses"], d["published"]) == (40, npass)
        s1 = stats(L)
        assert Q.each_local(G, L, *args) == off  # warm: the published roots hit
        assert (delta(L, s1)["hits"], delta(L, s1)["misses"]) == (npass, 40 - npass)


# ---------------------------------------------------------------- concurrency
def test_concurrent_checks_with_clear_configure_and_prefetch(G, L, F, REF):
    pool = batch(F, [4] * 5, b"mcc/conc")  # 5 roots, 4 keys each
    roots = list(dict.fromkeys(roots_of(pool)))
    jobs = [(t, k, (3 * t + 7 * k) % 20, ((3 * t + 7 * k + 1) % 20) if k % 3 == 2 else None) for t in range(4)
            for k in range(20)]
    want = {(t, k): ref1(REF, pool, i, j) for t, k, i, j in jobs}
    assert 0 < sum(want.values()) < len(want)
    got = {}
    stop = threading.Event()

    def worker(t):
        for tt, k, i, j in jobs:
            if tt == t:
                got[(t, k)] = verify1(L, pool, i, j) == 0

    def churn():
        i = 0
        while not stop.is_set():
            if i % 3 == 0:
                L.gbls_msgcache_configure(8 if i % 2 else 3)
            elif i % 3 == 1:
                L.gbls_msgcache_clear()
            else:
                assert L.gbls_msgcache_prefetch(b"".join(roots), 5, None) == 0
            i += 1
            stop.wait(0.002)

    prev = L.gbls_set_policy(0)
    L.gbls_set_policy(prev & ~G.INIT_NO_COALESCE)  # the coalescer on
    assert L.gbls_msgcache_configure(3) == 0 and L.gbls_msgcache_serve_checks(1) == 0
    try:
        s0 = stats(L)
        th = [threading.Thread(target=worker, args=(t,)) for t in range(4)] + [threading.Thread(target=churn)]
        for x in th:
            x.start()
        for x in th[:4]:
            x.join(120)
        stop.set()
        th[4].join(10)
        assert not any(x.is_alive() for x in th)
        assert got == want
        d = delta(L, s0)
        assert d["lookups"] == d["hits"] + d["misses"] > 0
    finally:
        stop.set()
        L.gbls_set_policy(prev)
        L.gbls_msgcache_serve_checks(0)
        assert L.gbls_msgcache_configure(0) == 0


# ---------------------------------------------------------------- two engines
def test_two_engines_on_one_gpu():
    out = subprocess.run([sys.executable, CHILD, "replicas"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["engines"] == 2 and r["ref"] == [True, False]
    assert r["first"] == [ENTERED] * r["distinct"] and r["entries"] == 2 * r["distinct"]
    assert r["again"] == [PRESENT] * r["distinct"]
    assert r["stats_prefetch"]["misses"] == r["stats_prefetch"]["published"] == 2 * r["distinct"]
    assert r["warm"] == [True, False] * 4 and r["stats_warm"]["hits"] == 8 and r["stats_warm"]["misses"] == 0
