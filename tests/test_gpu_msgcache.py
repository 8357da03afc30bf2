"""Message line cache (include/grandine_bls_gpu_msgcache.h) on the GPU: calls that find a message in
the cache skip hash_to_G2 and line generation for it, and every verdict, per-set rejection and
signature status stays what it is without the cache.  Expected verdicts come from the C oracle
(ref_multi_verify / ref_verify) on the same sets and scalars, never from the engine.  Every case
restores configure(0)."""
import contextlib
import ctypes
import json
import os
import subprocess
import sys
import threading

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "gpu_msgcache_child.py")
STATS = ("lookups", "hits", "misses", "published", "evictions", "bypassed", "entries", "reserved")
SET_SIDE = ("k_h2c_field", "k_h2c_map", "k_h2c_clear", "k_lines")


@pytest.fixture(scope="module")
def G():
    from grandine_amd import _lib as G
    G.lib()
    return G


@pytest.fixture(scope="module")
def L(G):
    return G.lib()


@pytest.fixture(scope="module")
def F(G):
    from grandine_amd import factory
    return factory


def _oracle(name):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
    C = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", name))
    C.ref_multi_verify.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                   ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_int]
    C.ref_verify.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    C.ref_sk_to_pk.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return C


@pytest.fixture(scope="module")
def REF():
    return _oracle("libbls_ref.so")


@pytest.fixture(scope="module")
def REF_FAST():
    return _oracle("libbls_ref_fast.so")


def u64(vals):
    return (ctypes.c_uint64 * max(len(vals), 1))(*vals)


def ref_mv(C, b, lo=0, hi=None):
    hi = b["n"] if hi is None else hi
    return bool(C.ref_multi_verify(b["msgs"][32 * lo:32 * hi], b["sigs"][192 * lo:192 * hi], b["pks"][96 * lo:96 * hi],
                                   u64(b["rands"][lo:hi]), hi - lo, 16))


def stats(L):
    out = (ctypes.c_uint64 * 8)()
    assert L.gbls_msgcache_stats(out) == 0
    return dict(zip(STATS, out))


def delta(L, before):
    now = stats(L)
    return {k: now[k] - before[k] for k in STATS[:6]}


@contextlib.contextmanager
def cache(L, slots):
    assert L.gbls_msgcache_slots() == 0
    assert L.gbls_msgcache_configure(slots) == 0 and L.gbls_msgcache_slots() == slots
    try:
        yield
    finally:
        assert L.gbls_msgcache_configure(0) == 0
        assert L.gbls_msgcache_slots() == 0 and stats(L)["entries"] == 0


@contextlib.contextmanager
def policy(L, G, on):
    prev = L.gbls_set_policy(0)
    L.gbls_set_policy((prev | G.INIT_DEDUP) if on else (prev & ~G.INIT_DEDUP))
    try:
        yield
    finally:
        L.gbls_set_policy(prev)


@contextlib.contextmanager
def stage_calls(L):
    """The stage-call counts of the calls inside, by stage name (filled on exit)."""
    names = [L.gbls_stage_name(k).decode() for k in range(32) if L.gbls_stage_name(k)]
    out = {}
    calls = (ctypes.c_uint32 * 32)()
    L.gbls_profile(1)
    try:
        L.gbls_profile_read(None, calls, 32)
        before = list(calls)
        yield out
        L.gbls_profile_read(None, calls, 32)
        out.update({n: calls[k] - before[k] for k, n in enumerate(names)})
    finally:
        L.gbls_profile(0)


def batch(F, sizes, seed, interleave=True):
    """Single-key sets signing len(sizes) distinct messages, sizes[g] sets on message g."""
    n = sum(sizes)
    if interleave:
        left, of = list(sizes), []
        while len(of) < n:
            for g in range(len(sizes)):
                if left[g]:
                    left[g] -= 1
                    of.append(g)
    else:
        of = [g for g, s in enumerate(sizes) for _ in range(s)]
    um = F.messages(len(sizes), seed)
    msgs = b"".join(um[32 * g:32 * g + 32] for g in of)
    sks = F.seeded_sks(n, seed)
    return dict(n=n, of=of, sks=sks, msgs=msgs, sigs=F.sign(sks, msgs), pks=F.public_keys(sks),
                rands=F.rands(n, sum(seed) + n))


def sub(b, idx):
    """The sets idx of b as a batch of their own."""
    return dict(n=len(idx), of=[b["of"][i] for i in idx], msgs=b"".join(b["msgs"][32 * i:32 * i + 32] for i in idx),
                sigs=b"".join(b["sigs"][192 * i:192 * i + 192] for i in idx),
                pks=b"".join(b["pks"][96 * i:96 * i + 96] for i in idx), rands=[b["rands"][i] for i in idx])


def corrupt(b, i, j):
    """Set i carries set j's signature."""
    s = bytearray(b["sigs"])
    s[192 * i:192 * i + 192] = b["sigs"][192 * j:192 * j + 192]
    return dict(b, sigs=bytes(s))


def mv(L, b):
    return L.gbls_multi_verify(b["msgs"], b["sigs"], b["pks"], u64(b["rands"]), b["n"]) == 0


# ---------------------------------------------------------------- 1. cold, then warm
def test_off_by_default_and_argument_errors(G, L):
    assert L.gbls_msgcache_slots() == 0
    assert L.gbls_msgcache_configure((1 << 20) + 1) == G.VERIFY_FAIL and L.gbls_last_error() == 102
    assert L.gbls_msgcache_slots() == 0
    assert L.gbls_msgcache_stats(None) == G.VERIFY_FAIL and L.gbls_last_error() == 102
    assert L.gbls_msgcache_clear() == 0


def test_cold_then_warm(G, L, F, REF):
    b = batch(F, [3, 3, 2], b"mc/cold")  # 8 sets on 3 messages
    assert ref_mv(REF, b)
    with cache(L, 16):
        s0 = stats(L)
        with stage_calls(L) as cold:
            assert mv(L, b)
        d = delta(L, s0)
        assert (d["lookups"], d["hits"], d["misses"], d["published"], d["bypassed"]) == (3, 0, 3, 3, 0)
        assert stats(L)["entries"] == 3
        assert [cold[k] for k in SET_SIDE] == [1, 1, 1, 1]
        assert (cold["k_linecache_load"], cold["k_linecache_store"]) == (0, 1)
        s1 = stats(L)
        with stage_calls(L) as warm:
            assert mv(L, b)
        d = delta(L, s1)
        assert (d["lookups"], d["hits"], d["misses"], d["published"]) == (3, 3, 0, 0)
        assert [warm[k] for k in SET_SIDE] == [0, 0, 0, 0]
        assert (warm["k_linecache_load"], warm["k_linecache_store"]) == (1, 0)
        assert warm["k_ml_group"] == 1 and warm["k_final_verdict"] == 1
        # clear: the capacity stays, the entries go, the next call is cold again
        assert L.gbls_msgcache_clear() == 0 and L.gbls_msgcache_slots() == 16 and stats(L)["entries"] == 0
        s2 = stats(L)
        assert mv(L, b)
        assert delta(L, s2)["misses"] == 3
    with stage_calls(L) as off:  # the cache off again: the plain path, no cache kernels
        assert mv(L, b)
    assert (off["k_linecache_load"], off["k_linecache_store"], off["k_g1s_msgsum"]) == (0, 0, 0)


# ---------------------------------------------------------------- 2. warm and invalid
def test_warm_and_invalid(G, L, F, REF):
    b = batch(F, [3, 3, 2], b"mc/inv")
    of = b["of"]
    same = [i for i in range(8) if of[i] == 0]
    other = of.index(1)
    cases = {
        "same message": corrupt(b, same[0], same[1]),
        "across messages": corrupt(corrupt(b, same[0], other), other, same[0]),
        "infinite key": dict(b, pks=b["pks"][:96 * 2] + bytes(96) + b["pks"][96 * 3:]),
    }
    want = {k: ref_mv(REF, c) for k, c in cases.items()}
    assert want == {"same message": False, "across messages": False, "infinite key": False}
    zero = dict(b, rands=b["rands"][:4] + [0] + b["rands"][5:])  # the reference only draws nonzero scalars
    comp = ctypes.create_string_buffer(96 * 8)
    G.check(L.gbls_g2_compress(b["sigs"], 8, comp), "compress")
    undecodable = bytearray(comp.raw)
    undecodable[96 * 5] &= 0x7F  # the compression flag

    def compressed(raw):
        st = G.i32_array(8)
        rc = L.gbls_multi_verify_compressed(b["msgs"], bytes(raw), b["pks"], None, None, u64(b["rands"]), 8, st)
        return rc, list(st)

    plain = {k: mv(L, c) for k, c in cases.items()}
    plain_zero, plain_dec = mv(L, zero), compressed(undecodable)
    assert plain == want and not plain_zero
    assert plain_dec[0] == plain_dec[1][5] != 0 and plain_dec[1][:5] + plain_dec[1][6:] == [0] * 7
    with cache(L, 16):
        assert mv(L, b)  # warms the three messages
        s0 = stats(L)
        with stage_calls(L) as used:
            got = {k: mv(L, c) for k, c in cases.items()}
            got_zero, got_dec = mv(L, zero), compressed(undecodable)
        assert got == want and got_zero == plain_zero and got_dec == plain_dec
        d = delta(L, s0)
        assert d["hits"] == d["lookups"] > 0 and d["published"] == 0
        assert used["k_lines"] == 0 and used["k_linecache_load"] >= 4
        assert compressed(comp.raw) == (0, [0] * 8)
        assert mv(L, b)  # and the entries still serve the valid batch


def test_failed_cold_batch_publishes_nothing(G, L, F, REF):
    b = batch(F, [2, 2], b"mc/fail")
    bad = corrupt(b, 0, 2)
    assert not ref_mv(REF, bad) and ref_mv(REF, b)
    with cache(L, 16):
        s0 = stats(L)
        assert not mv(L, bad)
        d = delta(L, s0)
        assert (d["misses"], d["published"]) == (2, 0) and stats(L)["entries"] == 0
        s1 = stats(L)
        assert mv(L, b)
        d = delta(L, s1)
        assert (d["hits"], d["misses"], d["published"]) == (0, 2, 2)
        assert mv(L, b) and delta(L, s1)["hits"] == 2


# ---------------------------------------------------------------- 3. segments
def test_mixed_hits_and_misses_in_segments(G, L, F, REF):
    """Messages A B C D.  Warm: A, B.  Segment 0: A B (all hits); segment 1: B C C (B shared with
    segment 0; invalid); segment 2: D D (all misses).  C rides only in the failing segment."""
    b = batch(F, [2, 3, 2, 2], b"mc/seg", interleave=False)  # A: 0 1, B: 2 3 4, C: 5 6, D: 7 8
    order = [0, 2, 3, 5, 6, 7, 8]
    x = sub(b, order)  # A B | B C C | D D
    seg = [0, 2, 5, 7]
    bad = corrupt(x, 3, 4)  # the two C sets: set 3 carries set 4's signature
    want = [ref_mv(REF, bad, seg[s], seg[s + 1]) for s in range(3)]
    assert want == [True, False, True]
    with cache(L, 16):
        assert mv(L, sub(b, [1, 4]))  # warms A and B
        s0 = stats(L)
        v = G.i32_array(3)
        with stage_calls(L) as used:
            rc = L.gbls_multi_verify_segments(bad["msgs"], bad["sigs"], bad["pks"], u64(bad["rands"]), 7,
                                              G.u32_array(seg), 3, v)
        assert rc == G.SUCCESS and [s == 0 for s in v] == want
        d = delta(L, s0)
        # distinct messages A B C D: two hits, two misses; only D's segment passed
        assert (d["lookups"], d["hits"], d["misses"], d["published"]) == (4, 2, 2, 1)
        assert (used["k_linecache_load"], used["k_linecache_store"], used["k_lines"]) == (1, 1, 1)
        s1 = stats(L)
        assert mv(L, sub(b, [7, 8])) and delta(L, s1)["hits"] == 1  # D is there
        s2 = stats(L)
        assert mv(L, sub(b, [5, 6])) and delta(L, s2)["misses"] == 1  # C is not


# ---------------------------------------------------------------- 4. every entry point
@pytest.fixture(scope="module")
def entry_env(G, L, F, REF):
    """12 sets on 3 messages whose keys are registry keys (for the indexed and committee forms)."""
    class E:
        pass
    e = E()
    e.reg_sks, e.reg = F.registry(64, b"mc/reg")
    assert not F.load_registry(e.reg).any()
    e.idx = [(7 * i + 3) % 64 for i in range(12)]
    um = F.messages(3, b"mc/entry")
    of = [i % 3 for i in range(12)]
    msgs = b"".join(um[32 * g:32 * g + 32] for g in of)
    sks = [e.reg_sks[k] for k in e.idx]
    e.b = dict(n=12, of=of, msgs=msgs, sigs=F.sign(sks, msgs), pks=F.public_keys(sks), rands=F.rands(12, 178))
    e.bad = corrupt(e.b, 4, 1)
    assert ref_mv(REF, e.b) and not ref_mv(REF, e.bad)
    # two committees of 8 registry keys; set i names committee i % 2 minus one absent member
    e.coms = [[(5 * c + 9 * j) % 64 for j in range(8)] for c in range(2)]
    e.absent = [[e.coms[i % 2][i % 8]] for i in range(12)]
    csk = [(sum(e.reg_sks[k] for k in e.coms[i % 2]) - e.reg_sks[e.absent[i][0]]) % F.R_ORDER for i in range(12)]
    cpk = b""
    for s in csk:
        out = ctypes.create_string_buffer(96)
        REF.ref_sk_to_pk(s.to_bytes(32, "big"), out)
        cpk += out.raw
    e.cb = dict(n=12, of=of, msgs=msgs, sigs=F.sign(csk, msgs), pks=cpk, rands=e.b["rands"])
    e.cbad = corrupt(e.cb, 7, 10)
    assert ref_mv(REF, e.cb) and not ref_mv(REF, e.cbad)
    return e


def compress(G, L, sigs, n):
    comp = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, comp), "compress")
    return comp.raw


@pytest.mark.parametrize("dedup", [False, True])
def test_every_entry_point(G, L, F, REF, entry_env, dedup):
    e = entry_env
    b, bad, r = e.b, e.bad, u64(e.b["rands"])
    idx = G.u32_array(e.idx)
    st = G.i32_array(12)
    assert not F.load_registry(e.reg).any()  # (another module may have rewritten the registry)
    cst = G.i32_array(2)
    flat = [k for c in e.coms for k in c]
    assert L.gbls_committees_set(0, G.u32_array(flat), G.u32_array([0, 8, 16]), 2, cst) == 0 and list(cst) == [0, 0]
    com = G.u32_array([i % 2 for i in range(12)])
    ab_idx, ab_off = G.u32_array([a[0] for a in e.absent]), G.u32_array(list(range(13)))
    # per-set truth of the bisected batch: two bad sets
    two_bad = corrupt(corrupt(b, 4, 1), 9, 0)
    per_set = [bool(REF.ref_verify(two_bad["sigs"][192 * i:192 * i + 192], two_bad["msgs"][32 * i:32 * i + 32], 32,
                                   two_bad["pks"][96 * i:96 * i + 96])) for i in range(12)]
    assert [i for i, ok in enumerate(per_set) if not ok] == [4, 9]

    def bisect(x):
        v = G.i32_array(12)
        assert L.gbls_multi_verify_bisect(x["msgs"], x["sigs"], x["pks"], None, None, r, 12, v) == G.SUCCESS
        return [s == 0 for s in v]

    calls = {
        "multi_verify": lambda x: L.gbls_multi_verify(x["msgs"], x["sigs"], x["pks"], r, 12) == 0,
        "indexed": lambda x: L.gbls_multi_verify_indexed(x["msgs"], x["sigs"], idx, None, r, 12) == 0,
        "compressed": lambda x: L.gbls_multi_verify_compressed(x["msgs"], compress(G, L, x["sigs"], 12), x["pks"], None,
                                                               G.u32_array(list(range(13))), r, 12, st) == 0,
    }
    try:
        with policy(L, G, dedup):
            for name, call in calls.items():
                with cache(L, 8):
                    s0 = stats(L)
                    assert call(b), name  # cold
                    assert (delta(L, s0)["misses"], delta(L, s0)["published"]) == (3, 3), name
                    s1 = stats(L)
                    assert call(b) and not call(bad), name  # warm
                    d = delta(L, s1)
                    assert (d["hits"], d["misses"]) == (6, 0), name
            with cache(L, 8):
                s0 = stats(L)
                assert bisect(two_bad) == per_set  # cold: the passing pieces publish
                assert delta(L, s0)["published"] == 3
                s1 = stats(L)
                assert bisect(two_bad) == per_set and bisect(b) == [True] * 12
                assert delta(L, s1)["misses"] == 0
            with cache(L, 8):
                def committees(x):
                    return L.gbls_multi_verify_committees(x["msgs"], compress(G, L, x["sigs"], 12), com, ab_idx, ab_off,
                                                          r, 12, st, 0) == 0
                s0 = stats(L)
                assert committees(e.cb)
                assert delta(L, s0)["published"] == 3
                s1 = stats(L)
                assert committees(e.cb) and not committees(e.cbad)
                assert (delta(L, s1)["hits"], delta(L, s1)["misses"]) == (6, 0)
    finally:
        L.gbls_committees_clear()


# ---------------------------------------------------------------- 5. eviction
def test_eviction(G, L, F, REF):
    b = batch(F, [1] * 6, b"mc/evict")
    assert all(ref_mv(REF, b, i, i + 1) for i in range(6)) and ref_mv(REF, b)
    with cache(L, 4):
        s0 = stats(L)
        for _ in range(3):
            for i in range(6):
                assert mv(L, sub(b, [i]))  # a batch verifies only on its own message's lines
        assert mv(L, b)
        d = delta(L, s0)
        assert d["evictions"] > 0 and stats(L)["entries"] <= 4
        assert d["lookups"] == d["hits"] + d["misses"] == 24
        # the last four singles are the entries; the six-message batch hits those four
        assert d["hits"] == 4 and d["published"] - d["evictions"] == stats(L)["entries"]


# ---------------------------------------------------------------- 6. across the line generators
@pytest.fixture(scope="module")
def wide(F):
    return batch(F, [1] * 1025, b"mc/wide")  # 1025 distinct messages: above kW4Max, the row/quad generators


def test_lines_of_the_large_generators_serve_small_calls(G, L, F, REF_FAST, wide):
    four = sub(wide, [0, 511, 1023, 1024])
    assert ref_mv(REF_FAST, wide) and ref_mv(REF_FAST, four)
    bad = corrupt(four, 1, 2)
    assert not ref_mv(REF_FAST, bad)
    with cache(L, 2048):
        s0 = stats(L)
        assert mv(L, wide)
        assert (delta(L, s0)["misses"], delta(L, s0)["published"]) == (1025, 1025)
        s1 = stats(L)
        with stage_calls(L) as used:
            assert mv(L, four) and not mv(L, bad) and mv(L, wide)
        assert (delta(L, s1)["hits"], delta(L, s1)["misses"]) == (4 + 4 + 1025, 0)
        assert used["k_lines"] == 0 and used["k_linecache_load"] == 3


def test_lines_of_the_small_generator_serve_a_large_call(G, L, F, REF_FAST, wide):
    four = sub(wide, [3, 500, 1000, 1024])
    with cache(L, 2048):
        assert mv(L, four)
        s0 = stats(L)
        assert mv(L, wide)  # 4 hits inside 1021 misses: the row generator beside cached one-wave lines
        assert (delta(L, s0)["hits"], delta(L, s0)["misses"]) == (4, 1021)
        assert not mv(L, corrupt(wide, 500, 501))


def child(*args):
    out = subprocess.run([sys.executable, CHILD] + list(args), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_lane_generator_in_a_fresh_process():
    r = child("lane")
    assert r["ref"] == [True, True, False]
    assert r["cold"] is True and r["warm_small"] == [True, False] and r["warm_all"] is True
    assert r["small_then_large"] is True
    assert r["stats_cold"]["published"] == r["n"] and r["stats_warm"]["misses"] == 0


# ---------------------------------------------------------------- 7. the MSM regime
@pytest.fixture(scope="module")
def msm_batch(F):
    return batch(F, [64] * 32, b"mc/msm")  # one segment of 2048 sets (kMsmMinPerSeg), 32 messages


def test_msm_regime(G, L, F, REF_FAST, msm_batch):
    b = msm_batch
    bad = corrupt(b, 1000, 1032)  # sets of one message
    assert b["of"][1000] == b["of"][1032]
    assert ref_mv(REF_FAST, b) and not ref_mv(REF_FAST, bad)
    with cache(L, 64):
        s0 = stats(L)
        with stage_calls(L) as cold:
            assert not mv(L, bad)  # cold and invalid: nothing published
            assert mv(L, b)        # cold and valid
        assert cold["k_msm"] == 2
        assert (delta(L, s0)["misses"], delta(L, s0)["published"]) == (64, 32)
        s1 = stats(L)
        with stage_calls(L) as warm:
            assert mv(L, b) and not mv(L, bad)
        assert (delta(L, s1)["hits"], delta(L, s1)["misses"]) == (64, 0)
        assert warm["k_msm"] == 2 and warm["k_lines"] == 0 and warm["k_linecache_load"] == 2


# ---------------------------------------------------------------- 8. concurrency
def test_concurrent_callers_with_clear_and_configure(G, L, F, REF):
    pool = batch(F, [4] * 5, b"mc/conc")  # 5 messages, 4 sets each
    by_msg = [[i for i in range(20) if pool["of"][i] == g] for g in range(5)]
    jobs = []
    for t in range(4):
        for k in range(20):
            g0, g1 = (t + k) % 5, (t + 2 * k + 1) % 5
            x = sub(pool, [by_msg[g0][k % 4], by_msg[g1][(k + 1) % 4], by_msg[g0][(k + 2) % 4]])
            if k % 3 == 2:
                x = corrupt(x, 0, 2)  # two sets of one message, different keys
            jobs.append((t, k, x))
    want = {(t, k): ref_mv(REF, x) for t, k, x in jobs}
    assert sum(want.values()) == 4 * 14
    got = {}
    stop = threading.Event()

    def worker(t):
        for tt, k, x in jobs:
            if tt == t:
                got[(t, k)] = mv(L, x)

    def churn():
        i = 0
        while not stop.is_set():
            L.gbls_msgcache_clear() if i % 2 else L.gbls_msgcache_configure(8 if i % 4 else 3)
            i += 1
            stop.wait(0.002)

    prev = L.gbls_set_policy(0)
    L.gbls_set_policy(prev & ~G.INIT_NO_COALESCE)  # the coalescer on
    assert L.gbls_msgcache_configure(3) == 0
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
        assert L.gbls_msgcache_configure(0) == 0


# ---------------------------------------------------------------- 9. two engines, sliced submissions
def test_two_engines_on_one_gpu():
    r = child("replicas")
    assert r["engines"] == 2
    assert r["ref"] == [True, False] and r["cold"] is True and r["warm"] == [True, False]
    # both engines looked the batch's messages up in their own table: all misses, then all hits
    assert r["stats_cold"]["misses"] == r["stats_cold"]["published"] == r["distinct"]
    assert r["stats_warm"]["hits"] == 2 * r["distinct"] and r["stats_warm"]["misses"] == 0
    assert r["small"] == [True, True, True, True] and r["entries"] >= r["distinct"]


def test_sliced_submission_bypasses_the_cache():
    r = child("sliced")
    assert r["ref"] == [True, False] and r["got"] == r["ref"]
    assert r["stats"]["bypassed"] == 2 * r["n"] and r["stats"]["published"] == 0 and r["stats"]["lookups"] == 0
    assert r["load_store_calls"] == [0, 0]
