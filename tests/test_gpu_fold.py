"""Verified folds on the GPU (include/grandine_bls_gpu_fold.h): gbls_verify_each_fold, the each-call
which also sums, per group of its own sets, the signatures that passed.

Expected values never come from the call under test.  Verdicts come from the C oracle's ref_verify
(with the signature statuses of gbls_g2_decompress and the key statuses of the spans key call, as in
tests/test_gpu_each.py); a sum is the Python oracle's aggregate_signatures over exactly the
occurrences whose set ref_verify accepts, compared byte for byte as affine Montgomery limbs, and its
compression is the oracle's g2_compress.  At the larger sizes the sums are also compared with
gbls_g2_decompress + gbls_g2_aggregate_segments over the host-filtered list: the three-submission
path the fold replaces.

The environment is that of tests/test_gpu_spans.py, which loads its own registry (600 keys and, at
index 600, the key of the secret r - s of key 5: two VALID sets then carry a signature and its
negation over one message) and its committee table; its helpers and those of tests/test_gpu_each.py
are imported."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_spans as S  # noqa: E402
import test_gpu_each as T  # noqa: E402
from test_gpu_spans import E, F, G, L, REF  # noqa: E402,F401  (fixtures)
from test_gpu_each import RV  # noqa: E402,F401  (fixture)

from oracle import bls12_381 as O  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = S.ROOT
Span = S.Span
INF_BYTES = bytes([0xC0]) + bytes(95)
NOT_IN_G2 = next(bytes.fromhex(c["in"]) for c in json.load(open(os.path.join(
    ROOT, "tests", "golden", "g2_decode.json")))["cases"] if c["status"] == 0 and not c["in_group"])


def row_min():
    txt = open(os.path.join(ROOT, "grandine_amd", "csrc", "gbls_common.h")).read()
    return int(re.search(r"constexpr uint32_t kRowAggregateMinSegs = (\d+);", txt).group(1))


def mont(a):
    return (a * (1 << 384) % O.P).to_bytes(48, "little")


def raw(pt):
    if pt is None:
        return bytes(192)
    (x0, x1), (y0, y1) = pt
    return mont(x0) + mont(x1) + mont(y0) + mont(y1)


def ints(a, n):
    return [a[i] for i in range(n)]


def fold(G, L, msgs, comp, sets, groups, with_bytes=True, fill=77):
    """The call under test.  Every output starts at a marker value."""
    n, nfold = len(sets), len(groups)
    st, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
    for i in range(n):
        st[i] = kst[i] = v[i] = fill
    fset, foff = S.flat(groups)
    out = ctypes.create_string_buffer(b"\xee" * (192 * max(nfold, 1)), 192 * max(nfold, 1))
    fb = ctypes.create_string_buffer(b"\xee" * (96 * max(nfold, 1)), 96 * max(nfold, 1))
    cnt = G.u32_array([0xEEEEEEEE] * nfold)
    rc = L.gbls_verify_each_fold(msgs, comp, *S.spans_args(G, sets), n, G.u32_array(fset or [0]), G.u32_array(foff), nfold,
                                 st, kst, v, out, fb if with_bytes else None, cnt)
    return (rc, L.gbls_last_error(), ints(st, n), ints(kst, n), ints(v, n),
            [out.raw[192 * g:192 * g + 192] for g in range(nfold)], ints(cnt, nfold),
            [fb.raw[96 * g:96 * g + 96] for g in range(nfold)])


class Oracle:
    """ref_verify per distinct (signature, message, key) and the Python oracle's decoding per distinct
    signature, each computed once and shared by the tests."""

    def __init__(self, RV):
        self.RV, self.verdict, self.point = RV, {}, {}

    def verify(self, pt192, msg, key96):
        k = (pt192, msg, key96)
        if k not in self.verdict:
            self.verdict[k] = bool(self.RV.ref_verify(pt192, msg, 32, key96))
        return self.verdict[k]

    def decode(self, comp96):
        if comp96 not in self.point:
            status, pt = O.g2_decompress(comp96)
            assert status == 0
            self.point[comp96] = pt
        return self.point[comp96]


@pytest.fixture(scope="module")
def ORC(RV):
    return Oracle(RV)


def expected(G, L, ORC, msgs, comp, sets, keys, groups):
    """(sig statuses, key statuses, verdicts, per group (point bytes, count, compressed bytes))."""
    n = len(sets)
    want_sst, pts = T.decode(G, L, comp)
    want_kst = S.span_keys(G, L, sets)[1]
    want_v = [G.SUCCESS if want_sst[i] == 0 and want_kst[i] == 0 and
              ORC.verify(pts[i], msgs[32 * i:32 * i + 32], keys[i]) else G.VERIFY_FAIL for i in range(n)]
    folds = []
    for g in groups:
        members = [s for s in g if want_v[s] == G.SUCCESS]
        total = O.aggregate_signatures([ORC.decode(comp[96 * s:96 * s + 96]) for s in members])
        folds.append((raw(total), len(members), INF_BYTES if total is None else O.g2_compress(total)))
    return want_sst, want_kst, want_v, folds


def check(G, L, ORC, msgs, comp, sets, keys, groups, with_bytes=True):
    want_sst, want_kst, want_v, folds = expected(G, L, ORC, msgs, comp, sets, keys, groups)
    rc, err, sst, kst, v, out, cnt, fb = fold(G, L, msgs, comp, sets, groups, with_bytes)
    assert (rc, err) == (G.SUCCESS, 0)
    assert (sst, kst, v) == (want_sst, want_kst, want_v)
    for g, (point, count, comp96) in enumerate(folds):
        assert cnt[g] == count, g
        assert out[g] == point, g
        assert fb[g] == (comp96 if with_bytes else b"\xee" * 96), g
    return want_v, folds


def three_submissions(G, L, comp, verdicts, groups):
    """Today's path: the host filters the verdicts, gbls_g2_decompress of the passing signatures, then
    gbls_g2_aggregate_segments (an empty segment is not sent)."""
    lists = [[s for s in g if verdicts[s] == G.SUCCESS] for g in groups]
    sent = [k for k, l in enumerate(lists) if l]
    flat = [s for k in sent for s in lists[k]]
    if not flat:
        return [bytes(192)] * len(groups)
    dec = ctypes.create_string_buffer(192 * len(flat))
    st = G.i32_array(len(flat))
    G.check(L.gbls_g2_decompress(b"".join(comp[96 * s:96 * s + 96] for s in flat), len(flat), dec, st), "decompress")
    off = [0]
    for k in sent:
        off.append(off[-1] + len(lists[k]))
    out, ast = ctypes.create_string_buffer(192 * len(sent)), G.i32_array(len(sent))
    G.check(L.gbls_g2_aggregate_segments(dec, G.u32_array(off), len(sent), out, ast), "aggregate")
    sums = [bytes(192)] * len(groups)
    for j, k in enumerate(sent):
        sums[k] = out.raw[192 * j:192 * j + 192]
    return sums


# ---------------------------------------------------------------- the 133-set environment with planted failures
PLANTED = {"flipped-bit": 10, "swapped-message": 23, "undecodable": 30, "bad-index": 44, "empty-plain": 58,
           "infinite-key": 72, "not-in-g2": 93}
SIGMA, MINUS_SIGMA = 100, 101


class Env133:
    pass


@pytest.fixture(scope="module")
def env(G, L, F, RV, E):
    e = Env133()
    sets = S.key_sets(E)
    assert len(sets) == 133
    # two valid sets over ONE message: validator 5 and the validator whose secret is r - s
    sets[SIGMA], sets[MINUS_SIGMA] = Span(E, plain=[5]), Span(E, plain=[S.NEG5])
    msgs = bytearray(F.messages(133, b"fold/sets"))
    msgs[32 * MINUS_SIGMA:32 * MINUS_SIGMA + 32] = msgs[32 * SIGMA:32 * SIGMA + 32]
    msgs = bytes(msgs)
    sigs = F.sign([sum(E.sks[v] for v in s.part) % F.R_ORDER or 1 for s in sets], msgs)
    comp = bytearray(S.compress(G, L, sigs))
    p = PLANTED
    comp[96 * p["flipped-bit"] + 95] ^= 0x01
    comp[96 * p["undecodable"]] &= 0x7F
    comp[96 * p["not-in-g2"]:96 * p["not-in-g2"] + 96] = NOT_IN_G2
    m = bytearray(msgs)
    m[32 * p["swapped-message"]:32 * p["swapped-message"] + 32] = msgs[32 * 24:32 * 25]
    sets[p["bad-index"]] = Span(E, plain=[S.NREG + 100])
    sets[p["empty-plain"]] = Span(E, plain=[])
    sets[p["infinite-key"]] = Span(E, plain=[5, S.NEG5])
    e.sets, e.msgs, e.comp = sets, bytes(m), bytes(comp)
    e.keys = [S.oracle_key(RV, E, F, s.part if i != p["bad-index"] else []) for i, s in enumerate(sets)]
    e.bad = sorted(p.values())
    return e


def test_planted_failures_are_in_no_sum(G, L, ORC, env):
    e, p = env, PLANTED
    good = [i for i in range(133) if i not in e.bad]
    groups = [list(range(133)),                                     # everything
              list(e.bad),                                          # only failing sets
              [SIGMA, MINUS_SIGMA],                                 # a signature with its negation
              [9, 10, 11], [29, 30, 31, 30], [92, 93, 94],          # a failing set between passing ones, one named twice
              [p["bad-index"]], [p["empty-plain"], 57], [p["infinite-key"], 71, 73], [p["swapped-message"], 22, 24],
              good[:17] + [SIGMA, SIGMA, MINUS_SIGMA],              # cancels down to one sigma more
              []]
    want_v, folds = check(G, L, ORC, e.msgs, e.comp, e.sets, e.keys, groups)
    assert [i for i in range(133) if want_v[i] != G.SUCCESS] == e.bad       # the oracle rejects exactly the planted sets
    assert folds[0][1] == 133 - len(e.bad)
    assert folds[1] == (bytes(192), 0, INF_BYTES)                             # count 0 says that nothing passed
    assert folds[2] == (bytes(192), 2, INF_BYTES)                             # infinity with its true count
    assert [f[1] for f in folds[3:10]] == [2, 2, 2, 0, 1, 2, 2]
    assert folds[10][1] == 20 and folds[11] == (bytes(192), 0, INF_BYTES)
    # against today's three submissions
    rc, err, sst, kst, v, out, cnt, fb = fold(G, L, e.msgs, e.comp, e.sets, groups)
    assert out == three_submissions(G, L, e.comp, want_v, groups)
    # no bytes asked for: the same points and counts, nothing written to a bytes array
    check(G, L, ORC, e.msgs, e.comp, e.sets, e.keys, groups[:4], with_bytes=False)


SHAPES = [[], [10], [11, 12], list(range(16)), list(range(8, 25)), list(range(65)), [3, 3, 4]]


@pytest.mark.parametrize("n", S.LAUNCHES)  # 1, 3, 64, 65
def test_sizes_and_both_kernel_forms(G, L, ORC, env, n):
    e = env
    assert row_min() == 128
    sets, msgs, comp, keys = e.sets[:n], e.msgs[:32 * n], e.comp[:96 * n], e.keys[:n]
    check(G, L, ORC, msgs, comp, sets, keys, [list(range(n))])              # one group of all sets
    for nfold in (len(SHAPES), row_min() - 1, row_min(), row_min() + 2):    # the workgroup form, the switch, rows
        groups = [[(s + 5 * (k // len(SHAPES))) % n for s in SHAPES[k % len(SHAPES)]] for k in range(nfold)]
        assert {len(g) for g in groups} == {0, 1, 2, 16, 17, 65, 3}
        want_v, folds = check(G, L, ORC, msgs, comp, sets, keys, groups)
        if n >= 64 and nfold in (len(SHAPES), row_min()):
            rc, err, sst, kst, v, out, cnt, fb = fold(G, L, msgs, comp, sets, groups)
            assert out == three_submissions(G, L, comp, want_v, groups)


def test_thousands_of_groups_take_the_row_form_without_the_simd_claim(G, L, ORC, env):
    """From 513 blocks of 64 lanes on (more than 2048 groups, what a merged gossip load can reach) the
    row form runs without claiming its SIMDs.  Sets 9, 10 and 11 (10 is the flipped bit), 2052 groups
    cycling five shapes, each shape's sum from the oracle."""
    e = env
    sets, msgs, comp, keys = e.sets[9:12], e.msgs[32 * 9:32 * 12], e.comp[96 * 9:96 * 12], e.keys[9:12]
    shapes = [[0], [1, 2], [], [2, 2, 0], [0, 1, 2, 1]]
    want_sst, want_kst, want_v, folds = expected(G, L, ORC, msgs, comp, sets, keys, shapes)
    assert want_v == [G.SUCCESS, G.VERIFY_FAIL, G.SUCCESS] and [f[1] for f in folds] == [1, 1, 0, 3, 2]
    txt = open(os.path.join(ROOT, "grandine_amd", "csrc", "bls_w4.h")).read()
    max_waves = int(re.search(r"constexpr uint32_t kExclusiveMaxWaves = (\d+);", txt).group(1))
    nfold = 4 * max_waves + 4
    assert (16 * nfold + 63) // 64 > max_waves and nfold >= row_min()
    groups = [shapes[k % len(shapes)] for k in range(nfold)]
    rc, err, sst, kst, v, out, cnt, fb = fold(G, L, msgs, comp, sets, groups)
    assert (rc, err, sst, kst, v) == (G.SUCCESS, 0, want_sst, want_kst, want_v)
    for g in range(nfold):
        assert (out[g], cnt[g], fb[g]) == folds[g % len(shapes)], g


def test_no_groups_is_the_each_call(G, L, env):
    e = env
    want = T.each(G, L, e.msgs, e.comp, e.sets)
    assert want[0] == G.SUCCESS and [i for i in range(133) if want[4][i] != G.SUCCESS] == e.bad
    got = fold(G, L, e.msgs, e.comp, e.sets, [])
    assert got[:5] == want and got[5:] == ([], [], [])
    # NULL group arrays are fine without groups
    n = 133
    st, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
    rc = L.gbls_verify_each_fold(e.msgs, e.comp, *S.spans_args(G, e.sets), n, None, None, 0, st, kst, v, None, None, None)
    assert (rc, L.gbls_last_error(), ints(st, n), ints(kst, n), ints(v, n)) == want
    # and the fold stage ran in no such call
    names = [L.gbls_stage_name(k).decode() for k in range(32) if L.gbls_stage_name(k)]
    assert "k_g2_fold" in names
    stage = names.index("k_g2_fold")
    calls = (ctypes.c_uint32 * 32)()
    L.gbls_profile(1)
    try:
        L.gbls_profile_reset()
        fold(G, L, e.msgs, e.comp, e.sets, [])
        L.gbls_profile_read(None, calls, 32)
        assert calls[stage] == 0
        L.gbls_profile_reset()
        fold(G, L, e.msgs, e.comp, e.sets, [[0, 1]])
        L.gbls_profile_read(None, calls, 32)
        assert calls[stage] == 1
    finally:
        L.gbls_profile(0)


def test_message_line_cache_serving_checks(G, L, ORC, env):
    e = env
    groups = [list(range(133)), [SIGMA, MINUS_SIGMA], list(e.bad), [9, 10, 11]]
    plain = fold(G, L, e.msgs, e.comp, e.sets, groups)
    assert plain[0] == G.SUCCESS
    out = (ctypes.c_uint64 * 8)()
    assert L.gbls_msgcache_configure(256) == 0
    prev = L.gbls_msgcache_serve_checks(1)
    try:
        assert L.gbls_msgcache_stats(out) == 0
        hits0 = out[1]
        assert fold(G, L, e.msgs, e.comp, e.sets, groups) == plain   # cold
        assert fold(G, L, e.msgs, e.comp, e.sets, groups) == plain   # warm
        assert L.gbls_msgcache_stats(out) == 0 and out[1] > hits0
    finally:
        L.gbls_msgcache_serve_checks(prev)
        assert L.gbls_msgcache_configure(0) == 0
    check(G, L, ORC, e.msgs, e.comp, e.sets, e.keys, groups)


# ---------------------------------------------------------------- the grouped regime
def test_grouped_regime_with_and_without_per_check(G, L, F, ORC, RV, E):
    """2050 single-key checks over four messages, 1 % planted bad sets; one group per message and
    one of all.  The checks are drawn from 16 validators x 4 messages, so that ref_verify decides
    every one of them (each distinct check once)."""
    n, nval = 2050, 16
    um = F.messages(4, b"fold/grouped")
    vals = [(31 * j + 7) % S.NREG for j in range(nval)]
    usig = S.compress(G, L, F.sign([E.sks[v] for v in vals for _ in range(4)], um * nval))   # [validator][message]
    rng = random.Random("fold/grouped")
    pick = [(rng.randrange(nval), i % 4) for i in range(n)]
    sets = [Span(E, plain=[vals[j]]) for j, _ in pick]
    msgs = b"".join(um[32 * m:32 * m + 32] for _, m in pick)
    comp = bytearray(b"".join(usig[96 * (4 * j + m):96 * (4 * j + m) + 96] for j, m in pick))
    bad = sorted(rng.sample(range(n), 20)) + [n - 1]
    for i in bad:                                           # another validator's valid signature of the message
        j, m = pick[i]
        k = 4 * ((j + 1) % nval) + m
        comp[96 * i:96 * i + 96] = usig[96 * k:96 * k + 96]
    comp = bytes(comp)
    key_of = {}
    for j in range(nval):
        key_of[j] = S.oracle_key(RV, E, F, [vals[j]])
    keys = [key_of[j] for j, _ in pick]
    groups = [[i for i in range(n) if pick[i][1] == m] for m in range(4)] + [list(range(n))]
    decided = len(ORC.verdict)
    prev = L.gbls_set_policy(0)
    try:
        L.gbls_set_policy(prev & ~G.INIT_PER_CHECK)
        want_v, folds = check(G, L, ORC, msgs, comp, sets, keys, groups)
        assert [i for i in range(n) if want_v[i] != G.SUCCESS] == sorted(set(bad))
        assert folds[4][1] == n - len(set(bad)) and sum(f[1] for f in folds[:4]) == folds[4][1]
        grouped = fold(G, L, msgs, comp, sets, groups)
        assert grouped[5] == three_submissions(G, L, comp, want_v, groups)
        L.gbls_set_policy(prev | G.INIT_PER_CHECK)
        assert fold(G, L, msgs, comp, sets, groups) == grouped
    finally:
        L.gbls_set_policy(prev)
    assert len(ORC.verdict) - decided <= 64 + 21            # (every check was decided by ref_verify, few of them distinct)


# ---------------------------------------------------------------- argument errors
def test_argument_errors_leave_the_pre_fill(G, L, env):
    e = env
    n = 5
    sets, msgs, comp = e.sets[:n], e.msgs[:32 * n], e.comp[:96 * n]
    args = S.spans_args(G, sets)

    def call(fset, foff, nfold, out=True, cnt=True, kst=True):
        st, ks, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
        for i in range(n):
            st[i] = ks[i] = v[i] = 77
        o = ctypes.create_string_buffer(b"\xee" * (192 * 3), 192 * 3)
        fb = ctypes.create_string_buffer(b"\xee" * (96 * 3), 96 * 3)
        c = G.u32_array([0xEEEEEEEE] * 3)
        rc = L.gbls_verify_each_fold(msgs, comp, *args, n, fset, foff, nfold, st, ks if kst else None, v, o if out else None,
                                     fb, c if cnt else None)
        return (rc, L.gbls_last_error(), ints(st, n), ints(ks, n), ints(v, n), o.raw, ints(c, 3), fb.raw)

    k = 3
    pre = (G.VERIFY_FAIL, 102, [G.BAD_ENCODING] * n, [G.BAD_ENCODING] * n, [G.VERIFY_FAIL] * n, bytes(192 * k), [0] * k,
           INF_BYTES * k)
    fset, foff = G.u32_array([0, 1, 4, 2, 2]), G.u32_array([0, 2, 2, 5])
    assert call(None, foff, k) == pre                                          # fold_set NULL
    assert call(fset, None, k) == pre                                          # fold_off NULL
    got = call(fset, foff, k, out=False)                                       # fold_out NULL
    assert got[:5] == pre[:5] and got[6:] == pre[6:] and got[5] == b"\xee" * (192 * k)
    got = call(fset, foff, k, cnt=False)                                       # fold_count NULL
    assert got[:6] == pre[:6] and got[7] == pre[7] and got[6] == [0xEEEEEEEE] * k
    assert call(fset, G.u32_array([1, 2, 2, 5]), k) == pre                     # fold_off[0] != 0
    assert call(fset, G.u32_array([0, 3, 2, 5]), k) == pre                     # decreasing
    assert call(G.u32_array([0, 1, 5, 2, 2]), foff, k) == pre                  # an entry == n
    assert call(G.u32_array([0, 1, 0xFFFFFFFF, 2, 2]), foff, k) == pre
    got = call(fset, foff, k, kst=False)                                       # an each-call error: the fold's pre-fill too
    assert got[:3] == pre[:3] and got[4:] == pre[4:]
    if ctypes.sizeof(ctypes.c_size_t) > 4:                                     # a group count past 32 bits: nothing is touched
        got = call(fset, foff, 1 << 32)
        assert got[:5] == pre[:5] and got[5] == b"\xee" * (192 * k) and got[6] == [0xEEEEEEEE] * k
    ok = call(fset, foff, k)                                                   # a following good call succeeds
    assert ok[:2] == (G.SUCCESS, 0) and ok[6] == [2, 0, 3] and ok[4] == [G.SUCCESS] * n


# ---------------------------------------------------------------- concurrent callers, two engines
def child(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_fold_child.py")] + list(args),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_concurrent_callers_subprocess():
    res = child("threads")
    assert res["solo_ok"] == [True] * 8                     # every solo run against gbls_g2_aggregate_segments
    assert res["errors"] == [] and res["exact"] == [res["calls"]] * res["threads"] == [20] * 8


def test_two_engines_subprocess():
    one, two = child("single"), child("replicas")
    assert (one["engines"], two["engines"]) == (1, 2)
    assert one["rc"] == two["rc"] == [0, 0]
    assert one["failing"] == two["failing"] == one["want_failing"]
    assert one["counts"] == two["counts"] == one["want_counts"]
    assert one["sums"] == two["sums"] == one["three_submissions"] == two["three_submissions"]
    assert one["bytes"] == two["bytes"]


# ---------------------------------------------------------------- the Python mirror
def test_python_mirror_on_the_gpu(G, L, F, ORC, RV, E):
    from grandine_amd import bls as B
    from grandine_amd import pools as P
    from grandine_amd import verifier as V
    keys48 = [E.comp[48 * i:48 * i + 48] for i in range(S.NREG + 1)]
    B.Registry.forget()
    try:
        B.Registry.mirror_finalized(keys48)  # first = 0 rewrites the registry: the committee table is cleared
        rng = random.Random("fold/mirror")
        size = 40
        committee = [(13 * j + 3) % S.NREG for j in range(size)]
        msg = F.messages(1, b"fold/mirror")
        comp = S.compress(G, L, F.sign([E.sks[v] for v in committee], msg * size))
        sig = [comp[96 * j:96 * j + 96] for j in range(size)]
        bits = [rng.random() < 0.3 for _ in range(size)]
        positions = rng.sample(range(size), 24)
        for k in (2, 9, 17):
            bits[positions[k]] = False                         # (the singles planted below are candidates)
        start = O.aggregate_signatures([ORC.decode(sig[j]) for j in range(size) if bits[j]])
        singles = [(pos, msg, sig[pos], committee[pos]) for pos in positions]
        for k in (2, 9, 17):                                   # another attester's signature: does not verify
            pos = singles[k][0]
            singles[k] = (pos, msg, sig[(pos + 1) % size], committee[pos])
        singles.insert(12, (singles[2][0], msg, sig[singles[2][0]], committee[singles[2][0]]))   # a later, valid single of position 2's
        pts = T.decode(G, L, b"".join(s[2] for s in singles))[1]
        ok = [ORC.verify(pts[k], msg, S.oracle_key(RV, E, F, [s[3]])) for k, s in enumerate(singles)]
        assert [k for k, x in enumerate(ok) if not x] == [2, 9, 18]
        # the reference loop over the singles the oracle accepts, first per position
        want_bits, want_sig, seen = list(bits), start, set()
        deferred_want = []
        for k, (pos, _, s, _) in enumerate(singles):
            if bits[pos]:
                continue
            if pos in seen:
                deferred_want.append(k)
                continue
            seen.add(pos)
            if ok[k]:
                want_bits[pos] = True
                want_sig = O.g2_add(want_sig, ORC.decode(s))
        agg = P.Aggregate(size, B.Signature(raw(start)), bits)
        verified, deferred = P.fold_verified_singles(agg, singles)
        assert deferred == deferred_want == [12]
        assert [k for k, x in enumerate(verified) if x is not None] == [k for k, s in enumerate(singles)
                                                                        if not bits[s[0]] and k != 12]
        assert all(verified[k] == ok[k] for k in range(len(singles)) if verified[k] is not None)
        assert agg.bits == want_bits and agg.signature.raw == raw(want_sig)
        # the deferred single's position is still missing: it is a candidate now, and verifies
        pos = singles[12][0]
        assert not agg.bits[pos]
        verified, deferred = P.fold_verified_singles(agg, [singles[12]])
        assert (verified, deferred) == ([True], []) and agg.bits[pos]
        assert agg.signature.raw == raw(O.g2_add(want_sig, ORC.decode(singles[12][2])))
        # MultiVerifier.verify_each_fold: the path, the verdicts, the sums
        mv = V.MultiVerifier()
        for _, m, s, index in singles:
            mv.verify_aggregate_indexed(m, s, [index], (), None)
        groups = [list(range(len(singles))), [2, 9, 18], [0, 0, 1]]
        oks, folds = mv.verify_each_fold(groups)
        assert oks == ok and mv.last_each_path == "fold"
        for g, (total, count, comp96) in zip(groups, folds):
            members = [k for k in g if ok[k]]
            want = O.aggregate_signatures([ORC.decode(singles[k][2]) for k in members])
            assert count == len(members) and total.raw == raw(want)
            assert bytes(comp96) == (INF_BYTES if want is None else O.g2_compress(want))
    finally:
        B.Registry.forget()
        S.load_all(G, L, F)
