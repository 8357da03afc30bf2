"""Local key sets on the GPU (include/grandine_bls_gpu_local.h): compressed public keys decoded
inside the submission.  gbls_g1_aggregate_local, gbls_verify_each_local and gbls_verify_items_local
against gbls_g1_decompress(validate = 1) (the decoding), the C oracle (ref_sk_to_pk over summed
secret keys, ref_verify, ref_multi_verify) and the engine's earlier calls over decoded points
(gbls_g1_aggregate_segments, gbls_verify_batch_compressed, gbls_multi_verify_segments, the span
calls for everything that is not local).  The calls under test are never a yardstick; every
comparison is byte for byte or verdict for verdict.

The environment is that of tests/test_gpu_spans.py and tests/test_gpu_each.py; their helpers and
fixtures are imported.  The local keys are 40 keys of known secret keys, the negation of one of
them, and every entry of tests/golden/g1_decode.json.  Tables up to kLocalWaveMax keys are decoded
one wave per key, larger ones one lane per key; both forms are crossed below."""
import ctypes
import json
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_each as T  # noqa: E402
import test_gpu_spans as S  # noqa: E402
from test_gpu_each import PK, RV  # noqa: E402,F401  (fixtures)
from test_gpu_spans import E, F, G, L, REF  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu

ROOT = S.ROOT
u64, flat, ints = S.u64, S.flat, T.ints
NKEYS = 40
LOCAL = 0xFFFFFFFE


def wave_max():
    txt = open(os.path.join(ROOT, "grandine_amd", "csrc", "gbls_local.h")).read()
    return int(re.search(r"constexpr uint32_t kLocalWaveMax = (\d+);", txt).group(1))


class Loc:
    """A local set: positions into the call's key table."""

    def __init__(self, positions):
        self.base, self.named, self.per, self.bitlist = LOCAL, [], [], True
        self.mask, self.field, self.lst, self.part = bytes(8), b"", list(positions), []


def is_local(s):
    return s.base == LOCAL


class Keys:
    pass


@pytest.fixture(scope="module")
def K(G, L, F):
    """The local key material: 40 valid keys, the negation of key 3, a valid key with its sign flag
    flipped, and the golden decode cases; decoded once by gbls_g1_decompress(validate = 1)."""
    k = Keys()
    k.sks, comp = F.registry(NKEYS, seed=b"local")
    k.valid = [comp[48 * i:48 * i + 48] for i in range(NKEYS)]
    k.neg3 = F.compress_g1(F.public_keys([F.R_ORDER - k.sks[3]]))
    flipped = bytearray(k.valid[7])
    flipped[0] ^= 0x20
    k.flipped = bytes(flipped)
    assert k.flipped == F.compress_g1(F.public_keys([F.R_ORDER - k.sks[7]]))
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "g1_decode.json")))["cases"]
    k.golden = [bytes.fromhex(c["in"]) for c in cases]
    k.golden_status = [c["validate_status"] for c in cases]
    k.inputs = k.golden + k.valid + [k.flipped]
    k.status, k.points = decompress(G, L, k.inputs)
    assert k.status[:len(cases)] == k.golden_status and not any(k.status[len(cases):])
    k.by_status = {s: k.inputs[k.status.index(s)] for s in (G.BAD_ENCODING, 2, 3, 6)}
    return k


def decompress(G, L, keys):
    """The yardstick of the decoding: gbls_g1_decompress(validate = 1), statuses and points."""
    n = len(keys)
    out, st = ctypes.create_string_buffer(96 * n), G.i32_array(n)
    G.check(L.gbls_g1_decompress(G.buf(b"".join(keys)), n, 1, out, st), "decompress")
    return ints(st, n), [out.raw[96 * i:96 * i + 96] for i in range(n)]


def table_args(G, table):
    return (G.buf(b"".join(table)) if table else None), len(table)


def marked(G, n, fill=77):
    a = G.i32_array(n)
    for i in range(n):
        a[i] = fill
    return a


def local_keys(G, L, sets, table, expect_rc=0, null_pst=False):
    n, t = len(sets), len(table)
    out = ctypes.create_string_buffer(b"\xff" * (96 * n), 96 * n)
    st, pst = marked(G, n), marked(G, t)
    rc = L.gbls_g1_aggregate_local(*S.spans_args(G, sets), *table_args(G, table), n, out, st, None if null_pst else pst)
    assert rc == expect_rc, (rc, L.gbls_last_error())
    return [out.raw[96 * i:96 * i + 96] for i in range(n)], ints(st, n), ints(pst, t)


def each_local(G, L, msgs, comp, sets, table, fill=77):
    n, t = len(sets), len(table)
    st, kst, v, pst = marked(G, n, fill), marked(G, n, fill), marked(G, n, fill), marked(G, t, fill)
    rc = L.gbls_verify_each_local(msgs, comp, *S.spans_args(G, sets), *table_args(G, table), n, st, kst, v, pst)
    return rc, L.gbls_last_error(), ints(st, n), ints(kst, n), ints(v, n), ints(pst, t)


def items_local(G, L, msgs, comp, sets, table, rands, seg, flags=0, fill=77):
    n, nseg, t = len(sets), len(seg) - 1, len(table)
    st, kst, v, pst = marked(G, n, fill), marked(G, n, fill), marked(G, nseg, fill), marked(G, t, fill)
    rc = L.gbls_verify_items_local(msgs, comp, *S.spans_args(G, sets), *table_args(G, table), u64(rands), n,
                                   G.u32_array(seg), nseg, st, kst, v, pst, flags)
    return rc, L.gbls_last_error(), ints(st, n), ints(kst, n), ints(v, nseg), ints(pst, t)


def ref_pk(REF, F, sk):
    sk %= F.R_ORDER
    if sk == 0:
        return bytes(96)
    out = ctypes.create_string_buffer(96)
    REF.ref_sk_to_pk(sk.to_bytes(32, "big"), out)
    return out.raw


# ---------------------------------------------------------------- 1. decode parity
def test_decode_parity_in_both_forms(G, L, K):
    assert set(K.status) == {0, G.BAD_ENCODING, 2, 3, 6}   # every nonzero status occurs (2: not on curve, 3: not in
    m = len(K.inputs)                                       # group, 6: infinity)
    W = wave_max()
    assert W >= 65
    for size in (1, 3, 16, 17, 64, 65, W, W + 1):
        table = [K.inputs[(size + j) % m] for j in range(size)]   # cyclic, every size from another start
        want_st = [K.status[(size + j) % m] for j in range(size)]
        want_pt = [K.points[(size + j) % m] for j in range(size)]
        keys, st, pst = local_keys(G, L, [Loc([j]) for j in range(size)], table)
        assert pst == want_st, size
        assert keys == want_pt, size                              # an invalid key: all-zero in both
        assert st == [G.BAD_ENCODING if s else 0 for s in want_st], size
    # every input went through both forms
    assert m <= 64 and m <= W + 1


def test_table_without_sets_and_null_status(G, L, K):
    table = K.inputs[:20]
    assert local_keys(G, L, [], table) == ([], [], K.status[:20])
    keys, st, pst = local_keys(G, L, [Loc([14])], table, null_pst=True)
    assert (keys, st) == ([K.points[14]], [0]) and pst == [77] * 20   # NULL: nothing written anywhere


# ---------------------------------------------------------------- 2. sums
class Sums:
    pass


@pytest.fixture(scope="module")
def SUMS(G, K):
    s = Sums()
    s.table = K.valid + [K.neg3, K.by_status[3], K.flipped]
    NEG3, BAD, s.npkb = NKEYS, NKEYS + 1, NKEYS + 3
    s.sk = K.sks + [-K.sks[3], None, -K.sks[7]]
    s.lists = [[], [0], [1, 2], [(5 * j) % NKEYS for j in range(17)], [(7 * j + 1) % NKEYS for j in range(300)],
               [4, 4], [3, NEG3], [s.npkb], [5], [0, BAD, 1], [5], [5, 6], [NKEYS + 2, 7, 9], [2, 0xFFFFFFFF],
               [7, NKEYS + 2]]
    s.status = [G.AGGR_TYPE_MISMATCH, 0, 0, 0, 0, 0, 0, G.BAD_ENCODING, 0, G.BAD_ENCODING, 0, 0, 0, G.BAD_ENCODING, 0]
    return s


def sum_key(REF, F, SUMS, lst, status):
    return ref_pk(REF, F, sum(SUMS.sk[p] for p in lst)) if status == 0 and lst else bytes(96)


def test_sums_of_local_keys(G, L, F, REF, K, SUMS):
    sets = [Loc(lst) for lst in SUMS.lists]
    n = len(sets)
    want_pst, pts = decompress(G, L, SUMS.table)
    assert want_pst == [0] * (NKEYS + 1) + [3, 0]
    want = [sum_key(REF, F, SUMS, lst, st) for lst, st in zip(SUMS.lists, SUMS.status)]
    assert want[6] == bytes(96) and want[14] == bytes(96) and want[5] != want[1]   # cancels; doubles
    keys, st, pst = local_keys(G, L, sets, SUMS.table)
    assert pst == want_pst and st == SUMS.status and keys == want
    assert keys[8] == keys[10] == pts[5]                                           # one key shared by several sets
    # the same sums through gbls_g1_aggregate_segments over the decoded points
    ok = [i for i in range(n) if all(p < SUMS.npkb and want_pst[p] == 0 for p in SUMS.lists[i])]
    assert [i for i in range(n) if i not in ok] == [7, 9, 13]
    idx, off = flat([SUMS.lists[i] for i in ok])
    out, sst = ctypes.create_string_buffer(96 * len(ok)), G.i32_array(len(ok))
    G.check(L.gbls_g1_aggregate_segments(G.buf(b"".join(pts[p] for p in idx)), G.u32_array(off), len(ok), out, sst),
            "segments")
    assert [out.raw[96 * k:96 * k + 96] for k in range(len(ok))] == [keys[i] for i in ok]
    assert ints(sst, len(ok)) == [st[i] for i in ok]
    # the long list in the row form of the piece kernel and in the lane form: the same bytes alone and in company
    assert local_keys(G, L, [sets[4]], SUMS.table)[0] == [keys[4]]
    assert local_keys(G, L, [sets[2]], SUMS.table)[0] == [keys[2]]


# ---------------------------------------------------------------- 3. mixed calls
def mixed_sets(E, SUMS):
    """133 sets: two of the span environment's, then a local one, and so on."""
    spans, out, k = S.key_sets(E), [], 0
    while len(out) < sum(S.LAUNCHES):
        out.append(Loc(SUMS.lists[k % len(SUMS.lists)]) if len(out) % 3 == 2 else spans[len(out)])
        k += len(out) % 3 == 0
    return out


def test_mixed_calls(G, L, F, REF, E, K, SUMS):
    sets = mixed_sets(E, SUMS)
    assert len(sets) == 133 and sum(map(is_local, sets)) == 44 and any(s.base is None for s in sets)
    others = [s for s in sets if not is_local(s)]
    okeys, ost = S.span_keys(G, L, others)        # the span call over everything that is not local
    assert ost == [0] * len(others)
    want_k, want_s, it = [], [], iter(zip(okeys, ost))
    for s in sets:
        if is_local(s):
            st = SUMS.status[SUMS.lists.index(s.lst)]
            want_k.append(sum_key(REF, F, SUMS, s.lst, st))
            want_s.append(st)
        else:
            k, st = next(it)
            want_k.append(k)
            want_s.append(st)
    pos = 0
    for n in S.LAUNCHES:
        keys, st, pst = local_keys(G, L, sets[pos:pos + n], SUMS.table)
        assert st == want_s[pos:pos + n] and keys == want_k[pos:pos + n], n
        assert pst == [0] * (NKEYS + 1) + [3, 0]
        pos += n
    # without a table and without a local set: the span call itself
    assert local_keys(G, L, others[:20], [])[:2] == (okeys[:20], ost[:20])


# ---------------------------------------------------------------- 4. per-set verdicts
LOCAL_PLANTED = {"valid": 5, "bad-encoding": 15, "not-on-curve": 17, "not-in-group": 19, "infinity": 26,
                 "wrong-key": 35, "undecodable-sig": 37, "pair": 62, "position-past": 64}


def each_env(G, L, F, RV, E, K):
    sets, signing, planted = T.each_sets(E)
    assert not set(LOCAL_PLANTED.values()) & set(planted.values())
    table = K.valid + [K.by_status[G.BAD_ENCODING], K.by_status[2], K.by_status[3], K.by_status[6]]
    lists = {"valid": [11], "bad-encoding": [NKEYS], "not-on-curve": [NKEYS + 1], "not-in-group": [NKEYS + 2],
             "infinity": [NKEYS + 3], "wrong-key": [12], "undecodable-sig": [13], "pair": [20, 21],
             "position-past": [len(table)]}
    sks = [sum(E.sks[v] for v in s.part) % F.R_ORDER or 1 for s in signing]
    key_sk = [None] * len(sets)        # the secret key behind a local set's key (None: no valid key)
    for name, i in LOCAL_PLANTED.items():
        sets[i] = Loc(lists[name])
        valid = all(p < NKEYS for p in lists[name])
        key_sk[i] = sum(K.sks[p] for p in lists[name]) if valid else None
        sks[i] = key_sk[i] if valid else 1
    sks[LOCAL_PLANTED["wrong-key"]] = K.sks[14]     # signed by another key
    msgs = F.messages(len(sets), b"local/sets")
    comp = S.compress(G, L, F.sign(sks, msgs))
    comp = T.clear_flag(T.swap(comp, planted["swap-a"], planted["swap-b"]), planted["undecodable"])
    comp = T.clear_flag(comp, LOCAL_PLANTED["undecodable-sig"])
    return sets, planted, table, key_sk, msgs, comp


def test_per_set_verdicts(G, L, F, RV, E, PK, K):
    sets, planted, table, key_sk, msgs, comp = each_env(G, L, F, RV, E, K)
    n = len(sets)
    want_pst, lpts = decompress(G, L, table)
    assert want_pst == [0] * NKEYS + [G.BAD_ENCODING, 2, 3, 6]
    want_sst, pts = T.decode(G, L, comp)
    others = [i for i in range(n) if not is_local(sets[i])]
    skst = dict(zip(others, S.span_keys(G, L, [sets[i] for i in others])[1]))
    want_kst = [skst[i] if i in skst else (0 if key_sk[i] is not None else G.BAD_ENCODING) for i in range(n)]
    okeys = [ref_pk(RV, F, key_sk[i] or 0) if is_local(sets[i]) else S.oracle_key(RV, E, F, sets[i].part) for i in range(n)]
    want_v = [G.SUCCESS if want_sst[i] == 0 and want_kst[i] == 0 and
              RV.ref_verify(pts[i], msgs[32 * i:32 * i + 32], 32, okeys[i]) else G.VERIFY_FAIL for i in range(n)]
    bad = set(planted.values()) | {LOCAL_PLANTED[k] for k in LOCAL_PLANTED if k not in ("valid", "pair")}
    assert [i for i in range(n) if want_v[i] != G.SUCCESS] == sorted(bad)
    assert want_v[LOCAL_PLANTED["valid"]] == want_v[LOCAL_PLANTED["pair"]] == G.SUCCESS
    # gbls_verify_batch_compressed over the decoded points agrees wherever a set has key points
    pidx, poff = flat([[("L", p) for p in s.lst if p < len(table)] if is_local(s) else [("R", v) for v in s.part]
                       for s in sets])
    pst_, pv_ = G.i32_array(n), G.i32_array(n)
    G.check(L.gbls_verify_batch_compressed(msgs, comp, b"".join(lpts[p] if t == "L" else PK[p] for t, p in pidx),
                                           G.u32_array(poff), n, pst_, pv_), "points")
    assert ints(pst_, n) == want_sst
    assert all(pv_[i] == want_v[i] for i in range(n) if want_kst[i] == 0)

    def check(order):
        rc, err, sst, kst, v, pst = each_local(G, L, b"".join(msgs[32 * i:32 * i + 32] for i in order),
                                               b"".join(comp[96 * i:96 * i + 96] for i in order),
                                               [sets[i] for i in order], table)
        assert (rc, err) == (G.SUCCESS, 0) and pst == want_pst
        assert sst == [want_sst[i] for i in order]
        assert kst == [want_kst[i] for i in order]
        assert v == [want_v[i] for i in order]
        for k, i in enumerate(order):
            if i in bad:   # every clean neighbour of a planted failure passes
                assert all(v[j] == G.SUCCESS for j in (k - 1, k + 1) if 0 <= j < len(order) and order[j] not in bad)

    pos = 0
    for m in S.LAUNCHES:
        check(list(range(pos, pos + m)))
        pos += m
    assert pos == n
    for m in (T.w4_max(), T.w4_max() + 1):
        check([i % n for i in range(m)])


def test_without_local_sets_each_equals_the_spans_call(G, L, F, RV, E):
    sets, signing, planted = T.each_sets(E)
    msgs, comp = T.signed(G, L, F, E, signing, b"each/sets")
    comp = T.clear_flag(T.swap(comp, planted["swap-a"], planted["swap-b"]), planted["undecodable"])
    want = T.each(G, L, msgs, comp, sets)
    assert want[0] == G.SUCCESS and set(want[4]) == {G.SUCCESS, G.VERIFY_FAIL}
    assert each_local(G, L, msgs, comp, sets, []) == want + ([],)


# ---------------------------------------------------------------- 5. items
class LItems:
    pass


@pytest.fixture(scope="module")
def local_items(G, L, F, RV, E, K):
    """The 14 sets and 6 items of tests/test_gpu_each.py, then three items with local sets: two
    valid ones (one key; a pair with a span set), and one whose second set names an invalid key."""
    base = T.make_items(G, L, F, RV, E)
    it = LItems()
    it.table = K.valid[:8] + [K.by_status[3]]
    extra = [Loc([0]), Loc([1, 2]), S.make_span(E, 20, [0, 1], random.Random("local/items")), Loc([3]), Loc([4]), Loc([8])]
    sk = [K.sks[0], K.sks[1] + K.sks[2], sum(E.sks[v] for v in extra[2].part), K.sks[3], K.sks[4], 1]
    it.sets = base.sets + extra
    it.seg = base.seg + [base.n + 1, base.n + 4, base.n + 6]
    it.n = len(it.sets)
    it.msgs = base.msgs + F.messages(6, b"local/items")
    it.sigs = base.sigs + F.sign([x % F.R_ORDER for x in sk], it.msgs[32 * base.n:])
    it.comp = S.compress(G, L, it.sigs)
    it.rands = base.rands + F.rands(6, 909)
    it.pks = base.pks + b"".join(ref_pk(RV, F, x) for x in sk[:5]) + bytes(96)
    it.want_kst = [0] * (it.n - 1) + [G.BAD_ENCODING]
    it.want_pst = [0] * 8 + [3]
    it.base = base
    return it


def test_items_against_the_oracle(G, L, RV, E, K, local_items):
    it = local_items
    nseg = len(it.seg) - 1
    zeros = [0] * it.n
    assert [b - a for a, b in zip(it.seg, it.seg[1:])] == [3, 3, 1, 2, 3, 2, 1, 3, 2] and decompress(G, L, it.table)[0] == it.want_pst
    # the oracle over the items whose keys are all valid; the last item holds an invalid key and fails alone
    want = T.ref_items(RV, it, seg=it.seg[:-1]) + [G.VERIFY_FAIL]
    assert want == [G.SUCCESS] * (nseg - 1) + [G.VERIFY_FAIL]
    for flags in (0, 1):   # 1: GBLS_CALL_BLOCK
        assert items_local(G, L, it.msgs, it.comp, it.sets, it.table, it.rands, it.seg, flags) == (
            G.SUCCESS, 0, zeros, it.want_kst, want, it.want_pst)
    # a swapped signature between two local items: both fail, nothing else does
    sw = bytearray(it.sigs)
    a, b = it.base.n, it.base.n + 3
    sw[192 * a:192 * a + 192], sw[192 * b:192 * b + 192] = it.sigs[192 * b:192 * b + 192], it.sigs[192 * a:192 * a + 192]
    want = T.ref_items(RV, it, sigs=bytes(sw), seg=it.seg[:-1]) + [G.VERIFY_FAIL]
    assert want == [G.SUCCESS] * 6 + [G.VERIFY_FAIL] * 3
    assert items_local(G, L, it.msgs, T.swap(it.comp, a, b), it.sets, it.table, it.rands, it.seg) == (
        G.SUCCESS, 0, zeros, it.want_kst, want, it.want_pst)


def test_empty_item_and_zero_scalar_as_the_segments_call(G, L, local_items):
    it = local_items
    # gbls_multi_verify_segments over the oracle's key points (an all-zero point for the invalid key)
    seg = it.seg[:7] + [it.seg[6]] + it.seg[7:] + [it.n]    # an empty item before the local ones and one at the end
    want = T.segments_points(G, L, it, it.rands, seg)
    assert want == [G.SUCCESS] * 6 + [G.VERIFY_FAIL] + [G.SUCCESS] * 2 + [G.VERIFY_FAIL] * 2
    assert items_local(G, L, it.msgs, it.comp, it.sets, it.table, it.rands, seg)[4] == want
    rands = list(it.rands)
    rands[it.base.n + 2] = 0                                  # a zero scalar in the item of three
    want = T.segments_points(G, L, it, rands, it.seg)
    assert want == [G.SUCCESS] * 7 + [G.VERIFY_FAIL] * 2
    assert items_local(G, L, it.msgs, it.comp, it.sets, it.table, rands, it.seg)[4] == want
    # nseg == 0: GBLS_SUCCESS, the set outputs at their pre-fill, the table decoded all the same
    got = items_local(G, L, it.msgs, it.comp, it.sets, it.table, it.rands, [0])
    assert got == (G.SUCCESS, 0, [G.BAD_ENCODING] * it.n, [G.BAD_ENCODING] * it.n, [], it.want_pst)


def test_without_local_sets_items_equal_the_spans_call(G, L, local_items):
    b = local_items.base
    for comp in (b.comp, T.clear_flag(T.swap(b.comp, 3, 5), 7)):
        for flags in (0, 1):
            want = T.items(G, L, b.msgs, comp, b.sets, b.rands, b.seg, flags=flags)
            assert want[0] == G.SUCCESS
            assert items_local(G, L, b.msgs, comp, b.sets, [], b.rands, b.seg, flags) == want + ([],)


# ---------------------------------------------------------------- 6. the grouped regime
def test_grouped_regime(G, L, F, RV, E, PK, K):
    rng = random.Random("local/grouped")
    n = 2050
    table = K.valid[:6] + [K.by_status[2]]
    small = [1, 2, 14, 15]
    sets, sks = [], []
    for i in range(n):
        if i % 3 == 0:
            lst = [i % 6] if i % 2 else [i % 6, (i + 1) % 6]
            sets.append(Loc(lst))
            sks.append(sum(K.sks[p] for p in lst))
        else:
            sets.append(S.make_span(E, small[i % 4], [0] if i % 2 else [0, 1], rng, bitlist=i % 5 != 0, shift=i))
            sks.append(sum(E.sks[v] for v in sets[-1].part))
    bad_sig, bad_key = [6, 1032, 2049], [300, 1500]
    for i in bad_key:
        sets[i] = Loc([1, 6])
    msgs = F.messages(n, b"local/grouped")
    comp = bytearray(S.compress(G, L, F.sign([x % F.R_ORDER or 1 for x in sks], msgs)))
    for i in bad_sig:
        comp[96 * i:96 * i + 96] = comp[96 * (i - 1):96 * i]
    comp = bytes(comp)
    rc, err, sst, kst, v, pst = each_local(G, L, msgs, comp, sets, table)
    assert (rc, err) == (G.SUCCESS, 0) and sst == [0] * n and pst == [0] * 6 + [2]
    assert [i for i in range(n) if kst[i]] == bad_key and all(kst[i] == G.BAD_ENCODING for i in bad_key)
    assert [i for i in range(n) if v[i] != G.SUCCESS] == sorted(bad_sig + bad_key)
    # the points call over decoded keys agrees on every set that has a key
    lpts = decompress(G, L, table)[1]
    pidx, poff = flat([[("L", p) for p in s.lst] if is_local(s) else [("R", x) for x in s.part] for s in sets])
    pst_, pv_ = G.i32_array(n), G.i32_array(n)
    G.check(L.gbls_verify_batch_compressed(msgs, comp, b"".join(lpts[p] if t == "L" else PK[p] for t, p in pidx),
                                           G.u32_array(poff), n, pst_, pv_), "points")
    assert [pv_[i] for i in range(n) if i not in bad_key] == [v[i] for i in range(n) if i not in bad_key]
    # samples against the oracle
    pts = T.decode(G, L, comp)[1]
    for i in sorted(bad_sig + [0, 3, 5, 7, 1031, 1033, 2048]):
        key = ref_pk(RV, F, sks[i]) if is_local(sets[i]) else S.oracle_key(RV, E, F, sets[i].part)
        ok = RV.ref_verify(pts[i], msgs[32 * i:32 * i + 32], 32, key)
        assert v[i] == (G.SUCCESS if ok else G.VERIFY_FAIL), i


# ---------------------------------------------------------------- 7. children, policies
def child(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_local_child.py")] + list(args),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_two_engines_subprocess():
    res = child("replicas")
    assert res["engines"] == 2 and res["rc"] == [0, 0]
    assert res["failing"] == res["want_failing"] and res["key_status"] == res["want_key_status"]
    assert res["pkb_status"] == res["want_pkb_status"] and res["items"] == [0, 5]


def test_concurrent_callers_with_their_own_tables_subprocess():
    res = child("threads")
    assert res["errors"] == [] and res["exact"] == [res["calls"]] * res["threads"] == [20] * 8


def test_dedup_and_message_cache(G, L, F, RV, E, K, local_items):
    it = LItems()
    it.__dict__.update(local_items.__dict__)
    um = F.messages(4, b"local/repeated")
    it.msgs = b"".join(um[32 * (i % 4):32 * (i % 4) + 32] for i in range(it.n))
    sk = [sum(E.sks[v] for v in s.part) for s in it.sets[:it.base.n]] + [K.sks[0], K.sks[1] + K.sks[2],
         sum(E.sks[v] for v in it.sets[it.base.n + 2].part), K.sks[3], K.sks[4], 1]
    it.sigs = F.sign([x % F.R_ORDER for x in sk], it.msgs)
    it.comp = S.compress(G, L, it.sigs)
    bad = T.clear_flag(T.swap(it.comp, 3, it.base.n), 7)
    want_good = T.ref_items(RV, it, seg=it.seg[:-1]) + [G.VERIFY_FAIL]
    assert want_good == [G.SUCCESS] * 8 + [G.VERIFY_FAIL]

    def both():
        return [items_local(G, L, it.msgs, c, it.sets, it.table, it.rands, it.seg) for c in (it.comp, bad)]

    plain = both()
    assert plain[0] == (G.SUCCESS, 0, [0] * it.n, it.want_kst, want_good, it.want_pst)
    assert plain[1][4] == [G.SUCCESS, G.VERIFY_FAIL, G.SUCCESS, G.VERIFY_FAIL, G.SUCCESS, G.SUCCESS, G.VERIFY_FAIL,
                           G.SUCCESS, G.VERIFY_FAIL]
    assert plain[1][2] == T.decode(G, L, bad)[0]
    with S.dedup_policy(L, G):
        assert both() == plain
    out = (ctypes.c_uint64 * 8)()
    assert L.gbls_msgcache_configure(256) == 0
    try:
        assert L.gbls_msgcache_stats(out) == 0
        hits0 = out[1]
        assert both() == plain   # cold
        assert both() == plain   # warm
        assert L.gbls_msgcache_stats(out) == 0 and out[1] > hits0
    finally:
        assert L.gbls_msgcache_configure(0) == 0


# ---------------------------------------------------------------- 8. argument errors
def test_argument_errors_fail_closed(G, L, local_items):
    it = local_items
    n, nseg, t = it.n, len(it.seg) - 1, len(it.table)
    first = it.base.n   # the first local set
    prefill = (G.VERIFY_FAIL, 102, [G.BAD_ENCODING] * n, [G.BAD_ENCODING] * n)

    def variant(i, **kw):
        out = list(it.sets)
        s = Loc([])
        s.__dict__.update(it.sets[i].__dict__)
        s.__dict__.update(kw)
        out[i] = s
        return out

    for sets in (variant(first, mask=S.mask_bytes([3])),   # a local set with committee bits
                 variant(first, field=b"\x03"),            # a local set with a bit string
                 variant(1, field=b"\x03"),                # a plain set with one, as in the span calls
                 variant(0, lst=[3])):                     # a span set with a key range
        assert each_local(G, L, it.msgs, it.comp, sets, it.table) == prefill + ([G.VERIFY_FAIL] * n, [G.BAD_ENCODING] * t)
        assert items_local(G, L, it.msgs, it.comp, sets, it.table, it.rands, it.seg) == prefill + (
            [G.VERIFY_FAIL] * nseg, [G.BAD_ENCODING] * t)
        assert local_keys(G, L, sets, it.table, expect_rc=G.VERIFY_FAIL) == ([bytes(96)] * n, [G.BAD_ENCODING] * n,
                                                                           [G.BAD_ENCODING] * t)
        assert L.gbls_last_error() == 102
    com, masks, bits, boff, idx, off = S.spans_args(G, it.sets)
    pkb, _ = table_args(G, it.table)
    rands, seg = u64(it.rands), G.u32_array(it.seg)

    def calls(off_, pkb_, npkb_):
        st, kst, v, pst = marked(G, n), marked(G, n), marked(G, n), marked(G, t)
        out = ctypes.create_string_buffer(b"\xff" * (96 * n), 96 * n)
        yield L.gbls_verify_each_local(it.msgs, it.comp, com, masks, bits, boff, idx, off_, pkb_, npkb_, n, st, kst, v, pst), (st, kst, v, pst)
        st, kst, v, pst = marked(G, n), marked(G, n), marked(G, nseg), marked(G, t)
        yield L.gbls_verify_items_local(it.msgs, it.comp, com, masks, bits, boff, idx, off_, pkb_, npkb_, rands, n, seg,
                                        nseg, st, kst, v, pst, 0), (st, kst, v, pst)
        st, pst = marked(G, n), marked(G, t)
        yield L.gbls_g1_aggregate_local(com, masks, bits, boff, idx, off_, pkb_, npkb_, n, out, st, pst), (st, pst)

    # a local set when pk_off is NULL; pkb == NULL with npkb > 0; npkb that does not fit 32 bits (pkb_status is
    # then left alone: the count names no array)
    for off_, pkb_, npkb_, pst_want in ((None, pkb, t, G.BAD_ENCODING), (off, None, t, G.BAD_ENCODING),
                                        (off, pkb, 1 << 32, 77)):
        for rc, outs in calls(off_, pkb_, npkb_):
            assert (rc, L.gbls_last_error()) == (G.VERIFY_FAIL, 102)
            assert ints(outs[0], n) == [G.BAD_ENCODING] * n and ints(outs[-1], t) == [pst_want] * t
            if len(outs) == 4:
                assert ints(outs[1], n) == [G.BAD_ENCODING] * n and set(ints(outs[2], nseg)) == {G.VERIFY_FAIL}
    # in the span calls 0xFFFFFFFE stays a base slot past the table: rejected per set, not an argument error
    keys, st = S.span_keys(G, L, [S.raw_span(None, LOCAL, [0], S.encode([1] * 9, True)), it.sets[1]])
    assert st == [G.BAD_ENCODING, 0] and keys[0] == bytes(96)
    # a following good call succeeds
    want = [G.SUCCESS] * (nseg - 1) + [G.VERIFY_FAIL]
    assert items_local(G, L, it.msgs, it.comp, it.sets, it.table, it.rands, it.seg) == (
        G.SUCCESS, 0, [0] * n, it.want_kst, want, it.want_pst)


# ---------------------------------------------------------------- 9. the Python mirror
def test_python_mirror_takes_the_local_path(G, L, F, RV, E, K, local_items):
    from grandine_amd import bls as B
    from grandine_amd import verifier as V
    it = local_items
    # the library's own methods give the C call's outputs
    args = ([it.msgs[32 * i:32 * i + 32] for i in range(it.n)], [it.comp[96 * i:96 * i + 96] for i in range(it.n)],
            [s.base for s in it.sets], [s.mask for s in it.sets], [s.field for s in it.sets], [s.lst for s in it.sets],
            it.table)
    want = [G.SUCCESS] * 8 + [G.VERIFY_FAIL]
    verdicts, statuses, pst = B.Signature.verify_items_local(*args, it.seg, randoms=it.rands, with_statuses=True)
    assert verdicts == [x == G.SUCCESS for x in want] and pst == it.want_pst
    assert statuses == [(0, k) for k in it.want_kst]
    per_set, pst = B.Signature.verify_each_local(*args)
    assert pst == it.want_pst and [ok for _, _, ok in per_set] == [True] * (it.n - 1) + [False]
    # MultiVerifier: triples that keep their 48 bytes ride along with the block's span sets
    b = S.make_block(G, L, F, RV, E)
    keys48 = [E.comp[48 * i:48 * i + 48] for i in range(S.NREG + 1)]
    B.Registry.forget()
    try:
        B.Registry.mirror_finalized(keys48)  # first = 0 rewrites the registry: the table is cleared
        raw = F.public_keys(E.sks)
        pk = [B.PublicKey(raw[96 * v:96 * v + 96]) for v in range(S.NREG + 1)]
        coms = [E.members[S.BIG_FIRST + c] for c in range(S.BIG_N)]
        comp = S.compress(G, L, b.sigs)
        lm = F.messages(3, b"local/mirror")
        lsig = S.compress(G, L, F.sign(K.sks[:3], lm))

        def triples(local_sigs, key2=K.valid[2]):
            out = []
            for i, s in enumerate(b.sets):
                msg, sig = b.msgs[32 * i:32 * i + 32], comp[96 * i:96 * i + 96]
                keys = [pk[v] for v in s.part]
                t = V.Triple()
                if s.base is None:
                    t.verify_aggregate_indexed(msg, sig, s.lst, keys, None)
                else:
                    t.verify_aggregate_committees(msg, sig, s.base, s.mask, [E.members[s.base + c] for c in s.named],
                                                  s.field, keys, None)
                out.append(t)
            for j, key in enumerate((K.valid[0], K.valid[1], key2)):
                t = V.Triple()
                t.verify_singular_bytes(lm[32 * j:32 * j + 32], local_sigs[96 * j:96 * j + 96], key)
                out.append(t)
            return out

        def run(members, local_sigs):
            assert B.Committees.set(S.BIG_FIRST, coms, members=members) == [0] * S.BIG_N
            mv = V.MultiVerifier(triples=triples(local_sigs))
            try:
                ok = mv.finish(randoms=b.rands + [3, 5, 7]) is None
            except V.SignatureInvalid:
                ok = False
            return ok, mv.last_path, mv.verify_each(), mv.last_each_path

        good, bad = [True] * (b.n + 3), [True] * b.n + [False, False, True]
        assert run(True, lsig) == (True, "local", good, "local")
        assert run(True, T.swap(lsig, 0, 1)) == (False, "local", bad, "local")
        mv = V.MultiVerifier(triples=triples(T.swap(lsig, 0, 1)))
        assert mv.verify_items([0] * b.n + [1, 2, 2], randoms=b.rands + [3, 5, 7]) == [True, False, False]
        assert mv.last_each_path == "local"
        # a local key that does not decode: the decoding error comes first, as for a signature
        mv = V.MultiVerifier(triples=triples(lsig, key2=K.by_status[3]))
        with pytest.raises(B.DecompressionFailed):
            mv.finish(randoms=b.rands + [3, 5, 7])
        assert mv.last_path == "local" and mv.verify_each() == [True] * (b.n + 2) + [False]
        # the slots loaded without members: the rest does not qualify for "spans", the kept bytes are decoded through
        # the engine and the points path gives the same outcomes
        assert run(False, lsig) == (True, "points", good, "points")
        assert run(False, T.swap(lsig, 0, 1)) == (False, "points", bad, "points")
    finally:
        B.Registry.forget()
        S.load_all(G, L, F)
