"""Per-set and per-item verdicts over span sets on the GPU (include/grandine_bls_gpu_each.h):
gbls_verify_each_spans and gbls_verify_items_spans against the C oracle (ref_verify,
ref_multi_verify, ref_sk_to_pk over summed secret keys) and against the engine's earlier calls
(gbls_g2_decompress for the signature statuses, the spans key call for the key statuses,
gbls_verify_batch_compressed and gbls_multi_verify_segments over explicit key points, the spans
batch call for one-item calls).  The calls under test are never a yardstick.

The environment is that of tests/test_gpu_spans.py (600 registry keys plus one negation, slots of
1 to 65 members, eight slots of 512, the twin, cancelling and member-less slots); its helpers are
imported."""
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
from test_gpu_spans import E, F, G, L, REF  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu

ROOT = S.ROOT
Span, u64, flat = S.Span, S.u64, S.flat


@pytest.fixture(scope="module")
def RV(REF):
    REF.ref_verify.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    return REF


@pytest.fixture(scope="module")
def PK(E, F):
    raw = F.public_keys(E.sks)
    return [raw[96 * v:96 * v + 96] for v in range(S.NREG + 1)]


def w4_max():
    txt = open(os.path.join(ROOT, "grandine_amd", "csrc", "gbls_common.h")).read()
    return int(re.search(r"#define GBLS_W4_MAX (\d+)", txt).group(1))


def ints(a, n):
    return [a[i] for i in range(n)]


def each(G, L, msgs, comp, sets, fill=77):
    n = len(sets)
    st, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
    for i in range(n):
        st[i] = kst[i] = v[i] = fill
    rc = L.gbls_verify_each_spans(msgs, comp, *S.spans_args(G, sets), n, st, kst, v)
    return rc, L.gbls_last_error(), ints(st, n), ints(kst, n), ints(v, n)


def items(G, L, msgs, comp, sets, rands, seg, flags=0, fill=77):
    n, nseg = len(sets), len(seg) - 1
    st, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(nseg)
    for i in range(n):
        st[i] = kst[i] = fill
    for s in range(nseg):
        v[s] = fill
    rc = L.gbls_verify_items_spans(msgs, comp, *S.spans_args(G, sets), u64(rands), n, G.u32_array(seg), nseg, st, kst, v,
                                   flags)
    return rc, L.gbls_last_error(), ints(st, n), ints(kst, n), ints(v, nseg)


def decode(G, L, comp):
    """The yardstick of sig_status: gbls_g2_decompress; also the points, for the oracle."""
    n = len(comp) // 96
    out, st = ctypes.create_string_buffer(192 * n), G.i32_array(n)
    G.check(L.gbls_g2_decompress(comp, n, out, st), "decompress")
    return ints(st, n), [out.raw[192 * i:192 * i + 192] for i in range(n)]


def points_each(G, L, PK, msgs, comp, sets):
    """The same checks through gbls_verify_batch_compressed over the participants' key points."""
    n = len(sets)
    idx, off = flat([s.part for s in sets])
    st, v = G.i32_array(n), G.i32_array(n)
    G.check(L.gbls_verify_batch_compressed(msgs, comp, b"".join(PK[i] for i in idx) or bytes(96), G.u32_array(off), n, st,
                                           v), "points")
    return ints(st, n), ints(v, n)


def signed(G, L, F, E, sets, seed):
    msgs = F.messages(len(sets), seed)
    sigs = F.sign([sum(E.sks[v] for v in s.part) % F.R_ORDER or 1 for s in sets], msgs)
    return msgs, S.compress(G, L, sigs)


def clear_flag(comp, i):
    out = bytearray(comp)
    out[96 * i] &= 0x7F  # the compression flag
    return bytes(out)


def swap(comp, i, j):
    out = bytearray(comp)
    out[96 * i:96 * i + 96], out[96 * j:96 * j + 96] = comp[96 * j:96 * j + 96], comp[96 * i:96 * i + 96]
    return bytes(out)


# ---------------------------------------------------------------- 1. per-set verdicts
PLANTED = {"swap-a": 10, "swap-b": 23, "undecodable": 30, "non-signer": 44, "malformed": 51, "no-participant": 58,
           "zero-mask": 72, "past-table": 79, "infinite": 93, "empty-plain": 100}


def each_sets(E):
    sets = S.key_sets(E)
    assert len(sets) == 133 and {1, 2, 3, 8, 64} <= {len(s.named) for s in sets if s.base is not None}
    assert {s.bitlist for s in sets if s.base is not None} == {True, False}
    assert any(s.base is not None and len(s.named) == 1 and not s.bitlist for s in sets) and any(s.base is None for s in sets)
    # a non-signer's bit: the next span set at or after its place that has a clear bit
    k = next(i for i in range(PLANTED["non-signer"], 133) if sets[i].base is not None and
             not all(x for b in sets[i].per for x in b))
    assert k < PLANTED["malformed"] - 1
    t = sets[k]
    per = [list(b) for b in t.per]
    c = next(i for i, b in enumerate(per) if not all(b))
    per[c][per[c].index(0)] = 1
    planted = dict(PLANTED, **{"non-signer": k})
    good = S.make_span(E, 0, [1, 3, 4], random.Random("each/bad"), kinds=["most", "most", "few"])
    bad = {
        "non-signer": Span(E, t.base, t.named, per, t.bitlist),
        "malformed": S.raw_span(E, good.base, good.named, good.field[:-1]),
        "no-participant": Span(E, good.base, good.named, [good.per[0], [0] * len(good.per[1]), good.per[2]], True),
        "zero-mask": S.raw_span(E, 0, [], b""),
        "past-table": S.raw_span(E, S.TABLE_SIZE, [0], S.encode([1] * 9, True)),
        "infinite": Span(E, S.CANCEL_A, [0, 1], [[1, 0, 0], [1, 0, 0]], True),
        "empty-plain": Span(E, plain=[]),
    }
    signing = list(sets)  # the signatures are those of the sets before the planting
    for name, s in bad.items():
        sets[planted[name]] = s
    return sets, signing, planted


def test_per_set_verdicts(G, L, F, RV, E, PK):
    sets, signing, planted = each_sets(E)
    n = len(sets)
    msgs, comp = signed(G, L, F, E, signing, b"each/sets")
    comp = clear_flag(swap(comp, planted["swap-a"], planted["swap-b"]), planted["undecodable"])
    # the yardsticks, once
    want_sst, pts = decode(G, L, comp)
    want_kst = S.span_keys(G, L, sets)[1]
    okeys = [S.oracle_key(RV, E, F, s.part) for s in sets]
    want_v = [G.SUCCESS if want_sst[i] == 0 and want_kst[i] == 0 and
              RV.ref_verify(pts[i], msgs[32 * i:32 * i + 32], 32, okeys[i]) else G.VERIFY_FAIL for i in range(n)]
    bad = set(planted.values())
    assert [i for i in range(n) if want_v[i] != G.SUCCESS] == sorted(bad)
    assert want_sst[planted["undecodable"]] != 0 and sum(1 for x in want_sst if x) == 1
    assert {i for i in range(n) if want_kst[i]} == {planted[k] for k in ("malformed", "no-participant", "zero-mask",
                                                                         "past-table", "empty-plain")}
    assert want_kst[planted["empty-plain"]] == G.AGGR_TYPE_MISMATCH and want_kst[planted["infinite"]] == 0
    assert okeys[planted["infinite"]] == bytes(96)
    pst, pv = points_each(G, L, PK, msgs, comp, sets)
    assert pst == want_sst

    def check(order):
        chunk = [sets[i] for i in order]
        rc, err, sst, kst, v = each(G, L, b"".join(msgs[32 * i:32 * i + 32] for i in order),
                                    b"".join(comp[96 * i:96 * i + 96] for i in order), chunk)
        assert (rc, err) == (G.SUCCESS, 0)
        assert sst == [want_sst[i] for i in order]
        assert kst == [want_kst[i] for i in order]
        assert v == [want_v[i] for i in order]
        for k, i in enumerate(order):
            if want_sst[i] == 0 and want_kst[i] == 0:
                assert v[k] == pv[i], i                      # ... as over explicit key points
            if i in bad:                                     # every clean neighbour of a planted failure passes
                assert all(v[j] == G.SUCCESS for j in (k - 1, k + 1) if 0 <= j < len(order) and order[j] not in bad)

    pos = 0
    for m in S.LAUNCHES:
        check(list(range(pos, pos + m)))
        pos += m
    assert pos == n
    # at the latency regime's bound and just above it: the same sets, repeated
    for m in (w4_max(), w4_max() + 1):
        check([i % n for i in range(m)])


# ---------------------------------------------------------------- 2. items
class Items:
    pass


def make_items(G, L, F, RV, E):
    it = Items()
    rng = random.Random("each/items")
    mk = lambda base, named, **kw: S.make_span(E, base, named, rng, **kw)  # noqa: E731
    it.sets = [mk(0, [1, 2]), Span(E, plain=[9, 10]), mk(3, [0], bitlist=False),            # 3
               mk(S.TAIL_FIRST, [0, 1, 2]), Span(E, plain=[77]), mk(5, [2, 9]),            # 3
               mk(20, [0, 1]),                                                             # 1
               Span(E, plain=[1, 2, 3]), mk(S.TWIN_A, [0, 1]),                              # 2
               mk(40, [0]), mk(41, [0, 1], bitlist=False), Span(E, plain=[400]),            # 3
               mk(S.BIG_FIRST, list(range(8))), Span(E, plain=[599])]                       # an 8-committee span and a plain set
    it.seg = [0, 3, 6, 7, 9, 12, 14]
    it.n = len(it.sets)
    it.msgs = F.messages(it.n, b"each/items")
    it.sigs = F.sign([sum(E.sks[v] for v in s.part) % F.R_ORDER for s in it.sets], it.msgs)
    it.comp = S.compress(G, L, it.sigs)
    it.rands = F.rands(it.n, 808)
    it.pks = b"".join(S.oracle_key(RV, E, F, s.part) for s in it.sets)
    return it


def ref_items(RV, it, sigs=None, rands=None, seg=None):
    sigs, rands, seg = sigs or it.sigs, rands or it.rands, seg or it.seg
    out = []
    for a, b in zip(seg, seg[1:]):
        ok = b > a and RV.ref_multi_verify(it.msgs[32 * a:32 * b], sigs[192 * a:192 * b], it.pks[96 * a:96 * b],
                                           u64(rands[a:b]), b - a, 16)
        out.append(G_SUCCESS if ok else G_FAIL)
    return out


G_SUCCESS, G_FAIL = 0, 5


@pytest.fixture(scope="module")
def item_batch(G, L, F, RV, E):
    return make_items(G, L, F, RV, E)


def test_items_against_the_oracle(G, L, RV, E, item_batch):
    it = item_batch
    nseg = len(it.seg) - 1
    zeros = [0] * it.n
    assert [b - a for a, b in zip(it.seg, it.seg[1:])] == [3, 3, 1, 2, 3, 2]
    want = ref_items(RV, it)
    assert want == [G.SUCCESS] * nseg
    assert items(G, L, it.msgs, it.comp, it.sets, it.rands, it.seg) == (G.SUCCESS, 0, zeros, zeros, want)
    # one item with a swapped signature (sets 3 and 5 of item 1)
    sw = bytearray(it.sigs)
    sw[192 * 3:192 * 4], sw[192 * 5:192 * 6] = it.sigs[192 * 5:192 * 6], it.sigs[192 * 3:192 * 4]
    want = ref_items(RV, it, sigs=bytes(sw))
    assert want == [G.SUCCESS, G.VERIFY_FAIL] + [G.SUCCESS] * 4
    assert items(G, L, it.msgs, swap(it.comp, 3, 5), it.sets, it.rands, it.seg) == (G.SUCCESS, 0, zeros, zeros, want)
    # one item with a signature that does not decode: its status, its item fails, the others pass
    comp = clear_flag(it.comp, 7)
    want_sst = decode(G, L, comp)[0]
    assert want_sst[7] != 0 and not any(want_sst[:7] + want_sst[8:])
    want = [G.SUCCESS] * 3 + [G.VERIFY_FAIL] + [G.SUCCESS] * 2
    assert items(G, L, it.msgs, comp, it.sets, it.rands, it.seg) == (G.SUCCESS, 0, want_sst, zeros, want)
    # one item with a malformed string: its key status
    sets = list(it.sets)
    sets[0] = S.raw_span(E, sets[0].base, sets[0].named, sets[0].field[:-1])
    want_kst = S.span_keys(G, L, sets)[1]
    assert want_kst == [G.BAD_ENCODING] + [0] * (it.n - 1)
    want = [G.VERIFY_FAIL] + [G.SUCCESS] * 5
    assert items(G, L, it.msgs, it.comp, sets, it.rands, it.seg) == (G.SUCCESS, 0, zeros, want_kst, want)


def segments_points(G, L, it, rands, seg):
    nseg = len(seg) - 1
    v = G.i32_array(nseg)
    G.check(L.gbls_multi_verify_segments(it.msgs, it.sigs, it.pks, u64(rands), it.n, G.u32_array(seg), nseg, v), "segments")
    return ints(v, nseg)


def test_empty_item_and_zero_scalar_as_the_segments_call(G, L, item_batch):
    it = item_batch
    zeros = [0] * it.n
    seg = [0, 3, 3, 6, 7, 9, 12, 14, 14]   # an empty item in the middle and one at the end
    want = segments_points(G, L, it, it.rands, seg)
    assert want == [G.SUCCESS, G.VERIFY_FAIL] + [G.SUCCESS] * 5 + [G.VERIFY_FAIL]
    assert items(G, L, it.msgs, it.comp, it.sets, it.rands, seg) == (G.SUCCESS, 0, zeros, zeros, want)
    rands = list(it.rands)
    rands[4] = 0                            # a zero scalar in item 1
    want = segments_points(G, L, it, rands, it.seg)
    assert want == [G.SUCCESS, G.VERIFY_FAIL] + [G.SUCCESS] * 4
    assert items(G, L, it.msgs, it.comp, it.sets, rands, it.seg) == (G.SUCCESS, 0, zeros, zeros, want)
    # n == 0 or nseg == 0: GBLS_SUCCESS, nothing written past the pre-fill (n statuses, nseg verdicts)
    def marked():
        a = G.i32_array(it.n)
        for i in range(it.n):
            a[i] = 77
        return a

    args = S.spans_args(G, it.sets)
    st, kst, v = marked(), marked(), marked()
    assert L.gbls_verify_items_spans(it.msgs, it.comp, *args, u64(it.rands), it.n, G.u32_array([0]), 0, st, kst, v, 0) == 0
    assert L.gbls_last_error() == 0 and ints(v, it.n) == [77] * it.n
    assert ints(st, it.n) == ints(kst, it.n) == [G.BAD_ENCODING] * it.n
    st, kst, v = marked(), marked(), marked()
    assert L.gbls_verify_each_spans(it.msgs, it.comp, *args, 0, st, kst, v) == 0 and L.gbls_last_error() == 0
    assert ints(st, it.n) == ints(kst, it.n) == ints(v, it.n) == [77] * it.n


@pytest.fixture(scope="module")
def block(G, L, F, RV, E):
    return S.make_block(G, L, F, RV, E)


@pytest.mark.parametrize("flags", [0, 1])  # 1: GBLS_CALL_BLOCK
def test_one_item_equals_the_batch_call(G, L, E, block, flags):
    b = block
    assert b.n == 12
    for sigs in (b.sigs, S.swapped(b)):
        rc, sst, err = S.mv_spans(G, L, b, sigs=sigs, flags=flags)
        assert err == 0 and sst == [0] * b.n and rc in (G.SUCCESS, G.VERIFY_FAIL)
        got = items(G, L, b.msgs, S.compress(G, L, sigs), b.sets, b.rands, [0, b.n], flags=flags)
        assert got == (G.SUCCESS, 0, [0] * b.n, [0] * b.n, [rc])
    assert S.mv_spans(G, L, b, flags=flags)[0] == G.SUCCESS != S.mv_spans(G, L, b, sigs=S.swapped(b), flags=flags)[0]


# ---------------------------------------------------------------- 3. the grouped regime
def test_grouped_regime(G, L, F, RV, E, PK):
    rng = random.Random("each/grouped")
    n = 2050
    small = [1, 2, 14, 15] + list(range(S.TAIL_FIRST, S.TABLE_SIZE - 1))   # with the slot after: 7, 8 or 9 members
    assert all(3 <= len(E.members[s]) <= 9 and 3 <= len(E.members[s + 1]) <= 9 for s in small)
    sets = []
    for i in range(n):
        base = small[i % len(small)]
        sets.append(S.make_span(E, base, [0] if i % 2 else [0, 1], rng, bitlist=i % 3 != 0, shift=i))
    msgs, comp = signed(G, L, F, E, sets, b"each/grouped")
    bad_sig, bad_str = [5, 1031, 2049], [700, 1500]
    comp = bytearray(comp)
    for i in bad_sig:
        comp[96 * i:96 * i + 96] = comp[96 * (i - 1):96 * i]   # its neighbour's valid signature
    comp = bytes(comp)
    for i in bad_str:
        sets[i] = S.raw_span(E, sets[i].base, sets[i].named, sets[i].field + b"\x01")
    rc, err, sst, kst, v = each(G, L, msgs, comp, sets)
    assert (rc, err) == (G.SUCCESS, 0) and sst == [0] * n
    assert [i for i in range(n) if kst[i]] == bad_str and all(kst[i] == G.BAD_ENCODING for i in bad_str)
    assert [i for i in range(n) if v[i] != G.SUCCESS] == sorted(bad_sig + bad_str)
    assert set(v) == {G.SUCCESS, G.VERIFY_FAIL}
    # the planted strings are malformed for the key call too, and the points call agrees on every verdict
    # (a malformed set has no key points to give: its participants are read from the string as planted)
    assert [S.span_keys(G, L, [sets[i]])[1] for i in bad_str] == [[G.BAD_ENCODING]] * 2
    pst, pv = points_each(G, L, PK, msgs, comp, sets)
    assert pst == sst and [pv[i] for i in range(n) if i not in bad_str] == [v[i] for i in range(n) if i not in bad_str]
    # the five and 11 good samples against the oracle
    pts = decode(G, L, comp)[1]
    for i in sorted(bad_sig + bad_str + [0, 1, 6, 699, 701, 1030, 1032, 1499, 1501, 2047, 2048]):
        ok = kst[i] == 0 and RV.ref_verify(pts[i], msgs[32 * i:32 * i + 32], 32, S.oracle_key(RV, E, F, sets[i].part))
        assert v[i] == (G.SUCCESS if ok else G.VERIFY_FAIL), i


# ---------------------------------------------------------------- 4, 5. two engines, concurrency
def child(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_each_child.py")] + list(args),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_two_engines_subprocess():
    res = child("replicas")
    assert res["engines"] == 2 and res["each"] == [0, 0]
    assert res["each_failing"] == [100, 3000, 4000] and res["each_verdicts_other"] == []
    assert res["each_key_status"] == [[100, 1], [4000, 1]] and res["each_sig_status"] == []
    assert res["items"] == [0, 0, [0, 5]] and res["items_status"] == [0, 0]


def test_concurrent_callers_subprocess():
    res = child("threads")
    assert res["errors"] == [] and res["exact"] == [res["calls"]] * res["threads"] == [20] * 8


# ---------------------------------------------------------------- 6. policies
def test_dedup_and_message_cache(G, L, F, RV, E, item_batch):
    """Items with repeated messages: the same verdicts and statuses with GBLS_INIT_DEDUP, and with
    the message line cache cold then warm, as without either."""
    it = Items()
    it.__dict__.update(item_batch.__dict__)
    um = F.messages(4, b"each/repeated")
    it.msgs = b"".join(um[32 * (i % 4):32 * (i % 4) + 32] for i in range(it.n))
    it.sigs = F.sign([sum(E.sks[v] for v in s.part) % F.R_ORDER for s in it.sets], it.msgs)
    it.comp = S.compress(G, L, it.sigs)
    bad = clear_flag(swap(it.comp, 3, 5), 7)
    sets = list(it.sets)
    sets[12] = S.raw_span(E, sets[12].base, sets[12].named, sets[12].field + b"\x01")   # one byte long
    plain = [items(G, L, it.msgs, it.comp, it.sets, it.rands, it.seg), items(G, L, it.msgs, bad, sets, it.rands, it.seg)]
    assert plain[0] == (G.SUCCESS, 0, [0] * it.n, [0] * it.n, ref_items(RV, it))
    assert plain[1][4] == [G.SUCCESS, G.VERIFY_FAIL, G.SUCCESS, G.VERIFY_FAIL, G.SUCCESS, G.VERIFY_FAIL]
    assert plain[1][2] == decode(G, L, bad)[0] and plain[1][3] == S.span_keys(G, L, sets)[1]

    def both():
        return [items(G, L, it.msgs, it.comp, it.sets, it.rands, it.seg), items(G, L, it.msgs, bad, sets, it.rands, it.seg)]

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


# ---------------------------------------------------------------- 7. argument errors
def test_argument_errors_fail_closed(G, L, item_batch):
    it = item_batch
    n, nseg = it.n, len(it.seg) - 1
    prefill = (G.VERIFY_FAIL, 102, [G.BAD_ENCODING] * n, [G.BAD_ENCODING] * n)

    def variant(i, **kw):
        out = list(it.sets)
        s = Span(None, plain=[])
        s.__dict__.update(it.sets[i].__dict__)
        s.__dict__.update(kw)
        out[i] = s
        return out

    for sets in (variant(1, mask=S.mask_bytes([3])),   # a plain set with committee bits
                 variant(1, field=b"\x03"),            # a plain set with aggregation bits
                 variant(0, lst=[3])):                 # a span set with a key range
        assert each(G, L, it.msgs, it.comp, sets) == prefill + ([G.VERIFY_FAIL] * n,)
        assert items(G, L, it.msgs, it.comp, sets, it.rands, it.seg) == prefill + ([G.VERIFY_FAIL] * nseg,)
    for seg in ([0, 3, 2, 7, 9, 12, 14], [1, 3, 6, 7, 9, 12, 14], [0, 3, 6, 7, 9, 12, 13]):   # bad seg_off
        assert items(G, L, it.msgs, it.comp, it.sets, it.rands, seg) == prefill + ([G.VERIFY_FAIL] * nseg,)
    # NULL bits_off, cbits, key_status or verdicts
    com, masks, bits, boff, idx, off = S.spans_args(G, it.sets)
    rands, seg = u64(it.rands), G.u32_array(it.seg)
    for null in ("boff", "masks", "kst", "v"):
        st, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
        a = dict(com=com, masks=masks, bits=bits, boff=boff, idx=idx, off=off, st=st, kst=kst, v=v)
        a[null] = None
        sets = (a["com"], a["masks"], a["bits"], a["boff"], a["idx"], a["off"])
        for call in ("each", "items"):
            for x in (st, kst, v):
                for i in range(n):
                    x[i] = 77
            if call == "each":
                rc = L.gbls_verify_each_spans(it.msgs, it.comp, *sets, n, a["st"], a["kst"], a["v"])
            else:
                rc = L.gbls_verify_items_spans(it.msgs, it.comp, *sets, rands, n, seg, nseg, a["st"], a["kst"], a["v"], 0)
            assert (rc, L.gbls_last_error()) == (G.VERIFY_FAIL, 102), (null, call)
            assert ints(st, n) == [G.BAD_ENCODING] * n
            assert null == "kst" or ints(kst, n) == [G.BAD_ENCODING] * n
            m = n if call == "each" else nseg
            assert null == "v" or ints(v, m) == [G.VERIFY_FAIL] * m
    # a following good call succeeds
    assert items(G, L, it.msgs, it.comp, it.sets, it.rands, it.seg) == (G.SUCCESS, 0, [0] * n, [0] * n, [G.SUCCESS] * nseg)
    assert each(G, L, it.msgs, it.comp, it.sets) == (G.SUCCESS, 0, [0] * n, [0] * n, [G.SUCCESS] * n)


# ---------------------------------------------------------------- 8. the Python mirror
def test_python_mirror_stays_on_the_compact_path(G, L, F, RV, E, block):
    from grandine_amd import bls as B
    from grandine_amd import verifier as V
    b = block
    keys48 = [E.comp[48 * i:48 * i + 48] for i in range(S.NREG + 1)]
    B.Registry.forget()
    try:
        B.Registry.mirror_finalized(keys48)  # first = 0 rewrites the registry: the table is cleared
        raw = F.public_keys(E.sks)
        pk = [B.PublicKey(raw[96 * v:96 * v + 96]) for v in range(S.NREG + 1)]
        coms = [E.members[S.BIG_FIRST + c] for c in range(S.BIG_N)]
        sw = S.swapped(b)   # sets 1 and 7
        comp = S.compress(G, L, sw)
        pts = decode(G, L, comp)[1]
        oracle = [bool(RV.ref_verify(pts[i], b.msgs[32 * i:32 * i + 32], 32, b.pks[96 * i:96 * i + 96])) for i in range(b.n)]
        assert [i for i, ok in enumerate(oracle) if not ok] == [1, 7]

        def triples():
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
            return out

        def run(members):
            assert B.Committees.set(S.BIG_FIRST, coms, members=members) == [0] * S.BIG_N
            mv = V.MultiVerifier(triples=triples())
            with pytest.raises(V.SignatureInvalid):
                mv.finish(randoms=b.rands)
            return mv.last_path, mv.verify_each(), mv.last_each_path

        assert run(True) == ("spans", oracle, "spans")
        its = list("abcdefghijkl")
        assert V.split_failed_batch(its, [[t] for t in triples()]) == ([x for x in its if x not in "bh"], ["b", "h"])
        mv = V.MultiVerifier(triples=triples())
        assert mv.verify_items([0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3], randoms=b.rands) == [False, True, False, True]
        assert mv.last_each_path == "spans"
        # the same triples with the slots loaded without members: the points path, the same outcomes
        assert run(False) == ("indices", oracle, "points")
        assert V.split_failed_batch(its, [[t] for t in triples()]) == ([x for x in its if x not in "bh"], ["b", "h"])
    finally:
        B.Registry.forget()
        S.load_all(G, L, F)
