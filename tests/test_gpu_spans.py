"""Span sets on the GPU (include/grandine_bls_gpu_spans.h): attestations over several committees, a
base slot, committee_bits and ONE bit string over the named committees; keys against the oracle and
against the indexed sum, rejections with unaffected neighbours, degenerate folds, batch verdicts
against the C oracle and against gbls_multi_verify_compressed_ex over explicit index lists, the
launch forms, replicas, and the Python mirror.

The secret keys are known, so the oracle's key of a set is ref_sk_to_pk(sum of the participants'
secret keys mod r) and every comparison is byte for byte or verdict for verdict.

Launch forms crossed here: k_g1_span_pieces runs one lane per piece while the longest piece of the
launch adds fewer than kCommitteeRowMin keys and one 16-lane row per piece from there on (the child
script forces each form over the same sets); k_g1_span_keys runs one lane per set while no set has
kSpanFoldRowMin = 8 pieces and one row per set from there on (launches of both kinds below)."""
import contextlib
import ctypes
import json
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NREG = 600          # ordinary registry keys; index NREG holds -key[5]
NEG5 = NREG
SIZES = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]   # slots 0..63 cycle these
BIG_FIRST, BIG_N = 64, 8                                    # eight 512-member committees
TWIN_A, TWIN_B = 72, 73                                     # identical members
CANCEL_A, CANCEL_B = 74, 75                                 # key 5 in one, its negation in the other
INF_SLOT, PLAIN_SLOT, GAP = 76, 77, 78                      # infinite sum; loaded without members; never written
TAIL_FIRST, TABLE_SIZE = 79, 100                            # slots 79..99: nine members each
KINDS = ["full", "one-clear", "one-set", "half", "most", "few"]
LAUNCHES = [1, 3, 64, 65]


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


@pytest.fixture(scope="module")
def REF():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s"])
    C = ctypes.CDLL(os.path.join(ROOT, "oracle", "_build", "libbls_ref.so"))
    C.ref_multi_verify.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                   ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_int]
    C.ref_sk_to_pk.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    return C


def u64(vals):
    return (ctypes.c_uint64 * max(len(vals), 1))(*vals)


def flat(lists):
    off = [0]
    for v in lists:
        off.append(off[-1] + len(v))
    return [i for v in lists for i in v], off


def members_of(c, size):
    return [(37 * c + 11 * j) % NREG for j in range(size)]  # 11 is coprime to 600: distinct up to 600 members


def set_call(G, L, first, coms, members=True):
    idx, off = flat(coms)
    st = G.i32_array(len(coms))
    call = L.gbls_committees_set_members if members else L.gbls_committees_set
    rc = call(first, G.u32_array(idx or [0]), G.u32_array(off), len(coms), st)
    return rc, [st[c] for c in range(len(coms))]


def encode(bits, bitlist):
    m = len(bits)
    out = bytearray(m // 8 + 1 if bitlist else (m + 7) // 8)
    for j, b in enumerate(bits):
        out[j >> 3] |= b << (j & 7)
    if bitlist:
        out[m >> 3] |= 1 << (m & 7)
    return bytes(out)


def mask_bytes(named):
    out = bytearray(8)
    for c in named:
        out[c >> 3] |= 1 << (c & 7)
    return bytes(out)


def committee_bits(m, kind, rng):
    """One committee's bits in one of the three directions (and their edges); never empty."""
    if kind == "full":  # the cached sum unchanged
        return [1] * m
    if kind == "one-clear":  # subtracts its absentee (m = 1: nobody to spare, full)
        return [int(j != m // 3 or m == 1) for j in range(m)]
    if kind == "one-set":  # sums its participant
        return [int(j == (2 * m) // 3) for j in range(m)]
    if kind == "half":  # the tie: participants
        chosen = set(rng.sample(range(m), max(1, m // 2)))
        return [int(j in chosen) for j in range(m)]
    bits = [int(rng.random() < (0.9 if kind == "most" else 0.25)) for _ in range(m)]
    bits[rng.randrange(m)] = 1
    return bits


class Env:
    pass


class Span:
    """One set: a span (base, named committees, their bits, the encoding) or a plain list."""

    def __init__(self, E, base=None, named=(), per=(), bitlist=True, plain=None):
        self.base, self.named, self.per, self.bitlist = base, list(named), [list(b) for b in per], bitlist
        if base is None:
            self.mask, self.field, self.lst, self.part = bytes(8), b"", list(plain), list(plain)
            return
        self.mask, self.lst = mask_bytes(self.named), []
        self.field = encode([x for b in self.per for x in b], bitlist)
        self.part = [v for c, b in zip(self.named, self.per) for v, x in zip(E.members[base + c], b) if x]


def make_span(E, base, named, rng, kinds=None, bitlist=True, shift=0):
    kinds = kinds or [KINDS[(shift + i) % len(KINDS)] for i in range(len(named))]
    return Span(E, base, named, [committee_bits(len(E.members[base + c]), k, rng) for c, k in zip(named, kinds)], bitlist)


def load_all(G, L, F):
    from grandine_amd import bls as B
    B.Registry.forget()
    E = Env()
    E.sks, comp = F.registry(NREG, seed=b"spans")
    E.sks = E.sks + [F.R_ORDER - E.sks[5]]
    comp += F.compress_g1(F.public_keys(E.sks[NREG:]))
    assert not F.load_registry(comp).any()
    E.comp = comp
    E.members = {s: members_of(s, SIZES[s % len(SIZES)]) for s in range(64)}
    for c in range(BIG_N):
        E.members[BIG_FIRST + c] = members_of(200 + c, 512)
    E.members[TWIN_A] = E.members[TWIN_B] = members_of(300, 12)
    E.members[CANCEL_A], E.members[CANCEL_B] = [5, 7, 9], [NEG5, 11, 13]
    inf = [5, NEG5]
    E.load_a = set_call(G, L, 0, [E.members[s] for s in range(INF_SLOT)] + [inf])
    E.load_b = set_call(G, L, PLAIN_SLOT, [members_of(310, 9)], members=False)
    for s in range(TAIL_FIRST, TABLE_SIZE):
        E.members[s] = members_of(400 + s, 9)
    E.load_c = set_call(G, L, TAIL_FIRST, [E.members[s] for s in range(TAIL_FIRST, TABLE_SIZE)])
    return E


@pytest.fixture(scope="module")
def E(G, L, F):
    from grandine_amd import bls as B
    env = load_all(G, L, F)
    yield env
    L.gbls_committees_clear()
    B.Registry.forget()


def oracle_key(REF, E, F, participants):
    s = sum(E.sks[i] for i in participants) % F.R_ORDER
    if not participants or s == 0:
        return bytes(96)
    out = ctypes.create_string_buffer(96)
    REF.ref_sk_to_pk(s.to_bytes(32, "big"), out)
    return out.raw


def spans_args(G, sets):
    idx, off = flat([s.lst for s in sets])
    _, boff = flat([s.field for s in sets])
    return (G.u32_array([G.NO_COMMITTEE if s.base is None else s.base for s in sets]),
            G.buf(b"".join(s.mask for s in sets)), G.buf(b"".join(s.field for s in sets)), G.u32_array(boff),
            G.u32_array(idx or [0]), G.u32_array(off))


def span_keys(G, L, sets, expect_rc=0):
    n = len(sets)
    out = ctypes.create_string_buffer(b"\xff" * (96 * n), 96 * n)
    st = G.i32_array(n)
    for i in range(n):
        st[i] = 77
    rc = L.gbls_g1_aggregate_spans(*spans_args(G, sets), n, out, st)
    assert rc == expect_rc, (rc, L.gbls_last_error())
    return [out.raw[96 * i:96 * i + 96] for i in range(n)], [st[i] for i in range(n)]


def indexed_keys(G, L, lists):
    n = len(lists)
    idx, off = flat(lists)
    out, st = ctypes.create_string_buffer(96 * n), G.i32_array(n)
    G.check(L.gbls_g1_aggregate_indexed(G.u32_array(idx or [0]), G.u32_array(off), n, out, st), "indexed")
    return [out.raw[96 * i:96 * i + 96] for i in range(n)], [st[i] for i in range(n)]


# ---------------------------------------------------------------- the table
def test_loads(G, L, E):
    assert E.load_a == (G.SUCCESS, [0] * (INF_SLOT + 1))  # (the infinite sum: SUCCESS, stored all-zero)
    assert E.load_b == (G.SUCCESS, [0]) and E.load_c == (G.SUCCESS, [0] * (TABLE_SIZE - TAIL_FIRST))
    assert L.gbls_committees_size() == TABLE_SIZE
    assert [L.gbls_committees_members(s) for s in (0, 12, 63, 64, 71, TWIN_B, PLAIN_SLOT, GAP, 99, 100)] == [
        1, 65, 64, 512, 512, 12, 0, 0, 9, 0]


# ---------------------------------------------------------------- keys
def key_sets(E):
    """133 sets: the masks {c} for c in 0, 1, 31, 32, 63, {0, 2, 5}, adjacent pairs, all 64, the eight
    big committees, from several bases, the directions rotating per committee, both encodings, every
    seventh set a plain list."""
    rng = random.Random("spans/keys")
    masks = [(0, [c]) for c in (0, 1, 31, 32, 63)] + [(0, [0, 2, 5]), (3, [0, 2, 5])]
    masks += [(0, [c, c + 1]) for c in (0, 6, 7, 12, 30, 31, 32, 62)] + [(5, [c, c + 1]) for c in (2, 9, 40)]
    masks += [(0, list(range(64))), (BIG_FIRST, list(range(8))), (BIG_FIRST + 2, [0, 1, 3]), (8, list(range(56))),
              (BIG_FIRST - 4, list(range(12)))]
    sets = [make_span(E, 0, [0, 2, 5], rng), make_span(E, 0, [63], rng, bitlist=False), Span(E, plain=[3, 4, 5]),
            make_span(E, 4, [0, 1], rng, shift=1)]
    i = 0
    while len(sets) < sum(LAUNCHES):
        if len(sets) % 7 == 5:
            sets.append(Span(E, plain=[(17 * i + 3 * j) % NREG for j in range(1 + i % 23)]))
        else:
            base, named = masks[i % len(masks)]
            sets.append(make_span(E, base, named, rng, bitlist=i % 2 == 0, shift=i // len(masks)))
        i += 1
    return sets


def test_keys_equal_oracle_and_indexed_sum(G, L, REF, E, F):
    sets = key_sets(E)
    assert len(sets) == 133
    want = [oracle_key(REF, E, F, s.part) for s in sets]
    pos, got = 0, []
    for n in LAUNCHES:
        chunk = sets[pos:pos + n]
        pos += n
        # the first two launches fold in one lane, the other two in rows
        assert (max(len(s.named) for s in chunk) >= 8) == (n >= 64)
        keys, st = span_keys(G, L, chunk)
        assert st == [0] * n
        got += keys
    for i, s in enumerate(sets):
        assert got[i] == want[i] != bytes(96), (i, s.base, s.named)
    ikeys, ist = indexed_keys(G, L, [s.part for s in sets])
    assert ist == [0] * len(sets) and ikeys == got
    # one set took all three directions in its committees (C - S, S, and C unchanged)
    def direction(b):
        return "C" if all(b) else "C-S" if len(b) - sum(b) < sum(b) else "S"
    assert any({direction(b) for b in s.per} == {"C", "C-S", "S"} for s in sets)
    # pk_idx / pk_off may be NULL when no set is plain
    spans = [s for s in sets[:20] if s.base is not None]
    com, masks, bits, boff, _, _ = spans_args(G, spans)
    out, st = ctypes.create_string_buffer(96 * len(spans)), G.i32_array(len(spans))
    assert L.gbls_g1_aggregate_spans(com, masks, bits, boff, None, None, len(spans), out, st) == 0
    assert [out.raw[96 * i:96 * i + 96] for i in range(len(spans))] == [got[i] for i in range(20) if sets[i].base is not None]


# ---------------------------------------------------------------- rejections
def neighbours(E, REF, F):
    rng = random.Random("spans/neighbours")
    sets = [make_span(E, 0, [1, 2], rng), Span(E, plain=[9, 10]), make_span(E, BIG_FIRST, [0, 5], rng, bitlist=False),
            make_span(E, 2, list(range(9)), rng)]
    return sets, [oracle_key(REF, E, F, s.part) for s in sets]


def raw_span(E, base, named, field):
    s = Span(E, plain=[])
    s.base, s.named, s.mask, s.field = base, list(named), mask_bytes(named), field
    return s


def check_rejected(G, L, E, REF, F, bad, status, at=2):
    sets, want = neighbours(E, REF, F)
    at = len(sets) if at is None else at
    sets.insert(at, bad)
    want.insert(at, bytes(96))
    keys, st = span_keys(G, L, sets)
    assert st == [status if i == at else 0 for i in range(len(sets))] and keys == want, (bad.base, bad.named, bad.field.hex())


def test_rejected_span_sets(G, L, REF, E, F):
    rng = random.Random("spans/rejected")
    BAD = G.BAD_ENCODING
    good = make_span(E, 0, [1, 3, 4], rng, kinds=["most", "most", "few"])   # M = 7 + 9 + 15 = 31
    good8 = make_span(E, 0, [1, 2, 3], rng, kinds=["most", "few", "most"])  # M = 24: the lengths differ
    assert span_keys(G, L, [good, good8])[1] == [0, 0]
    nine = encode([1] * 9, True)
    cases = [
        raw_span(E, 0, [], b""), raw_span(E, 5, [], nine),                          # all-zero committee_bits
        raw_span(E, TABLE_SIZE, [0], nine), raw_span(E, 1 << 24, [0], nine),        # past the table
        raw_span(E, TABLE_SIZE - 20, [0, 20], nine),                                # ... with bit 20, 20 below its end
        raw_span(E, TABLE_SIZE - 20, [20], nine),
        raw_span(E, 0xFFFFFFF0, [16], encode([1], True)),                           # + 16 = 2^32: not slot 0
        raw_span(E, 0xFFFFFFF0, [17], encode([1] * 7, True)),                       # ... nor slot 1
        raw_span(E, CANCEL_B, [0, 1], encode([1] * 5, True)),                       # an invalid (infinite-sum) slot
        raw_span(E, INF_SLOT, [0], encode([1, 1], True)),
        raw_span(E, CANCEL_B, [0, 2], encode([1] * 12, True)),                      # a slot loaded without members
        raw_span(E, PLAIN_SLOT, [0], nine),
        raw_span(E, PLAIN_SLOT, [1, 2], nine), raw_span(E, GAP, [0], b""),          # the gap
    ]
    for f, tag in ((good, "31"), (good8, "24")):
        v, l = encode([x for b in f.per for x in b], False), f.field
        M = sum(len(b) for b in f.per)
        strings = [v + b"\0", l + b"\0", v[:-1], b""]                               # one byte long, one short
        strings.append(l[:-1] if M % 8 else l[:-1] + b"\0")                         # (M % 8 == 0: no delimiter)
        for s in (v, l):
            top = 8 * len(s) - 1
            for pos in (M + 1, top):                                                # a stray bit above the delimiter
                if M < pos <= top:
                    t = bytearray(s)
                    t[pos >> 3] |= 1 << (pos & 7)
                    strings.append(bytes(t))
        cases += [raw_span(E, f.base, f.named, s) for s in strings]
    # a named committee without a participant: first, middle, last (a single-committee set included)
    for i in range(3):
        per = [b if j != i else [0] * len(b) for j, b in enumerate(good.per)]
        cases.append(Span(E, good.base, good.named, per, i % 2 == 0))
    cases.append(Span(E, 9, [0], [[0] * 33], True))
    assert len(cases) >= 30
    for bad in cases:
        check_rejected(G, L, E, REF, F, bad, BAD)
    # a short string as the LAST set of the call (its windows run past every row of the buffer)
    for s in (good.field[:-1], good.field[:1], b""):
        check_rejected(G, L, E, REF, F, raw_span(E, good.base, good.named, s), BAD, at=None)
    check_rejected(G, L, E, REF, F, raw_span(E, BIG_FIRST, list(range(8)), b"\xff" * 3), BAD, at=None)
    # plain sets keep their statuses
    check_rejected(G, L, E, REF, F, Span(E, plain=[]), G.AGGR_TYPE_MISMATCH)
    check_rejected(G, L, E, REF, F, Span(E, plain=[3, 10 ** 9]), BAD)


def test_argument_errors_fail_closed(G, L, REF, E, F):
    sets, want = neighbours(E, REF, F)
    n = len(sets)

    def variant(i, **kw):
        out = list(sets)
        s = Span(E, plain=[])
        s.__dict__.update(sets[i].__dict__)
        s.__dict__.update(kw)
        out[i] = s
        return out

    bad_calls = [variant(1, mask=mask_bytes([3])),              # a plain set with committee bits
                 variant(1, field=b"\x03"),                     # a plain set with aggregation bits
                 variant(0, lst=[3])]                           # a span set with a key range
    for bad in bad_calls:
        keys, st = span_keys(G, L, bad, expect_rc=G.VERIFY_FAIL)
        assert L.gbls_last_error() == 102
        assert st == [G.BAD_ENCODING] * n and keys == [bytes(96)] * n
        sst = G.i32_array(n)
        rc = L.gbls_multi_verify_spans(bytes(32 * n), bytes(96 * n), *spans_args(G, bad), u64([1] * n), n, sst, 0)
        assert (rc, L.gbls_last_error()) == (G.VERIFY_FAIL, 102) and [sst[i] for i in range(n)] == [G.BAD_ENCODING] * n
    # bits_off is required, and so are the masks
    com, masks, bits, boff, idx, off = spans_args(G, sets)
    out, st = ctypes.create_string_buffer(b"\xff" * (96 * n), 96 * n), G.i32_array(n)
    for args in ((com, masks, bits, None, idx, off), (com, None, bits, boff, idx, off)):
        assert L.gbls_g1_aggregate_spans(*args, n, out, st) == G.VERIFY_FAIL and L.gbls_last_error() == 102
        assert out.raw == bytes(96 * n) and [st[i] for i in range(n)] == [G.BAD_ENCODING] * n
        sst = G.i32_array(n)
        rc = L.gbls_multi_verify_spans(bytes(32 * n), bytes(96 * n), *args, u64([1] * n), n, sst, 0)
        assert (rc, L.gbls_last_error()) == (G.VERIFY_FAIL, 102) and [sst[i] for i in range(n)] == [G.BAD_ENCODING] * n
    # n == 0 is a verdict, not an error
    assert L.gbls_multi_verify_spans(bytes(32), bytes(96), com, masks, bits, boff, idx, off, u64([1]), 0, st, 0) == G.VERIFY_FAIL
    assert L.gbls_last_error() == 0
    assert span_keys(G, L, sets) == (want, [0] * n)


# ---------------------------------------------------------------- degenerate folds
def compress(G, L, sigs):
    n = len(sigs) // 192
    out = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, out), "compress")
    return out.raw


def test_twin_slots_double_and_opposite_contributions_cancel(G, L, REF, E, F):
    rng = random.Random("spans/degenerate")
    doubled = []
    for kind in ("full", "one-clear", "one-set", "half"):   # the same bits in both twins, in each direction
        b = committee_bits(12, kind, rng)
        doubled.append(Span(E, TWIN_A, [0, 1], [b, b], kind != "half"))
    cancel = Span(E, CANCEL_A, [0, 1], [[1, 0, 0], [1, 0, 0]], True)       # key 5 and its negation
    partly = Span(E, CANCEL_A, [0, 1], [[1, 1, 0], [1, 0, 1]], False)      # ... with keys 7 and 13 beside them
    sets = doubled + [cancel, partly]
    keys, st = span_keys(G, L, sets)
    assert st == [0] * len(sets)
    for s, k in zip(doubled, keys):
        assert k == oracle_key(REF, E, F, s.part) != bytes(96) and s.part[:len(s.part) // 2] == s.part[len(s.part) // 2:]
    assert keys[4] == bytes(96)   # infinity: all-zero with SUCCESS
    assert keys[5] == oracle_key(REF, E, F, [7, 13])
    # as a verification the infinite key fails the batch
    good = make_span(E, 0, [1, 2], rng)
    batch = [good, cancel]
    msgs = F.messages(2, b"spans/cancel")
    sigs = F.sign([sum(E.sks[v] for v in good.part) % F.R_ORDER, E.sks[7]], msgs)
    sst = G.i32_array(2)
    rc = L.gbls_multi_verify_spans(msgs, compress(G, L, sigs), *spans_args(G, batch), u64(F.rands(2, 5)), 2, sst, 0)
    assert (rc, [sst[0], sst[1]], L.gbls_last_error()) == (G.VERIFY_FAIL, [0, 0], 0)
    rc = L.gbls_multi_verify_spans(msgs, compress(G, L, sigs), *spans_args(G, [good]), u64(F.rands(2, 5)), 1, sst, 0)
    assert rc == G.SUCCESS


# ---------------------------------------------------------------- verdicts
class Batch:
    pass


def make_block(G, L, F, REF, E, msg_repeat=1):
    """A block: 8 span sets over the eight 512-member committees (absent per committee: 0, 5, 51 or
    256), 3 plain sets and a single-committee Bitvector set (the sync aggregate)."""
    b = Batch()
    rng = random.Random("spans/block")
    b.sets = []
    for i in range(8):
        per = []
        for c in range(BIG_N):
            absent = set(rng.sample(range(512), [0, 5, 51, 256][(i + c) % 4]))
            per.append([int(j not in absent) for j in range(512)])
        b.sets.append(Span(E, BIG_FIRST, list(range(BIG_N)), per, True))
    for i in (2, 5, 9):
        b.sets.insert(i, Span(E, plain=[(91 * i + 7) % NREG]))
    sync = set(rng.sample(range(512), 40))
    b.sets.append(Span(E, BIG_FIRST + 6, [0], [[int(j not in sync) for j in range(512)]], False))
    b.n = len(b.sets)
    k = b.n // msg_repeat
    um = F.messages(k, b"spans/block/%d" % msg_repeat)
    b.msgs = b"".join(um[32 * (i % k):32 * (i % k) + 32] for i in range(b.n))
    b.sigs = F.sign([sum(E.sks[v] for v in s.part) % F.R_ORDER for s in b.sets], b.msgs)
    b.pks = b"".join(oracle_key(REF, E, F, s.part) for s in b.sets)
    b.rands = F.rands(b.n, 4242)
    return b


def mv_spans(G, L, b, sets=None, sigs=None, comp=None, flags=0):
    st = G.i32_array(b.n)
    comp = compress(G, L, b.sigs if sigs is None else sigs) if comp is None else comp
    rc = L.gbls_multi_verify_spans(b.msgs, comp, *spans_args(G, b.sets if sets is None else sets), u64(b.rands), b.n,
                                   st, flags)
    return rc, [st[i] for i in range(b.n)], L.gbls_last_error()


def mv_lists(G, L, b, sets=None, sigs=None, comp=None, flags=0):
    """The same sets through gbls_multi_verify_compressed_ex over explicit participant lists."""
    idx, off = flat([s.part for s in (b.sets if sets is None else sets)])
    st = G.i32_array(b.n)
    comp = compress(G, L, b.sigs if sigs is None else sigs) if comp is None else comp
    rc = L.gbls_multi_verify_compressed_ex(b.msgs, comp, None, G.u32_array(idx), G.u32_array(off), u64(b.rands), b.n,
                                           st, flags)
    return rc, [st[i] for i in range(b.n)], L.gbls_last_error()


def ref_mv(REF, E, F, b, sets=None, sigs=None):
    pks = b.pks if sets is None else b"".join(oracle_key(REF, E, F, s.part) for s in sets)
    return bool(REF.ref_multi_verify(b.msgs, b.sigs if sigs is None else sigs, pks, u64(b.rands), b.n, 16))


def swapped(b, i=1, j=7):
    s = bytearray(b.sigs)
    s[192 * i:192 * i + 192], s[192 * j:192 * j + 192] = b.sigs[192 * j:192 * j + 192], b.sigs[192 * i:192 * i + 192]
    return bytes(s)


@pytest.fixture(scope="module")
def block(G, L, F, REF, E):
    return make_block(G, L, F, REF, E)


@pytest.mark.parametrize("flags", [0, 1])  # 1: GBLS_CALL_BLOCK
def test_block_verdicts(G, L, REF, E, F, block, flags):
    b = block
    ok = [0] * b.n
    assert b.n == 12 and sum(s.base is None for s in b.sets) == 3 and b.sets[-1].bitlist is False
    assert ref_mv(REF, E, F, b)
    assert mv_spans(G, L, b, flags=flags) == mv_lists(G, L, b, flags=flags) == (G.SUCCESS, ok, 0)
    sw = swapped(b)
    assert not ref_mv(REF, E, F, b, sigs=sw)
    assert mv_spans(G, L, b, sigs=sw, flags=flags) == mv_lists(G, L, b, sigs=sw, flags=flags) == (G.VERIFY_FAIL, ok, 0)

    def tampered(k, s):
        return b.sets[:k] + [s] + b.sets[k + 1:]

    k = 3
    t = b.sets[k]
    assert t.base == BIG_FIRST and len(t.named) == 8
    # one non-signer's bit set
    c = next(i for i, bits in enumerate(t.per) if not all(bits))
    per = [list(x) for x in t.per]
    per[c][per[c].index(0)] = 1
    # a committee bit cleared and a committee bit added, the string following the mask
    cleared = Span(E, t.base, t.named[:4] + t.named[5:], t.per[:4] + t.per[5:], True)
    added = Span(E, t.base - 1, [0] + [c + 1 for c in t.named], [[1] * len(E.members[t.base - 1])] + t.per, True)
    for s in (Span(E, t.base, t.named, per, True), cleared, added):
        sets = tampered(k, s)
        assert not ref_mv(REF, E, F, b, sets=sets)
        assert mv_spans(G, L, b, sets=sets, flags=flags) == mv_lists(G, L, b, sets=sets, flags=flags) == (G.VERIFY_FAIL, ok, 0)
    # ... and the mask alone changed: the string no longer fits the named committees
    for named in (t.named[:4] + t.named[5:], t.named + [8]):
        assert mv_spans(G, L, b, sets=tampered(k, raw_span(E, t.base, named, t.field)), flags=flags) == (G.VERIFY_FAIL, ok, 0)
    # a signature that does not decode is returned first, with the statuses of the lists call
    comp = bytearray(compress(G, L, sw))
    comp[96 * 6] &= 0x7F  # the compression flag
    rc, st, err = mv_spans(G, L, b, comp=bytes(comp), flags=flags)
    assert (rc, st, err) == mv_lists(G, L, b, comp=bytes(comp), flags=flags)
    assert rc == st[6] != G.SUCCESS and [x for i, x in enumerate(st) if i != 6] == [0] * (b.n - 1)


@contextlib.contextmanager
def dedup_policy(L, G):
    prev = L.gbls_set_policy(0)
    L.gbls_set_policy(prev | G.INIT_DEDUP)
    try:
        yield
    finally:
        L.gbls_set_policy(prev)


def test_dedup_and_message_cache(G, L, F, REF, E, block):
    rep = make_block(G, L, F, REF, E, msg_repeat=4)
    assert len(set(rep.msgs[32 * i:32 * i + 32] for i in range(rep.n))) == 3
    assert (ref_mv(REF, E, F, rep), ref_mv(REF, E, F, rep, sigs=swapped(rep))) == (True, False)
    for b in (block, rep):
        with dedup_policy(L, G):
            assert mv_spans(G, L, b) == mv_lists(G, L, b) == (G.SUCCESS, [0] * b.n, 0)
            assert mv_spans(G, L, b, sigs=swapped(b)) == mv_lists(G, L, b, sigs=swapped(b)) == (G.VERIFY_FAIL, [0] * b.n, 0)
    # the message line cache, cold then warm
    out = (ctypes.c_uint64 * 8)()
    assert L.gbls_msgcache_configure(256) == 0
    try:
        for b, distinct in ((block, 12), (rep, 3)):
            assert L.gbls_msgcache_stats(out) == 0
            hits0, miss0 = out[1], out[2]
            assert mv_spans(G, L, b) == (G.SUCCESS, [0] * b.n, 0)             # cold
            assert L.gbls_msgcache_stats(out) == 0 and (out[1] - hits0, out[2] - miss0) == (0, distinct)
            assert mv_spans(G, L, b) == (G.SUCCESS, [0] * b.n, 0)             # warm
            assert L.gbls_msgcache_stats(out) == 0 and (out[1] - hits0, out[2] - miss0) == (distinct, distinct)
            assert mv_spans(G, L, b, sigs=swapped(b)) == (G.VERIFY_FAIL, [0] * b.n, 0)
    finally:
        assert L.gbls_msgcache_configure(0) == 0


# ---------------------------------------------------------------- the forms, replicas
def child(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_spans_child.py")] + list(args),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_launch_forms_give_the_same_bytes_subprocess():
    """GBLS_COMMITTEE_ROW_MIN (read under GBLS_INIT_TUNING in a fresh engine): every piece on rows,
    and every piece on single lanes, give the keys of the indexed sum, byte for byte."""
    rows = child("switch", "GBLS_COMMITTEE_ROW_MIN=1")
    lanes = child("switch", "GBLS_COMMITTEE_ROW_MIN=1000000")
    for res in (rows, lanes):
        assert res["sets"] >= 60 and res["equal"] == res["sets"] and res["longest"] >= 12
    assert rows["digest"] == lanes["digest"]


def test_replicas_subprocess():
    """Two engines on the one GPU: a 4200-set one-segment batch of two-committee spans takes the
    sharded-partials path of verify_host, each engine resolving its shard's slice of the masks and
    the bits against its own member blocks."""
    res = child("replicas")
    assert res["engines"] == 2 and res["big"] == [0, 5] and res["big_err"] == [0, 0]


# ---------------------------------------------------------------- the Python mirror
def test_python_mirror_takes_the_spans_path(G, L, F, REF, E, block):
    from grandine_amd import bls as B
    from grandine_amd import verifier as V
    b = block
    keys48 = [E.comp[48 * i:48 * i + 48] for i in range(NREG + 1)]
    B.Registry.forget()
    try:
        B.Registry.mirror_finalized(keys48)  # first = 0 rewrites the registry: the table is cleared
        assert B.Committees.size() == 0
        raw = F.public_keys(E.sks)
        pk = [B.PublicKey(raw[96 * v:96 * v + 96]) for v in range(NREG + 1)]
        coms = [E.members[BIG_FIRST + c] for c in range(BIG_N)]

        def run(sigs, members, single_as_committee=True):
            assert B.Committees.set(BIG_FIRST, coms, members=members) == [0] * BIG_N
            mv = V.MultiVerifier()
            comp = compress(G, L, sigs)
            for i, s in enumerate(b.sets):
                msg, sig = b.msgs[32 * i:32 * i + 32], comp[96 * i:96 * i + 96]
                keys = [pk[v] for v in s.part]
                if s.base is None:
                    mv.verify_aggregate_indexed(msg, sig, s.lst, keys, None)
                elif len(s.named) == 1 and single_as_committee:
                    mv.verify_aggregate_committee(msg, sig, s.base, E.members[s.base], s.field, keys, None)
                else:
                    mv.verify_aggregate_committees(msg, sig, s.base, s.mask, [E.members[s.base + c] for c in s.named],
                                                   s.field, keys, None)
            try:
                mv.finish(randoms=b.rands)
                return mv.last_path, True
            except V.SignatureInvalid:
                return mv.last_path, False

        assert run(b.sigs, True) == ("spans", ref_mv(REF, E, F, b)) == ("spans", True)
        assert run(swapped(b), True) == ("spans", ref_mv(REF, E, F, b, sigs=swapped(b))) == ("spans", False)
        assert run(b.sigs, True, single_as_committee=False) == ("spans", True)
        # the same triples with the slots loaded without members: the indexed path, same verdicts
        assert run(b.sigs, False, single_as_committee=False) == ("indices", True)
        assert run(swapped(b), False, single_as_committee=False) == ("indices", False)
    finally:
        B.Registry.forget()
        load_all(G, L, F)
