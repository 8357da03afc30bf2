"""Aggregation-bit sets on the GPU (include/grandine_bls_gpu_bits.h): committee slots with resident
member lists, keys chosen on the device from a slot and the SSZ bits as they arrive, batch
verification over such keys mixed with plain registry-indexed sets, rejections, rewrites, replicas
and concurrent rewrites, and the Python mirror.

The secret keys are known, so the oracle's key of a set is ref_sk_to_pk(sum of the participants'
secret keys mod r) and every comparison is byte for byte or verdict for verdict.

Launch forms crossed here: k_g1_bits_keys runs one lane per set (64 sets per block) while the
longest set of the launch adds fewer than kCommitteeRowMin keys (min(participants, absentees) of a
committee set, a plain set's list), and one 16-lane row per set (4 per block) from there on; the
child script forces each form over the same sets."""
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
SIZES = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 512, 2048]
PATTERNS = ["all", "none", "one-set", "one-clear", "alternating", "half", "half+1", "random-a", "random-b"]
LAUNCHES = [1, 3, 4, 5, 64, 65, 130]   # sets per launch (then the rest of the 288 combinations)
GAP = 16            # never written
X_SLOT, INF_SLOT, EMPTY_SLOT, BADIDX_SLOT = 17, 18, 19, 20   # the second load, slots 17..24
DBL_SLOT, IDN_SLOT = 21, 22
PLAIN_SLOT, DROPPED_SLOT = 25, 26
BIG_FIRST, BIG_N = 30, 8   # eight 512-member committees
TABLE_SIZE = BIG_FIRST + BIG_N


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


def pattern_bits(m, name):
    rng = random.Random("%d/%s" % (m, name))
    if name == "all":
        return [1] * m
    if name == "none":
        return [0] * m
    if name == "one-set":
        return [int(j == (2 * m) // 3) for j in range(m)]
    if name == "one-clear":
        return [int(j != m // 3) for j in range(m)]
    if name == "alternating":
        return [j & 1 for j in range(m)]
    if name in ("half", "half+1"):  # exactly half (the tie: participants) and one more (absentees)
        chosen = set(rng.sample(range(m), min(m, m // 2 + (name == "half+1"))))
        return [int(j in chosen) for j in range(m)]
    return [int(rng.random() < (0.9 if name == "random-a" else 0.3)) for j in range(m)]


def encode(bits, bitlist):
    m = len(bits)
    out = bytearray(m // 8 + 1 if bitlist else (m + 7) // 8)
    for j, b in enumerate(bits):
        out[j >> 3] |= b << (j & 7)
    if bitlist:
        out[m >> 3] |= 1 << (m & 7)
    return bytes(out)


class Env:
    pass


def load_all(G, L, F):
    """Registry (first = 0) and the committee table; returns the statuses of each load."""
    from grandine_amd import bls as B
    B.Registry.forget()
    E = Env()
    E.sks, comp = F.registry(NREG, seed=b"bits")
    E.sks = E.sks + [F.R_ORDER - E.sks[5]]
    comp += F.compress_g1(F.public_keys(E.sks[NREG:]))
    assert not F.load_registry(comp).any()
    assert L.gbls_registry_size() >= NREG + 1
    E.comp = comp
    E.members = {}
    a = [members_of(c, SIZES[c]) for c in range(len(SIZES))]
    E.load_a = set_call(G, L, 0, a)
    E.size_a = L.gbls_committees_size()
    b = {X_SLOT: [5, NEG5, 7], INF_SLOT: [5, NEG5], EMPTY_SLOT: [], BADIDX_SLOT: [1, 2, 10 ** 9, 3],
         DBL_SLOT: [5, 5, NEG5], IDN_SLOT: [5, NEG5, 5], 23: members_of(77, 12), 24: members_of(78, 40)}
    E.load_b = set_call(G, L, X_SLOT, [b[s] for s in range(X_SLOT, 25)])
    E.load_c = set_call(G, L, PLAIN_SLOT, [members_of(80, 9)], members=False)
    E.load_d = (set_call(G, L, DROPPED_SLOT, [members_of(81, 9)]), L.gbls_committees_members(DROPPED_SLOT),
                set_call(G, L, DROPPED_SLOT, [members_of(81, 9)], members=False))
    big = [members_of(200 + c, 512) for c in range(BIG_N)]
    E.load_e = set_call(G, L, BIG_FIRST, big)
    for c, m in enumerate(a):
        E.members[c] = m
    for s in (X_SLOT, DBL_SLOT, IDN_SLOT, 23, 24):
        E.members[s] = b[s]
    for c, m in enumerate(big):
        E.members[BIG_FIRST + c] = m
    E.sum_only = {PLAIN_SLOT: members_of(80, 9), DROPPED_SLOT: members_of(81, 9)}
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


def bits_args(G, slots, fields, lists):
    idx, off = flat(lists)
    _, boff = flat(fields)
    return (G.u32_array([G.NO_COMMITTEE if s is None else s for s in slots]), G.buf(b"".join(fields)),
            G.u32_array(boff), G.u32_array(idx or [0]), G.u32_array(off))


def bits_keys(G, L, slots, fields, lists=None, expect_rc=0):
    n = len(slots)
    lists = [[] for _ in slots] if lists is None else lists
    out = ctypes.create_string_buffer(b"\xff" * (96 * n), 96 * n)
    st = G.i32_array(n)
    rc = L.gbls_g1_aggregate_bits(*bits_args(G, slots, fields, lists), n, out, st)
    assert rc == expect_rc, (rc, L.gbls_last_error())
    return [out.raw[96 * i:96 * i + 96] for i in range(n)], [st[i] for i in range(n)]


def committee_keys(G, L, slots, lists):
    n = len(slots)
    idx, off = flat(lists)
    out = ctypes.create_string_buffer(96 * n)
    st = G.i32_array(n)
    rc = L.gbls_g1_aggregate_committees(G.u32_array([G.NO_COMMITTEE if s is None else s for s in slots]),
                                        G.u32_array(idx or [0]), G.u32_array(off), n, out, st)
    assert rc == G.SUCCESS, (rc, L.gbls_last_error())
    return [out.raw[96 * i:96 * i + 96] for i in range(n)], [st[i] for i in range(n)]


# ---------------------------------------------------------------- the table
def test_loads_and_member_counts(G, L, E):
    assert E.load_a == (G.SUCCESS, [G.SUCCESS] * len(SIZES)) and E.size_a == len(SIZES)
    # {5, -5}: an infinite sum is a SUCCESS stored all-zero (an invalid slot); the empty committee and
    # the one naming index 10^9 are rejected
    assert E.load_b == (G.SUCCESS, [0, 0, G.AGGR_TYPE_MISMATCH, G.BAD_ENCODING, 0, 0, 0, 0])
    assert E.load_c == (G.SUCCESS, [0]) and E.load_e == (G.SUCCESS, [0] * BIG_N)
    assert E.load_d == ((G.SUCCESS, [0]), 9, (G.SUCCESS, [0]))
    assert L.gbls_committees_size() == TABLE_SIZE
    count = [L.gbls_committees_members(s) for s in range(TABLE_SIZE + 2)]
    for s in range(TABLE_SIZE + 2):
        want = len(E.members[s]) if s in E.members else 2 if s == INF_SLOT else 0
        assert count[s] == want, s   # the gap, rejected slots, plain and dropped slots, past the table: 0
    # the sums are those of gbls_committees_set: the slots read back through the committees call
    keys, st = committee_keys(G, L, [3, PLAIN_SLOT, DROPPED_SLOT, GAP], [[], [], [], []])
    assert st == [0, 0, 0, G.BAD_ENCODING]


# ---------------------------------------------------------------- 5. keys
def all_combinations(E):
    """(slot, bits, encoding) for every size, pattern and encoding: 288 sets."""
    out = []
    for c, m in enumerate(SIZES):
        for name in PATTERNS:
            bits = pattern_bits(m, name)
            for bitlist in (False, True):
                out.append((c, bits, encode(bits, bitlist)))
    return out


@pytest.fixture(scope="module")
def combos(REF, E, F):
    sets = all_combinations(E)
    want = [oracle_key(REF, E, F, [v for v, b in zip(E.members[s], bits) if b]) for s, bits, _ in sets]
    return sets, want


def test_keys_equal_oracle_and_committees_call(G, L, E, combos):
    sets, want = combos
    assert len(sets) == 288
    pos, launches = 0, []
    for n in LAUNCHES + [len(sets) - sum(LAUNCHES)]:
        launches.append(sets[pos:pos + n])
        pos += n
    assert pos == len(sets)
    got = []
    for chunk in launches:
        keys, st = bits_keys(G, L, [s for s, _, _ in chunk], [f for _, _, f in chunk])
        assert st == [0] * len(chunk)
        got += keys
    for i, (s, bits, field) in enumerate(sets):
        assert got[i] == want[i], (i, len(bits), sum(bits), len(field))
        if not any(bits):
            assert got[i] == bytes(96)   # no participant: infinity, all-zero with SUCCESS
    # the committees call on the equivalent explicit lists, in both of its forms
    absent = [[v for v, b in zip(E.members[s], bits) if not b] for s, bits, _ in sets]
    part = [[v for v, b in zip(E.members[s], bits) if b] for s, bits, _ in sets]
    k1, st1 = committee_keys(G, L, [s for s, _, _ in sets], absent)
    k2, st2 = committee_keys(G, L, [None] * len(sets), part)
    assert st1 == [0] * len(sets) and k1 == got
    for i in range(len(sets)):
        assert (st2[i], k2[i]) == ((0, got[i]) if part[i] else (G.AGGR_TYPE_MISMATCH, bytes(96))), i


def test_whole_table_in_one_launch_with_plain_sets(G, L, REF, E, F, combos):
    """All 288 combinations and 32 plain sets in one launch (the row form: the longest set adds
    1024 keys), the plain sets between the committee sets."""
    sets, want = combos
    slots, fields, lists, expect = [], [], [], []
    for i, (s, bits, field) in enumerate(sets):
        slots.append(s)
        fields.append(field)
        lists.append([])
        expect.append(want[i])
        if i % 9 == 4:
            plain = members_of(300 + i, 1 + i % 20)
            slots.append(None)
            fields.append(b"")
            lists.append(plain)
            expect.append(oracle_key(REF, E, F, plain))
    keys, st = bits_keys(G, L, slots, fields, lists)
    assert st == [0] * len(slots) and keys == expect


def test_odd_byte_lengths_start_unaligned(G, L, E, combos):
    """Consecutive bit strings of 1, 3, 5, 9 and 33 bytes: most start at an odd offset, the last
    one ends the buffer."""
    sets, want = combos
    odd = [i for i, (_, _, f) in enumerate(sets) if len(f) % 2 == 1]
    pick = odd[::4]
    assert len(pick) >= 40 and {len(sets[i][2]) for i in pick} >= {1, 3, 5, 9, 33}
    starts, pos = [], 0
    for i in pick:
        starts.append(pos)
        pos += len(sets[i][2])
    assert sum(s % 4 != 0 for s in starts) > len(pick) // 2
    keys, st = bits_keys(G, L, [sets[i][0] for i in pick], [sets[i][2] for i in pick])
    assert st == [0] * len(pick) and keys == [want[i] for i in pick]


def test_key_and_its_negation(G, L, REF, E, F):
    p5_7, two_p5 = oracle_key(REF, E, F, [5, 7]), oracle_key(REF, E, F, [5, 5])
    slots = [INF_SLOT, X_SLOT, X_SLOT, DBL_SLOT, IDN_SLOT, X_SLOT]
    fields = [encode([1, 0], True), encode([1, 0, 1], True), encode([1, 1, 0], False), encode([1, 1, 0], True),
              encode([1, 1, 0], False), encode([0, 0, 1], True)]
    keys, st = bits_keys(G, L, slots, fields)
    # {5, -5}: the whole sum is infinite, the slot is invalid whatever the bits select
    assert (st[0], keys[0]) == (G.BAD_ENCODING, bytes(96))
    # {5, -5, 7}, C = key 7: bits {5, 7} subtract -5: the generic final addition
    assert (st[1], keys[1]) == (0, p5_7)
    # ... bits {5, -5} subtract 7: C - C, the identity, written all-zero with SUCCESS
    assert (st[2], keys[2]) == (0, bytes(96))
    # {5, 5, -5}, C = key 5: bits {5, 5} subtract -5: C + C, a doubling
    assert (st[3], keys[3]) == (0, two_p5)
    # {5, -5, 5}, C = key 5: bits {5, -5} subtract 5: the identity
    assert (st[4], keys[4]) == (0, bytes(96))
    # the participants' direction: one of three
    assert (st[5], keys[5]) == (0, oracle_key(REF, E, F, [7]))


# ---------------------------------------------------------------- 6. rejections
def valid_sets(E, REF, F):
    sets = [(4, pattern_bits(15, "one-clear"), True), (23, pattern_bits(12, "alternating"), False),
            (10, pattern_bits(63, "random-a"), True), (24, pattern_bits(40, "half"), True),
            (13, pattern_bits(257, "one-clear"), False)]
    slots = [s for s, _, _ in sets]
    fields = [encode(b, l) for _, b, l in sets]
    want = [oracle_key(REF, E, F, [v for v, x in zip(E.members[s], b) if x]) for s, b, _ in sets]
    return slots, fields, want


def check_one_rejected(G, L, E, REF, F, slot, field, status, lst=None, plain=False):
    slots, fields, want = valid_sets(E, REF, F)
    slots.insert(2, None if plain else slot)
    fields.insert(2, field)
    want.insert(2, bytes(96))
    lists = [[] for _ in slots]
    if lst is not None:
        lists[2] = lst
    keys, st = bits_keys(G, L, slots, fields, lists)
    assert st == [0, 0, status, 0, 0, 0] and keys == want, (slot, field.hex())


def test_malformed_bit_strings(G, L, REF, E, F):
    def flip(field, pos):
        t = bytearray(field)
        t[pos >> 3] |= 1 << (pos & 7)
        return bytes(t)

    cases = []
    for slot, m in ((4, 15), (5, 16), (6, 17), (9, 33), (14, 512)):
        bits = pattern_bits(m, "random-a")
        v, l = encode(bits, False), encode(bits, True)
        cases += [(slot, v + b"\0"), (slot, l + b"\0"), (slot, v[:-1])]      # one byte long, one short
        if m % 8:
            cases.append((slot, l[:-1]))
        else:
            cases.append((slot, l[:-1] + b"\0"))                              # the long form without its delimiter
        for s in (v, l):
            top = 8 * len(s) - 1
            for pos in (m + 1, top):                                          # a stray bit above position m
                if m < pos <= top:
                    cases.append((slot, flip(s, pos)))
        if m % 8 and m % 8 != 7:
            cases.append((slot, flip(flip(v, m), m + 1)))                     # at m and above it
    assert len(cases) >= 30
    for slot, field in cases:
        check_one_rejected(G, L, E, REF, F, slot, field, G.BAD_ENCODING)
    # position m itself: the two encodings have one length when m % 8 != 0 and bit m decides, so a
    # Bitvector with bit m set IS the Bitlist of the same members
    bits = pattern_bits(17, "random-a")
    keys, st = bits_keys(G, L, [6, 6], [flip(encode(bits, False), 17), encode(bits, True)])
    assert st == [0, 0] and keys[0] == keys[1] == oracle_key(REF, E, F, [v for v, b in zip(E.members[6], bits) if b])


def test_rejected_slots(G, L, REF, E, F):
    nine = encode([1] * 9, True)
    for slot, field in ((TABLE_SIZE, nine), (TABLE_SIZE + 1000, nine), (1 << 24, nine),   # past the table
                        (GAP, nine), (GAP, b""),                                          # never written
                        (PLAIN_SLOT, nine), (PLAIN_SLOT, encode([1] * 9, False)),         # a sum without members
                        (EMPTY_SLOT, b""), (EMPTY_SLOT, b"\x01"),                         # load status nonzero
                        (BADIDX_SLOT, encode([1] * 4, True)), (BADIDX_SLOT, encode([1, 1, 0, 0], False)),
                        (DROPPED_SLOT, nine),                                             # dropped by a plain set
                        (INF_SLOT, encode([1, 1], True))):
        check_one_rejected(G, L, E, REF, F, slot, field, G.BAD_ENCODING)
    # a plain set: an empty list, a bad index
    check_one_rejected(G, L, E, REF, F, None, b"", G.AGGR_TYPE_MISMATCH, lst=[], plain=True)
    check_one_rejected(G, L, E, REF, F, None, b"", G.BAD_ENCODING, lst=[3, 10 ** 9], plain=True)


def test_argument_errors_fail_closed(G, L, REF, E, F):
    slots, fields, want = valid_sets(E, REF, F)
    n = len(slots)
    # a committee set with an index range; a plain set with bits
    for bad_slots, bad_fields, bad_lists in ((slots, fields, [[], [3], [], [], []]),
                                            (slots[:2] + [None] + slots[3:], fields, [[], [], [4], [], []])):
        keys, st = bits_keys(G, L, bad_slots, bad_fields, bad_lists, expect_rc=G.VERIFY_FAIL)
        assert L.gbls_last_error() == 102
        assert st == [G.BAD_ENCODING] * n and keys == [bytes(96)] * n
        sst = G.i32_array(n)
        rc = L.gbls_multi_verify_bits(bytes(32 * n), bytes(96 * n), *bits_args(G, bad_slots, bad_fields, bad_lists),
                                      u64([1] * n), n, sst, 0)
        assert (rc, L.gbls_last_error()) == (G.VERIFY_FAIL, 102) and [sst[i] for i in range(n)] == [G.BAD_ENCODING] * n
    # pk_idx / pk_off may be NULL when no set is plain
    com, bits, boff, _, _ = bits_args(G, slots, fields, [[] for _ in slots])
    out, st = ctypes.create_string_buffer(96 * n), G.i32_array(n)
    assert L.gbls_g1_aggregate_bits(com, bits, boff, None, None, n, out, st) == 0
    assert [out.raw[96 * i:96 * i + 96] for i in range(n)] == want
    # bits_off is required; n == 0 is a verdict
    assert L.gbls_g1_aggregate_bits(com, bits, None, None, None, n, out, st) == G.VERIFY_FAIL and L.gbls_last_error() == 102
    assert L.gbls_multi_verify_bits(bytes(32), bytes(96), com, bits, boff, None, None, u64([1]), 0, st, 0) == G.VERIFY_FAIL
    assert L.gbls_last_error() == 0


# ---------------------------------------------------------------- 7. verdicts
class Batch:
    pass


def make_batch(G, L, F, REF, E, kind, msg_repeat=1):
    """slot: 64 sets over the eight 512-member committees, about 5 % absent.  block: 48 sets, every
    fourth a plain single-key set (the proposer, RANDAO, exits), the others committees of mixed
    sizes and both encodings."""
    b = Batch()
    rng = random.Random("batch/" + kind)
    b.n = 64 if kind == "slot" else 48
    b.slots, b.fields, b.lists, b.parts, b.absent = [], [], [], [], []
    mixed = [2, 4, 6, 9, 11, 12, 13, 14, 23, 24, BIG_FIRST, BIG_FIRST + 3]
    for i in range(b.n):
        if kind == "block" and i % 4 == 3:
            v = [(91 * i + 7) % NREG]
            b.slots.append(None), b.fields.append(b""), b.lists.append(v), b.parts.append(v), b.absent.append(None)
            continue
        s = BIG_FIRST + i % BIG_N if kind == "slot" else mixed[i % len(mixed)]
        m = E.members[s]
        bits = [int(rng.random() < (0.95 if i % 5 else 0.4)) for _ in m]
        bits[i % len(m)] = 1
        b.slots.append(s), b.fields.append(encode(bits, i % 2 == 0)), b.lists.append([])
        b.parts.append([v for v, x in zip(m, bits) if x])
        b.absent.append([v for v, x in zip(m, bits) if not x])
    um = F.messages(b.n // msg_repeat, b"bits/%s/%d" % (kind.encode(), msg_repeat))
    k = b.n // msg_repeat
    b.msgs = b"".join(um[32 * (i % k):32 * (i % k) + 32] for i in range(b.n))
    b.sigs = F.sign([sum(E.sks[v] for v in p) % F.R_ORDER for p in b.parts], b.msgs)
    b.pks = b"".join(oracle_key(REF, E, F, p) for p in b.parts)
    b.rands = F.rands(b.n, 777)
    return b


def compress(G, L, sigs):
    n = len(sigs) // 192
    out = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, out), "compress")
    return out.raw


def mv_bits(G, L, b, sigs=None, slots=None, fields=None, flags=0, comp=None):
    st = G.i32_array(b.n)
    comp = compress(G, L, b.sigs if sigs is None else sigs) if comp is None else comp
    rc = L.gbls_multi_verify_bits(b.msgs, comp, *bits_args(G, b.slots if slots is None else slots,
                                                           b.fields if fields is None else fields, b.lists),
                                  u64(b.rands), b.n, st, flags)
    return rc, [st[i] for i in range(b.n)], L.gbls_last_error()


def mv_committees(G, L, b, sigs=None, comp=None, flags=0):
    """The same sets through the committees call: absentee lists for the committee sets."""
    idx, off = flat([b.lists[i] if b.slots[i] is None else b.absent[i] for i in range(b.n)])
    st = G.i32_array(b.n)
    comp = compress(G, L, b.sigs if sigs is None else sigs) if comp is None else comp
    rc = L.gbls_multi_verify_committees(b.msgs, comp, G.u32_array([G.NO_COMMITTEE if s is None else s for s in b.slots]),
                                        G.u32_array(idx or [0]), G.u32_array(off), u64(b.rands), b.n, st, flags)
    return rc, [st[i] for i in range(b.n)], L.gbls_last_error()


def ref_mv(REF, b, sigs=None, pks=None):
    return bool(REF.ref_multi_verify(b.msgs, b.sigs if sigs is None else sigs, b.pks if pks is None else pks,
                                     u64(b.rands), b.n, 16))


def swapped(b, i=4, j=29):
    s = bytearray(b.sigs)
    s[192 * i:192 * i + 192], s[192 * j:192 * j + 192] = b.sigs[192 * j:192 * j + 192], b.sigs[192 * i:192 * i + 192]
    return bytes(s)


@pytest.fixture(scope="module")
def slot_batch(G, L, F, REF, E):
    return make_batch(G, L, F, REF, E, "slot")


@pytest.fixture(scope="module")
def block_batch(G, L, F, REF, E):
    return make_batch(G, L, F, REF, E, "block")


def test_slot_shape_verdicts(G, L, REF, slot_batch):
    b = slot_batch
    ok = [0] * b.n
    assert ref_mv(REF, b) and mv_bits(G, L, b) == mv_committees(G, L, b) == (G.SUCCESS, ok, 0)
    sw = swapped(b)
    assert not ref_mv(REF, b, sigs=sw) and mv_bits(G, L, b, sigs=sw) == mv_committees(G, L, b, sigs=sw) == (G.VERIFY_FAIL, ok, 0)


@pytest.mark.parametrize("flags", [0, 1])  # 1: GBLS_CALL_BLOCK
def test_block_shape_verdicts(G, L, REF, E, F, block_batch, flags):
    b = block_batch
    ok = [0] * b.n
    assert sum(s is None for s in b.slots) == 12
    assert ref_mv(REF, b) and mv_bits(G, L, b, flags=flags) == mv_committees(G, L, b, flags=flags) == (G.SUCCESS, ok, 0)
    sw = swapped(b)
    assert not ref_mv(REF, b, sigs=sw)
    assert mv_bits(G, L, b, sigs=sw, flags=flags) == mv_committees(G, L, b, sigs=sw, flags=flags) == (G.VERIFY_FAIL, ok, 0)
    # one bit more than signed: the key includes a non-signer
    k = next(i for i in range(b.n) if b.slots[i] is not None and b.absent[i])
    m = E.members[b.slots[k]]
    j = m.index(b.absent[k][0])
    f = bytearray(b.fields[k])
    f[j >> 3] |= 1 << (j & 7)
    fields = b.fields[:k] + [bytes(f)] + b.fields[k + 1:]
    pks = b.pks[:96 * k] + oracle_key(REF, E, F, b.parts[k] + [m[j]]) + b.pks[96 * (k + 1):]
    assert not ref_mv(REF, b, pks=pks) and mv_bits(G, L, b, fields=fields, flags=flags) == (G.VERIFY_FAIL, ok, 0)
    # no bit set: an infinite key fails the batch; a malformed string fails it too, sig_status all SUCCESS
    for field in (encode([0] * len(m), True), b.fields[k] + b"\0", b"\xff" * (len(b.fields[k]) + 2)):
        fields = b.fields[:k] + [field] + b.fields[k + 1:]
        assert mv_bits(G, L, b, fields=fields, flags=flags) == (G.VERIFY_FAIL, ok, 0), field.hex()
    # a slot without members fails the batch
    slots = b.slots[:k] + [PLAIN_SLOT] + b.slots[k + 1:]
    assert mv_bits(G, L, b, slots=slots, flags=flags) == (G.VERIFY_FAIL, ok, 0)
    # a signature that does not decode is returned first, with the statuses of the committees call
    comp = bytearray(compress(G, L, sw))
    comp[96 * 17] &= 0x7F  # the compression flag
    rc, st, err = mv_bits(G, L, b, comp=bytes(comp), flags=flags)
    assert (rc, st, err) == mv_committees(G, L, b, comp=bytes(comp), flags=flags)
    assert rc == st[17] != G.SUCCESS and [x for i, x in enumerate(st) if i != 17] == [0] * (b.n - 1)


@contextlib.contextmanager
def dedup_policy(L, G):
    prev = L.gbls_set_policy(0)
    L.gbls_set_policy(prev | G.INIT_DEDUP)
    try:
        yield
    finally:
        L.gbls_set_policy(prev)


def test_dedup_and_message_cache(G, L, F, REF, E, block_batch):
    rep = make_batch(G, L, F, REF, E, "block", msg_repeat=4)
    assert len(set(rep.msgs[32 * i:32 * i + 32] for i in range(rep.n))) == 12
    assert (ref_mv(REF, rep), ref_mv(REF, rep, sigs=swapped(rep))) == (True, False)
    for b in (block_batch, rep):
        with dedup_policy(L, G):
            assert mv_bits(G, L, b) == mv_committees(G, L, b) == (G.SUCCESS, [0] * b.n, 0)
            assert mv_bits(G, L, b, sigs=swapped(b)) == (G.VERIFY_FAIL, [0] * b.n, 0)
    # the message line cache, cold then warm
    out = (ctypes.c_uint64 * 8)()
    assert L.gbls_msgcache_configure(256) == 0
    try:
        for b, distinct in ((block_batch, 48), (rep, 12)):
            assert L.gbls_msgcache_stats(out) == 0
            hits0, miss0 = out[1], out[2]
            assert mv_bits(G, L, b) == (G.SUCCESS, [0] * b.n, 0)             # cold
            assert L.gbls_msgcache_stats(out) == 0 and (out[1] - hits0, out[2] - miss0) == (0, distinct)
            assert mv_bits(G, L, b) == (G.SUCCESS, [0] * b.n, 0)             # warm
            assert L.gbls_msgcache_stats(out) == 0 and (out[1] - hits0, out[2] - miss0) == (distinct, distinct)
            assert mv_bits(G, L, b, sigs=swapped(b)) == (G.VERIFY_FAIL, [0] * b.n, 0)
    finally:
        assert L.gbls_msgcache_configure(0) == 0


# ---------------------------------------------------------------- 8. a slot rewritten with another size
def test_slot_rewritten_with_another_size(G, L, REF, E, F):
    old = E.members[3]                      # 9 members
    new = members_of(991, 40)
    old_bits, new_bits = pattern_bits(9, "one-clear"), pattern_bits(40, "random-a")
    fo, fn = encode(old_bits, True), encode(new_bits, True)
    want_old = oracle_key(REF, E, F, [v for v, b in zip(old, old_bits) if b])
    want_new = oracle_key(REF, E, F, [v for v, b in zip(new, new_bits) if b])
    try:
        assert bits_keys(G, L, [3, 2, 3], [fo, encode([1] * 8, True), fn]) == (
            [want_old, oracle_key(REF, E, F, E.members[2]), bytes(96)], [0, 0, G.BAD_ENCODING])
        assert set_call(G, L, 3, [new]) == (G.SUCCESS, [0]) and L.gbls_committees_members(3) == 40
        assert L.gbls_committees_size() == TABLE_SIZE
        assert bits_keys(G, L, [3, 2, 3], [fo, encode([1] * 8, True), fn]) == (
            [bytes(96), oracle_key(REF, E, F, E.members[2]), want_new], [G.BAD_ENCODING, 0, 0])
    finally:
        assert set_call(G, L, 3, [old]) == (G.SUCCESS, [0])
    assert bits_keys(G, L, [3], [fo]) == ([want_old], [0]) and L.gbls_committees_members(3) == 9


# ---------------------------------------------------------------- 9. replicas, concurrency, the forms
def child(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_bits_child.py")] + list(args),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_replicas_and_concurrent_rewrites_subprocess():
    """Two engines on the one GPU: a 4200-set one-segment batch takes the sharded-partials path of
    verify_host (each engine resolving its shard's slice of the bits against its own member
    blocks), and four threads verify sets of slots that a fifth keeps rewriting with
    gbls_committees_set_members (the same committee in two member orders, under bits whose key is
    the same in both: any verdict other than the expected one is a torn or freed member list)."""
    res = child("replicas")
    assert res["engines"] == 2 and res["table"] == 24
    assert res["big"] == [0, 5] and res["big_err"] == [0, 0]
    assert res["threads"] == {"wrong": 0, "errors": 0, "verified": 4 * 6, "rewrites": res["threads"]["rewrites"]}
    assert res["threads"]["rewrites"] >= 1


def test_launch_forms_give_the_same_bytes_subprocess():
    """GBLS_COMMITTEE_ROW_MIN (read under GBLS_INIT_TUNING in a fresh engine): every set on rows,
    and every set on single lanes, give the keys of the indexed sum, byte for byte."""
    rows = child("switch", "GBLS_COMMITTEE_ROW_MIN=1")
    lanes = child("switch", "GBLS_COMMITTEE_ROW_MIN=1000000")
    for res in (rows, lanes):
        assert res["sets"] == 288 + 32 and res["equal"] == res["sets"] and res["longest"] == 1024
    assert rows["digest"] == lanes["digest"]


# ---------------------------------------------------------------- invalidation (reloads the table)
def test_clear_and_registry_rewrite_drop_the_members(G, L, F, REF, E):
    slots, fields, want = valid_sets(E, REF, F)
    n = len(slots)
    st1 = G.i32_array(1)
    try:
        assert bits_keys(G, L, slots, fields) == (want, [0] * n)
        assert L.gbls_committees_clear() == 0
        assert [L.gbls_committees_members(s) for s in slots] == [0] * n
        assert bits_keys(G, L, slots, fields) == ([bytes(96)] * n, [G.BAD_ENCODING] * n)
        fresh = load_all(G, L, F)
        assert fresh.members == E.members and bits_keys(G, L, slots, fields) == (want, [0] * n)
        # rewriting a loaded key (the same bytes) drops every cached sum and every member list
        G.check(L.gbls_registry_set(10, G.buf(E.comp[480:528]), 1, st1), "registry_set")
        assert st1[0] == 0 and L.gbls_committees_size() == 0
        assert [L.gbls_committees_members(s) for s in slots] == [0] * n
        assert bits_keys(G, L, slots, fields) == ([bytes(96)] * n, [G.BAD_ENCODING] * n)
    finally:
        fresh = load_all(G, L, F)
    assert fresh.members == E.members and L.gbls_committees_size() == TABLE_SIZE
    # an append keeps the table and the members
    n0 = L.gbls_registry_size()
    G.check(L.gbls_registry_set(n0, G.buf(E.comp[:48]), 1, st1), "registry_set")
    assert L.gbls_committees_size() == TABLE_SIZE and bits_keys(G, L, slots, fields) == (want, [0] * n)


# ---------------------------------------------------------------- 10. the Python mirror
def test_python_mirror_takes_the_bits_path(G, L, F, REF, E, block_batch):
    from grandine_amd import bls as B
    from grandine_amd import verifier as V
    b = block_batch
    keys48 = [E.comp[48 * i:48 * i + 48] for i in range(NREG + 1)]
    B.Registry.forget()
    try:
        B.Registry.mirror_finalized(keys48)  # first = 0 rewrites the registry: the table is cleared
        assert B.Committees.size() == 0
        raw = F.public_keys(E.sks)
        pk = [B.PublicKey(raw[96 * v:96 * v + 96]) for v in range(NREG + 1)]
        coms = [E.members.get(s, [0]) for s in range(TABLE_SIZE)]

        def run(sigs, members):
            assert B.Committees.set(0, coms, members=members) == [0] * len(coms)
            mv = V.MultiVerifier()
            comp = compress(G, L, sigs)
            for i in range(b.n):
                msg, sig = b.msgs[32 * i:32 * i + 32], comp[96 * i:96 * i + 96]
                if b.slots[i] is None:
                    mv.verify_aggregate_indexed(msg, sig, b.lists[i], [pk[v] for v in b.lists[i]], None)
                else:
                    mv.verify_aggregate_committee(msg, sig, b.slots[i], E.members[b.slots[i]], b.fields[i],
                                                  [pk[v] for v in b.parts[i]], None)
            try:
                mv.finish(randoms=b.rands)
                return mv.last_path, True
            except V.SignatureInvalid:
                return mv.last_path, False

        assert run(b.sigs, True) == ("bits", ref_mv(REF, b)) == ("bits", True)
        assert run(swapped(b), True) == ("bits", ref_mv(REF, b, sigs=swapped(b))) == ("bits", False)
        # the same triples with the slots loaded without members: the committees path, same verdicts
        assert run(b.sigs, False) == ("committees", True)
        assert run(swapped(b), False) == ("committees", False)
    finally:
        B.Registry.forget()
        load_all(G, L, F)
