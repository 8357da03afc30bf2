"""Cached committee key sums on the GPU (include/grandine_bls_gpu_committees.h): the committee
table, keys formed as committee sum minus absentees, batch verification over such keys, their
equivalence with the participant-list path, invalidation by registry rewrites, replicas and
concurrent rewrites, and the Python mirror.

The secret keys are known, so the oracle's key of a set is ref_sk_to_pk(sum of the participants'
secret keys mod r) and every comparison is byte for byte or verdict for verdict.

Launch forms crossed here: launch_g1_aggregate_idx sums up to 127 committees one workgroup each and
128 or more (kRowAggregateMinSegs) one 16-lane row each; k_g1_committee_keys runs one lane per set
while the longest list of the launch is shorter than kCommitteeRowMin keys and one 16-lane row per
set from that length on (ROW_MIN below; the lane form has 64 sets per block, the row form 4)."""
import contextlib
import ctypes
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NREG = 600          # ordinary registry keys; index NREG holds -key[5] (the doubling case)
NEG5 = NREG
SIZES = [1, 2, 15, 16, 17, 64, 257]
ROW_MIN = 12        # kCommitteeRowMin (grandine_amd/csrc/gbls_common.h)
FIRST_B, N_B = 10, 130   # the second load: 130 committees at slots 10..139 (slots 7..9 never written)
EMPTY_B, BAD_B = 10 + 23, 10 + 57
DBL_SLOT = 140      # committee {5}
TABLE_SIZE = 141


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
    return [(37 * c + 11 * j) % NREG for j in range(size)]  # 11 is coprime to 600: distinct members


def committees_set(G, L, first, coms):
    idx, off = flat(coms)
    st = G.i32_array(len(coms))
    rc = L.gbls_committees_set(first, G.u32_array(idx or [0]), G.u32_array(off), len(coms), st)
    return rc, [st[c] for c in range(len(coms))]


class Env:
    pass


def load_all(G, L, F):
    """Registry (first = 0) and the committee table; returns the statuses of each load."""
    from grandine_amd import bls as B
    B.Registry.forget()
    E = Env()
    E.sks, comp = F.registry(NREG, seed=b"committees")
    E.sks = E.sks + [F.R_ORDER - E.sks[5]]
    comp += F.compress_g1(F.public_keys(E.sks[NREG:]))
    assert not F.load_registry(comp).any()
    assert L.gbls_registry_size() >= NREG + 1  # a registry never shrinks: other tests may have loaded more
    E.comp = comp
    E.members = {}
    # 7 committees at slots 0..6: the workgroup form of launch_g1_aggregate_idx
    a = [members_of(c, SIZES[c]) for c in range(7)]
    E.rc_a, E.st_a = committees_set(G, L, 0, a)
    E.size_a = L.gbls_committees_size()
    # 130 committees at slots 10..139: the row form; one empty, one naming index 10^9
    b = [members_of(100 + c, SIZES[c % 7]) for c in range(N_B)]
    b[EMPTY_B - FIRST_B] = []
    b[BAD_B - FIRST_B] = b[BAD_B - FIRST_B][:3] + [10 ** 9] + b[BAD_B - FIRST_B][3:]
    E.rc_b, E.st_b = committees_set(G, L, FIRST_B, b)
    E.size_b = L.gbls_committees_size()
    E.rc_d, E.st_d = committees_set(G, L, DBL_SLOT, [[5]])
    for c, m in enumerate(a):
        E.members[c] = m
    for c, m in enumerate(b):
        if FIRST_B + c not in (EMPTY_B, BAD_B):
            E.members[FIRST_B + c] = m
    E.members[DBL_SLOT] = [5]
    return E


@pytest.fixture(scope="module")
def E(G, L, F):
    from grandine_amd import bls as B
    env = load_all(G, L, F)
    yield env
    L.gbls_committees_clear()
    B.Registry.forget()


def oracle_key(REF, E, F, participants):
    if not participants:
        return bytes(96)
    s = sum(E.sks[i] for i in participants) % F.R_ORDER
    if s == 0:
        return bytes(96)
    out = ctypes.create_string_buffer(96)
    REF.ref_sk_to_pk(s.to_bytes(32, "big"), out)
    return out.raw


def committee_keys(G, L, slots, lists):
    n = len(slots)
    idx, off = flat(lists)
    out = ctypes.create_string_buffer(96 * n)
    st = G.i32_array(n)
    rc = L.gbls_g1_aggregate_committees(G.u32_array([G.NO_COMMITTEE if s is None else s for s in slots]),
                                        G.u32_array(idx or [0]), G.u32_array(off), n, out, st)
    assert rc == G.SUCCESS, (rc, L.gbls_last_error())
    return [out.raw[96 * i:96 * i + 96] for i in range(n)], [st[i] for i in range(n)]


def indexed_keys(G, L, lists):
    n = len(lists)
    idx, off = flat(lists)
    out = ctypes.create_string_buffer(96 * n)
    st = G.i32_array(n)
    G.check(L.gbls_g1_aggregate_indexed(G.u32_array(idx or [0]), G.u32_array(off), n, out, st), "aggregate_indexed")
    return [out.raw[96 * i:96 * i + 96] for i in range(n)], [st[i] for i in range(n)]


# ---------------------------------------------------------------- 4. the table
def test_table_statuses_and_slots(G, L, F, REF, E):
    assert (E.rc_a, E.st_a, E.size_a) == (G.SUCCESS, [G.SUCCESS] * 7, 7)
    want_b = [G.SUCCESS] * N_B
    want_b[EMPTY_B - FIRST_B] = G.AGGR_TYPE_MISMATCH
    want_b[BAD_B - FIRST_B] = G.BAD_ENCODING
    assert (E.rc_b, E.st_b, E.size_b) == (G.SUCCESS, want_b, FIRST_B + N_B)
    assert (E.rc_d, E.st_d) == (G.SUCCESS, [G.SUCCESS]) and L.gbls_committees_size() == TABLE_SIZE
    # a slot with an empty absentee list reads back as the cached sum
    slots = list(range(TABLE_SIZE + 2))
    keys, st = committee_keys(G, L, slots, [[] for _ in slots])
    for s in slots:
        if s in E.members:
            assert (st[s], keys[s]) == (G.SUCCESS, oracle_key(REF, E, F, E.members[s])), s
        else:  # 7..9 never written, the empty one, the one with a bad index, two past the size
            assert s in (7, 8, 9, EMPTY_B, BAD_B, TABLE_SIZE, TABLE_SIZE + 1)
            assert (st[s], keys[s]) == (G.BAD_ENCODING, bytes(96)), s


def test_table_rewrite_and_arguments(G, L, F, REF, E):
    old = E.members[3]
    new = members_of(991, 40)
    try:
        assert committees_set(G, L, 3, [new]) == (G.SUCCESS, [G.SUCCESS])
        assert L.gbls_committees_size() == TABLE_SIZE
        keys, st = committee_keys(G, L, [3, 2, 4], [[], [], []])
        assert st == [0, 0, 0]
        assert keys == [oracle_key(REF, E, F, m) for m in (new, E.members[2], E.members[4])]
    finally:
        assert committees_set(G, L, 3, [old]) == (G.SUCCESS, [G.SUCCESS])
    assert committee_keys(G, L, [3], [[]])[0] == [oracle_key(REF, E, F, old)]
    # offsets that do not start at 0 or decrease, and a table past 2^20 slots: GBLS_ERR_ARG
    st = G.i32_array(2)
    for off in ([1, 2, 3], [0, 2, 1]):
        assert L.gbls_committees_set(0, G.u32_array([1, 2, 3]), G.u32_array(off), 2, st) == G.VERIFY_FAIL
        assert L.gbls_last_error() == 102
    assert L.gbls_committees_set((1 << 20) - 1, G.u32_array([1, 2]), G.u32_array([0, 1, 2]), 2, st) == G.VERIFY_FAIL
    assert L.gbls_last_error() == 102 and L.gbls_committees_size() == TABLE_SIZE


# ---------------------------------------------------------------- 5. keys
ABSENT = [0, 1, 2, 15, 16, 17, "all-but-one", "all"]


def key_sets(E, n, long_lists):
    """n sets over the loaded committees, committee sizes cycling through SIZES and absentee counts
    through ABSENT; every fourth set names no committee and lists its participants instead.
    long_lists: lists of up to 256 keys (the row form); else every list is shorter than ROW_MIN
    (the lane form), so large committees lose at most ROW_MIN - 1 members."""
    by_size = {z: [s for s in sorted(E.members) if len(E.members[s]) == z] for z in SIZES}
    slots, lists, parts = [], [], []
    for i in range(n):
        cand = by_size[SIZES[i % 7]]
        s = cand[(i // 7) % len(cand)]
        m = E.members[s]
        want = ABSENT[i % len(ABSENT)]
        k = len(m) if want == "all" else len(m) - 1 if want == "all-but-one" else min(want, len(m))
        if not long_lists:
            k = min(k, ROW_MIN - 1)
        absent = [m[(i + j) % len(m)] for j in range(k)]
        part = [v for v in m if v not in absent]
        if i % 4 == 3 and part and (long_lists or len(part) < ROW_MIN):
            slots.append(None)
            lists.append(part)
        else:
            slots.append(s)
            lists.append(absent)
        parts.append(part)
    return slots, lists, parts


@pytest.mark.parametrize("n,long_lists", [(9, False), (300, True), (300, False), (9, True)])
def test_keys_equal_oracle_and_indexed_sum(G, L, F, REF, E, n, long_lists):
    slots, lists, parts = key_sets(E, n, long_lists)
    longest = max(len(v) for v in lists)
    assert (longest >= ROW_MIN) == long_lists  # the form this launch takes
    assert any(s is None for s in slots) and any(not p for p in parts) and any(not v for v in lists)
    keys, st = committee_keys(G, L, slots, lists)
    ref_keys, ref_st = indexed_keys(G, L, parts)
    for i in range(n):
        assert st[i] == G.SUCCESS, i
        assert keys[i] == oracle_key(REF, E, F, parts[i]), (i, slots[i], len(lists[i]))
        assert keys[i] == ref_keys[i], i
        if not parts[i]:  # every member absent: infinity, all-zero bytes
            assert keys[i] == bytes(96) and ref_st[i] == G.AGGR_TYPE_MISMATCH
        else:
            assert ref_st[i] == G.SUCCESS


def test_keys_degenerate_and_rejected(G, L, F, REF, E):
    two_p = oracle_key(REF, E, F, [5, 5])
    m = E.members[5]
    slots = [DBL_SLOT, DBL_SLOT, None, None, 5, TABLE_SIZE + 3, 8, 5]
    lists = [[NEG5], [5], [], [5, NEG5], [m[0], 10 ** 9], [], [m[0]], m + [m[0], m[0]]]
    keys, st = committee_keys(G, L, slots, lists)
    assert (st[0], keys[0]) == (G.SUCCESS, two_p)            # {P} minus -P: a doubling
    assert (st[1], keys[1]) == (G.SUCCESS, bytes(96))        # {P} minus P: the identity
    assert (st[2], keys[2]) == (G.AGGR_TYPE_MISMATCH, bytes(96))  # no committee, empty list
    assert (st[3], keys[3]) == (G.SUCCESS, bytes(96))        # no committee, a sum that cancels
    assert (st[4], keys[4]) == (G.BAD_ENCODING, bytes(96))   # an index past the registry
    assert (st[5], keys[5]) == (G.BAD_ENCODING, bytes(96))   # a slot past the table
    assert (st[6], keys[6]) == (G.BAD_ENCODING, bytes(96))   # a slot never written
    # non-members are not checked: the key is what the formula gives (here -2 m[0])
    want = oracle_key(REF, E, F, [m[0], m[0]])
    neg = want[:48] + ((O_P() - int.from_bytes(want[48:], "little")) % O_P()).to_bytes(48, "little")
    assert (st[7], keys[7]) == (G.SUCCESS, neg)


def O_P():
    from oracle import bls12_381 as O
    return O.P


# ---------------------------------------------------------------- 6. / 7. verdicts
N = 48


class Batch:
    pass


def make_batch(G, L, F, REF, E, tag, msg_repeat=1):
    """40 committee sets and 8 sets without a committee (every sixth), fixed nonzero scalars."""
    b = Batch()
    valid = [s for s in sorted(E.members) if len(E.members[s]) >= 15 and s != 3]
    b.slots, b.lists, b.parts, b.coms = [], [], [], []
    for i in range(N):
        s = valid[(7 * i) % len(valid)]
        m = E.members[s]
        absent = m[i % 5:i % 5 + (i % 4)]  # 0..3 absentees
        part = [v for v in m if v not in absent]
        b.slots.append(None if i % 6 == 5 else s)
        b.lists.append(part if i % 6 == 5 else absent)
        b.parts.append(part)
        b.coms.append(s)
    um = F.messages(N // msg_repeat, b"committees/" + tag)
    b.msgs = b"".join(um[32 * (i % (N // msg_repeat)):32 * (i % (N // msg_repeat)) + 32] for i in range(N))
    sums = [sum(E.sks[v] for v in p) % F.R_ORDER for p in b.parts]
    b.sigs = F.sign(sums, b.msgs)
    b.pks = b"".join(oracle_key(REF, E, F, p) for p in b.parts)
    b.rands = F.rands(N, 4242)
    return b


def compress(G, L, sigs):
    n = len(sigs) // 192
    out = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, out), "compress")
    return out.raw


def mv_committees(G, L, b, sigs=None, slots=None, lists=None, flags=0, comp=None):
    slots = b.slots if slots is None else slots
    idx, off = flat(b.lists if lists is None else lists)
    st = G.i32_array(N)
    comp = compress(G, L, b.sigs if sigs is None else sigs) if comp is None else comp
    rc = L.gbls_multi_verify_committees(b.msgs, comp, G.u32_array([G.NO_COMMITTEE if s is None else s for s in slots]),
                                        G.u32_array(idx or [0]), G.u32_array(off), u64(b.rands), N, st, flags)
    return rc, [st[i] for i in range(N)], L.gbls_last_error()


def mv_indexed(G, L, b, sigs=None, comp=None):
    idx, off = flat(b.parts)
    st = G.i32_array(N)
    comp = compress(G, L, b.sigs if sigs is None else sigs) if comp is None else comp
    rc = L.gbls_multi_verify_compressed_ex(b.msgs, comp, None, G.u32_array(idx), G.u32_array(off), u64(b.rands), N, st, 0)
    return rc, [st[i] for i in range(N)], L.gbls_last_error()


def ref_mv(REF, b, sigs=None, pks=None):
    return bool(REF.ref_multi_verify(b.msgs, b.sigs if sigs is None else sigs, b.pks if pks is None else pks,
                                     u64(b.rands), N, 16))


def swapped(b, i=4, j=29):
    s = bytearray(b.sigs)
    s[192 * i:192 * i + 192], s[192 * j:192 * j + 192] = b.sigs[192 * j:192 * j + 192], b.sigs[192 * i:192 * i + 192]
    return bytes(s)


@pytest.fixture(scope="module")
def batch(G, L, F, REF, E):
    return make_batch(G, L, F, REF, E, b"plain")


@pytest.mark.parametrize("flags", [0, 1])  # 1: GBLS_CALL_BLOCK
def test_verdicts(G, L, F, REF, E, batch, flags):
    b = batch
    ok = [0] * N
    assert sum(s is None for s in b.slots) == 8
    assert ref_mv(REF, b)
    assert mv_committees(G, L, b, flags=flags) == (G.SUCCESS, ok, 0)
    sw = swapped(b)
    assert not ref_mv(REF, b, sigs=sw)
    assert mv_committees(G, L, b, sigs=sw, flags=flags) == (G.VERIFY_FAIL, ok, 0)
    # one absentee omitted: the key includes a non-signer
    k = next(i for i in range(N) if b.slots[i] is not None and len(b.lists[i]) >= 2)
    lists = list(b.lists)
    lists[k] = b.lists[k][1:]
    pks = b.pks[:96 * k] + oracle_key(REF, E, F, b.parts[k] + b.lists[k][:1]) + b.pks[96 * (k + 1):]
    assert not ref_mv(REF, b, pks=pks)
    assert mv_committees(G, L, b, lists=lists, flags=flags) == (G.VERIFY_FAIL, ok, 0)
    # a slot past the table, an invalid slot, every member absent: the batch fails, no engine error
    for slot, lst in ((TABLE_SIZE + 3, b.lists[k]), (8, b.lists[k]), (b.slots[k], E.members[b.slots[k]])):
        slots, lists = list(b.slots), list(b.lists)
        slots[k], lists[k] = slot, lst
        assert mv_committees(G, L, b, slots=slots, lists=lists, flags=flags) == (G.VERIFY_FAIL, ok, 0), slot
    # a signature that does not decode is returned first, with the statuses of the existing path
    comp = bytearray(compress(G, L, sw))
    comp[96 * 17] &= 0x7F  # the compression flag
    rc, st, err = mv_committees(G, L, b, comp=bytes(comp), flags=flags)
    assert (rc, st, err) == mv_indexed(G, L, b, comp=bytes(comp))
    assert rc == st[17] != G.SUCCESS and [x for i, x in enumerate(st) if i != 17] == [0] * (N - 1)


def test_argument_errors_fail_closed(G, L, batch):
    b = batch
    idx, off = flat(b.lists)
    st = G.i32_array(N)
    com = G.u32_array([G.NO_COMMITTEE if s is None else s for s in b.slots])
    comp = compress(G, L, b.sigs)
    assert L.gbls_multi_verify_committees(b.msgs, comp, com, G.u32_array(idx), None, u64(b.rands), N, st, 0) == G.VERIFY_FAIL
    assert L.gbls_last_error() == 102 and [st[i] for i in range(N)] == [G.BAD_ENCODING] * N  # pk_off is required
    assert L.gbls_multi_verify_committees(b.msgs, comp, com, G.u32_array(idx), G.u32_array(off), u64(b.rands), 0, st,
                                          0) == G.VERIFY_FAIL
    assert L.gbls_last_error() == 0  # n == 0: a verdict


@contextlib.contextmanager
def dedup_policy(L, G):
    prev = L.gbls_set_policy(0)
    L.gbls_set_policy(prev | G.INIT_DEDUP)
    try:
        yield
    finally:
        L.gbls_set_policy(prev)


def test_equivalence_with_the_participant_path(G, L, F, REF, E, batch):
    for b in (batch, make_batch(G, L, F, REF, E, b"repeat", msg_repeat=4)):
        dedup = b is not batch
        assert len(set(b.msgs[32 * i:32 * i + 32] for i in range(N))) == (12 if dedup else N)
        with (dedup_policy(L, G) if dedup else contextlib.nullcontext()):
            clean, bad = mv_committees(G, L, b), mv_committees(G, L, b, sigs=swapped(b))
            assert clean == mv_indexed(G, L, b) and bad == mv_indexed(G, L, b, sigs=swapped(b))
        assert (clean[0], bad[0]) == (G.SUCCESS, G.VERIFY_FAIL)
        assert (ref_mv(REF, b), ref_mv(REF, b, sigs=swapped(b))) == (True, False)


# ---------------------------------------------------------------- 8. invalidation
def test_registry_rewrite_clears_and_append_keeps(G, L, F, REF, E, batch):
    st = G.i32_array(1)
    try:
        # rewriting a loaded key (the same bytes) drops every cached sum
        G.check(L.gbls_registry_set(10, G.buf(E.comp[480:528]), 1, st), "registry_set")
        assert st[0] == 0 and L.gbls_committees_size() == 0
        assert mv_committees(G, L, batch) == (G.VERIFY_FAIL, [0] * N, 0)
        keys, kst = committee_keys(G, L, [0], [[]])
        assert (kst, keys) == ([G.BAD_ENCODING], [bytes(96)])
    finally:
        fresh = load_all(G, L, F)
    assert fresh.members == E.members and L.gbls_committees_size() == TABLE_SIZE
    assert mv_committees(G, L, batch) == (G.SUCCESS, [0] * N, 0)
    # an append keeps the table and the verdicts
    n0 = L.gbls_registry_size()
    G.check(L.gbls_registry_set(n0, G.buf(E.comp[:48]), 1, st), "registry_set")
    assert L.gbls_registry_size() == n0 + 1 and L.gbls_committees_size() == TABLE_SIZE
    assert mv_committees(G, L, batch) == (G.SUCCESS, [0] * N, 0)
    assert mv_committees(G, L, batch, sigs=swapped(batch)) == (G.VERIFY_FAIL, [0] * N, 0)
    assert committee_keys(G, L, [2], [[]])[0] == [oracle_key(REF, E, F, E.members[2])]


# ---------------------------------------------------------------- 9. replicas, concurrency, the switch
def child(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_committees_child.py")] + list(args),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_replicas_and_concurrent_rewrites_subprocess():
    """Two engines on the one GPU: a 4200-set one-segment batch takes the sharded-partials path of
    verify_host (each engine resolving its shard's keys from its own table replica), and four
    threads verify while a fifth rewrites another slot range."""
    res = child("replicas")
    assert res["engines"] == 2 and res["table"] == 16
    assert res["big"] == [0, 5] and res["big_err"] == [0, 0]
    assert res["threads"] == {"wrong": 0, "errors": 0, "verified": 4 * 6, "rewrites": res["threads"]["rewrites"]}
    assert res["threads"]["rewrites"] >= 1


@pytest.mark.parametrize("row_min", [1, 1000000])
def test_list_length_switch_subprocess(row_min):
    """GBLS_COMMITTEE_ROW_MIN (read under GBLS_INIT_TUNING in a fresh engine): every list on rows,
    and every list on single lanes, give the keys of the indexed sum."""
    res = child("switch", "GBLS_COMMITTEE_ROW_MIN=%d" % row_min)
    assert res["sets"] == 150 and res["equal"] == 150 and res["longest"] == 257


# ---------------------------------------------------------------- 10. the Python mirror
def test_python_mirror_takes_the_committees_path(G, L, F, REF, E, batch):
    from grandine_amd import bls as B
    from grandine_amd import verifier as V
    b = batch
    keys48 = [E.comp[48 * i:48 * i + 48] for i in range(NREG + 1)]
    B.Registry.forget()
    try:
        B.Registry.mirror_finalized(keys48)  # first = 0 rewrites the registry: the table is cleared
        assert B.Committees.size() == 0
        slots = sorted(set(b.coms))
        lo = min(slots)
        coms = [E.members.get(s, [0]) for s in range(lo, max(slots) + 1)]
        assert B.Committees.set(lo, coms) == [0] * len(coms) and B.Committees.size() == max(slots) + 1
        raw = F.public_keys(E.sks)
        pk = [B.PublicKey(raw[96 * v:96 * v + 96]) for v in range(NREG + 1)]

        def run(sigs, forget_slot=None):
            mv = V.MultiVerifier()
            comp = compress(G, L, sigs)
            for i in range(N):
                com = E.members[b.coms[i]]
                mv.verify_aggregate_committee(b.msgs[32 * i:32 * i + 32], comp[96 * i:96 * i + 96], b.coms[i], com,
                                              [v in b.parts[i] for v in com], [pk[v] for v in b.parts[i]], None)
            saved = dict(B.Committees._members)
            if forget_slot is not None:
                B.Committees._members.pop(forget_slot)
            try:
                mv.finish(randoms=b.rands)
                return mv.last_path, True
            except V.SignatureInvalid:
                return mv.last_path, False
            finally:
                B.Committees._members = saved

        assert run(b.sigs) == ("committees", ref_mv(REF, b)) == ("committees", True)
        assert run(swapped(b)) == ("committees", ref_mv(REF, b, sigs=swapped(b))) == ("committees", False)
        # one slot not loaded in the mirror: the registry-index path, same verdicts
        assert run(b.sigs, forget_slot=slots[0]) == ("indices", True)
        assert run(swapped(b), forget_slot=slots[0]) == ("indices", False)
    finally:
        B.Registry.forget()
        load_all(G, L, F)
