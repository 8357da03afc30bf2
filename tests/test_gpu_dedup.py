"""Message-grouped batch verification (GBLS_INIT_DEDUP) on the GPU: one hash_to_G2 and one Miller
pair per distinct message of a segment, e(sum_i r_i pk_i, H(m)), with every verdict, per-set
rejection and signature status unchanged.  Expected verdicts come from the C oracle
(ref_multi_verify / ref_verify) on the same sets and scalars; a run with the policy off is
asserted equal in addition.  Every case restores the previous policy."""
import contextlib
import ctypes
import os
import re
import subprocess
import sys
import threading

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    """The same oracle built with its faster tower (tests/test_ref_oracle.py checks the two equal),
    for the shapes of thousands of sets."""
    return _oracle("libbls_ref_fast.so")


def u64(vals):
    return (ctypes.c_uint64 * max(len(vals), 1))(*vals)


def ref_mv(C, b, lo=0, hi=None):
    hi = b["n"] if hi is None else hi
    n = hi - lo
    return bool(C.ref_multi_verify(b["msgs"][32 * lo:32 * hi], b["sigs"][192 * lo:192 * hi], b["pks"][96 * lo:96 * hi],
                                   u64(b["rands"][lo:hi]), n, 16))


@contextlib.contextmanager
def policy(L, G, on=True):
    """The DEDUP policy bit set (or cleared) with the other policy bits kept, restored on exit."""
    prev = L.gbls_set_policy(0)
    L.gbls_set_policy((prev | G.INIT_DEDUP) if on else (prev & ~G.INIT_DEDUP))
    try:
        yield
    finally:
        L.gbls_set_policy(prev)


def stage_index(L, name):
    return [L.gbls_stage_name(k).decode() for k in range(32) if L.gbls_stage_name(k)].index(name)


@contextlib.contextmanager
def msgsum_calls(L):
    """Counts the k_g1s_msgsum launches of the calls inside (out[0] on exit)."""
    out = [0]
    calls = (ctypes.c_uint32 * 32)()
    k = stage_index(L, "k_g1s_msgsum")
    L.gbls_profile(1)
    try:
        L.gbls_profile_read(None, calls, 32)
        before = calls[k]
        yield out
        L.gbls_profile_read(None, calls, 32)
        out[0] = calls[k] - before
    finally:
        L.gbls_profile(0)


def batch(F, sizes, seed, interleave=True):
    """Single-key sets signing len(sizes) distinct messages, sizes[g] sets on message g; the
    groups' members interleaved (set i of the round-robin order) unless interleave is off."""
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


def corrupt(b, i, j):
    """Set i carries set j's signature."""
    c = dict(b)
    s = bytearray(b["sigs"])
    s[192 * i:192 * i + 192] = b["sigs"][192 * j:192 * j + 192]
    c["sigs"] = bytes(s)
    return c


def mv(L, b):
    return L.gbls_multi_verify(b["msgs"], b["sigs"], b["pks"], u64(b["rands"]), b["n"]) == 0


def check_both_policies(L, G, C, b, expect=None):
    """Oracle verdict == grouped verdict (== plain verdict), and the grouped run used the kernel."""
    want = ref_mv(C, b)
    if expect is not None:
        assert want == expect
    with policy(L, G), msgsum_calls(L) as used:
        assert mv(L, b) == want
    assert used[0] >= 1
    with policy(L, G, on=False), msgsum_calls(L) as used:
        assert mv(L, b) == want
    assert used[0] == 0


# ---------------------------------------------------------------- 1. policy plumbing
def test_policy_bit_is_set_returned_and_sticky(G, L):
    assert G.INIT_DEDUP == 0x800
    prev = L.gbls_set_policy(G.INIT_DEDUP)
    try:
        assert L.gbls_set_policy(0) == G.INIT_DEDUP
        assert L.gbls_set_policy(G.INIT_DEDUP) == 0
        assert L.gbls_init(0, 0) == G.SUCCESS  # a lazy init does not clear it
        assert L.gbls_set_policy(G.INIT_DEDUP | G.INIT_PER_CHECK) == G.INIT_DEDUP
        assert L.gbls_set_policy(0) == G.INIT_DEDUP | G.INIT_PER_CHECK
        assert L.gbls_init(0, G.INIT_DEDUP) == G.SUCCESS  # gbls_init accepts it and turns it on
        assert L.gbls_set_policy(0) == G.INIT_DEDUP
        assert L.gbls_set_policy(0) == 0
    finally:
        L.gbls_set_policy(prev)
    from grandine_amd import bls as B
    prev = B.set_policy(B.POLICY_DEDUP)
    try:
        assert B.set_policy(prev) == B.POLICY_DEDUP
    finally:
        L.gbls_set_policy(prev)


# ---------------------------------------------------------------- 2. small shapes
SMALL = {"n2_same": [2], "n3_2+1": [2, 1], "n64_one": [64], "n65_one": [65], "n130_1_2_63_64": [1, 2, 63, 64]}


@pytest.mark.parametrize("name", list(SMALL))
def test_small_shapes(G, L, F, REF, name):
    sizes = SMALL[name]
    b = batch(F, sizes, b"dedup/" + name.encode())
    check_both_policies(L, G, REF, b, expect=True)
    big = max(range(len(sizes)), key=lambda g: sizes[g])
    members = [i for i, g in enumerate(b["of"]) if g == big]
    # a corrupted signature inside a duplicate group (another member's signature)
    check_both_policies(L, G, REF, corrupt(b, members[-1], members[0]), expect=False)
    singles = [g for g, s in enumerate(sizes) if s == 1]
    if singles:  # a corrupted signature in a singleton group beside duplicates
        i = b["of"].index(singles[0])
        check_both_policies(L, G, REF, corrupt(b, i, members[0]), expect=False)


# ---------------------------------------------------------------- 3. algebraic edges
def test_swapped_signatures_in_one_group(G, L, F, REF):
    b = batch(F, [2], b"dedup/swap")
    sw = dict(b, sigs=b["sigs"][192:384] + b["sigs"][:192])
    assert sw["rands"][0] != sw["rands"][1]
    check_both_policies(L, G, REF, sw, expect=False)
    eq = dict(sw, rands=[sw["rands"][0]] * 2)  # equal scalars: the sums coincide, the oracle passes
    check_both_policies(L, G, REF, eq, expect=True)


def test_opposite_keys_and_signatures(G, L, F, REF):
    """(pk, sig) and (-pk, -sig) on one message under equal scalars: the group's sum and S are both
    infinity; the group contributes e(O, H) = 1."""
    from oracle import bls12_381 as O
    b = batch(F, [1], b"dedup/neg")
    P = O.P

    def neg_fp(raw):
        v = int.from_bytes(raw, "little")
        return ((P - v) % P).to_bytes(48, "little")

    npk = b["pks"][:48] + neg_fp(b["pks"][48:96])
    nsig = b["sigs"][:96] + neg_fp(b["sigs"][96:144]) + neg_fp(b["sigs"][144:192])
    r = b["rands"][0]
    two = dict(n=2, msgs=b["msgs"] * 2, pks=b["pks"] + npk, sigs=b["sigs"] + nsig, rands=[r, r])
    check_both_policies(L, G, REF, two)
    # with a third, honest set in the same group the sum is that set's point
    c = batch(F, [3], b"dedup/neg3")
    three = dict(n=3, msgs=c["msgs"][:32] * 3, pks=c["pks"][:96] + b["pks"] + npk, rands=[c["rands"][0], r, r],
                 sigs=F.sign(c["sks"][:1], c["msgs"][:32]) + F.sign(b["sks"], c["msgs"][:32]))
    s2 = three["sigs"][192:384]
    three["sigs"] += s2[:96] + neg_fp(s2[96:144]) + neg_fp(s2[144:192])
    check_both_policies(L, G, REF, three, expect=True)


def test_same_set_twice_under_equal_scalars(G, L, F, REF):
    b = batch(F, [1], b"dedup/dbl")
    two = dict(n=2, msgs=b["msgs"] * 2, pks=b["pks"] * 2, sigs=b["sigs"] * 2, rands=b["rands"] * 2)
    check_both_policies(L, G, REF, two, expect=True)  # the doubling case of the group sum


def test_rejections_inside_a_group(G, L, F, REF):
    b = batch(F, [4, 2], b"dedup/rej")
    i = [k for k, g in enumerate(b["of"]) if g == 0][2]
    inf_pk = dict(b, pks=b["pks"][:96 * i] + bytes(96) + b["pks"][96 * (i + 1):])
    check_both_policies(L, G, REF, inf_pk, expect=False)  # an infinite key must fail
    inf_sig = dict(b, sigs=b["sigs"][:192 * i] + bytes(192) + b["sigs"][192 * (i + 1):])
    check_both_policies(L, G, REF, inf_sig)  # an infinite signature: as the oracle
    zero = dict(b, rands=b["rands"][:i] + [0] + b["rands"][i + 1:])
    with policy(L, G):
        assert not mv(L, zero)  # a zero scalar fails closed (the reference only draws nonzero ones)
    with policy(L, G, on=False):
        assert not mv(L, zero)


# ---------------------------------------------------------------- 4. segments
def test_segments_share_a_message(G, L, F, REF):
    b = batch(F, [9, 3], b"dedup/seg", interleave=False)  # message 0: sets 0..8, message 1: 9..11
    seg = [0, 0, 5, 5, 12]  # an empty segment, sets 0..4, another empty one, sets 5..11
    bad = corrupt(b, 6, 7)  # inside segment 3's group of message 0
    want = [ref_mv(REF, bad, 0, 5), ref_mv(REF, bad, 5, 12)]
    assert want == [True, False]
    for on in (True, False):
        v = G.i32_array(4)
        with policy(L, G, on=on), msgsum_calls(L) as used:
            rc = L.gbls_multi_verify_segments(bad["msgs"], bad["sigs"], bad["pks"], u64(bad["rands"]), 12,
                                              G.u32_array(seg), 4, v)
        assert rc == G.SUCCESS and (used[0] >= 1) == on
        # an empty segment: VERIFY_FAIL, as gbls_multi_verify of no sets
        assert [x == 0 for x in v] == [False, want[0], False, want[1]]


# ---------------------------------------------------------------- 5. key sources, fused decompression
def test_key_lists_and_compressed_signatures(G, L, F, REF):
    sizes = [1, 3, 64, 3, 1, 64]  # key-list sizes of the six sets
    um = F.messages(2, b"dedup/kl")
    of = [0, 1, 0, 0, 1, 0]
    n, nkeys = len(sizes), sum(sizes)
    sks = F.seeded_sks(nkeys, b"dedup/kl")
    keys = F.public_keys(sks)
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    sums = [sum(sks[off[i]:off[i + 1]]) % F.R_ORDER for i in range(n)]
    msgs = b"".join(um[32 * g:32 * g + 32] for g in of)
    sigs = F.sign(sums, msgs)
    comp = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(sigs, n, comp), "compress")
    agg = b""
    for s in sums:
        out = ctypes.create_string_buffer(96)
        REF.ref_sk_to_pk(s.to_bytes(32, "big"), out)
        agg += out.raw
    rands = F.rands(n, 77)
    b = dict(n=n, msgs=msgs, sigs=sigs, pks=agg, rands=rands)
    assert ref_mv(REF, b)
    bad_sig = corrupt(b, 3, 2)
    assert not ref_mv(REF, bad_sig)
    bad_comp = ctypes.create_string_buffer(96 * n)
    G.check(L.gbls_g2_compress(bad_sig["sigs"], n, bad_comp), "compress")
    undecodable = bytearray(comp.raw)
    undecodable[96 * 2] &= 0x7F  # the compression flag of a signature inside message 0's group
    for on in (True, False):
        st = G.i32_array(n)
        with policy(L, G, on=on), msgsum_calls(L) as used:
            ok = L.gbls_multi_verify_compressed_ex(msgs, comp.raw, G.buf(keys), None, G.u32_array(off), u64(rands), n,
                                                   st, 0)
            bad = L.gbls_multi_verify_compressed_ex(msgs, bad_comp.raw, G.buf(keys), None, G.u32_array(off),
                                                    u64(rands), n, st, 0)
            dec = L.gbls_multi_verify_compressed(msgs, bytes(undecodable), G.buf(keys), None, G.u32_array(off),
                                                 u64(rands), n, st)
        assert (ok, bad) == (G.SUCCESS, G.VERIFY_FAIL)
        assert dec == st[2] != G.SUCCESS and [st[i] for i in range(n) if i != 2] == [0] * (n - 1)
        assert (used[0] >= 3) == on


def test_indexed_over_a_registry(G, L, F, REF):
    reg_sks, reg = F.registry(64, b"dedup/reg")
    assert not F.load_registry(reg).any()
    idx = [(7 * i + 3) % 64 for i in range(12)]
    um = F.messages(3, b"dedup/idx")
    of = [i % 3 for i in range(12)]
    msgs = b"".join(um[32 * g:32 * g + 32] for g in of)
    sks = [reg_sks[k] for k in idx]
    b = dict(n=12, msgs=msgs, sigs=F.sign(sks, msgs), pks=F.public_keys(sks), rands=F.rands(12, 78))
    bad = corrupt(b, 4, 1)
    assert ref_mv(REF, b) and not ref_mv(REF, bad)
    for on in (True, False):
        with policy(L, G, on=on), msgsum_calls(L) as used:
            assert L.gbls_multi_verify_indexed(msgs, b["sigs"], G.u32_array(idx), None, u64(b["rands"]), 12) == G.SUCCESS
            assert L.gbls_multi_verify_indexed(msgs, bad["sigs"], G.u32_array(idx), None, u64(b["rands"]),
                                               12) == G.VERIFY_FAIL
            out_of_range = list(idx)
            out_of_range[5] = 1 << 31  # a registry index out of range inside a group fails the batch
            assert L.gbls_multi_verify_indexed(msgs, b["sigs"], G.u32_array(out_of_range), None, u64(b["rands"]),
                                               12) == G.VERIFY_FAIL
        assert (used[0] >= 3) == on


# ---------------------------------------------------------------- 6. bisection
def test_bisect_two_invalid_sets_in_one_group(G, L, F, REF):
    b = batch(F, [30, 20, 14], b"dedup/bisect")
    members = [i for i, g in enumerate(b["of"]) if g == 1]
    x, y = members[3], members[11]
    bad = corrupt(corrupt(b, x, members[0]), y, members[1])
    expect = [bool(REF.ref_verify(bad["sigs"][192 * i:192 * i + 192], bad["msgs"][32 * i:32 * i + 32], 32,
                                  bad["pks"][96 * i:96 * i + 96])) for i in range(64)]
    assert [i for i, ok in enumerate(expect) if not ok] == [x, y]
    for on in (True, False):
        v = G.i32_array(64)
        with policy(L, G, on=on), msgsum_calls(L) as used:
            rc = L.gbls_multi_verify_bisect(bad["msgs"], bad["sigs"], bad["pks"], None, None, u64(bad["rands"]), 64, v)
        assert rc == G.SUCCESS and [s == 0 for s in v] == expect
        assert (used[0] >= 1) == on


# ---------------------------------------------------------------- 7. / 8. the MSM and lane regimes
@pytest.fixture(scope="module")
def msm_batch(F):
    return batch(F, [64] * 32, b"dedup/msm")  # one segment of 2048 sets (kMsmMinPerSeg), 32 messages


@pytest.mark.parametrize("bad", [False, True])
def test_msm_regime(G, L, F, REF_FAST, msm_batch, bad):
    b = corrupt(msm_batch, 1000, 1032) if bad else msm_batch  # sets 1000 and 1032 share message 8
    assert b["of"][1000] == b["of"][1032]
    check_both_policies(L, G, REF_FAST, b, expect=not bad)


@pytest.fixture(scope="module")
def lane_batch(F):
    return batch(F, [2] * 2048, b"dedup/lane")  # 4096 sets, 2048 groups > kW4Max: the lane forms


@pytest.mark.parametrize("bad", [False, True])
def test_lane_regime(G, L, F, REF_FAST, lane_batch, bad):
    b = corrupt(lane_batch, 77, 77 + 2048) if bad else lane_batch
    assert b["of"][77] == b["of"][77 + 2048]
    check_both_policies(L, G, REF_FAST, b, expect=not bad)


# ---------------------------------------------------------------- 9. the coalescer
def test_coalesced_callers_keep_their_verdicts(G, L, F, REF):
    batches = []
    for t in range(16):
        b = batch(F, [8], b"dedup/co/%d" % (t % 4))  # four messages shared by the 16 callers
        b["rands"] = F.rands(8, 900 + t)
        if t % 2:
            b = corrupt(b, t % 8, (t + 1) % 8)
        batches.append(b)
    want = [ref_mv(REF, b) for b in batches]
    assert want == [t % 2 == 0 for t in range(16)]
    got = [None] * 16
    gate = threading.Barrier(16)

    def worker(t):
        gate.wait()
        got[t] = mv(L, batches[t])

    with policy(L, G), msgsum_calls(L) as used:
        th = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
        for x in th:
            x.start()
        for x in th:
            x.join()
    assert got == want
    assert used[0] >= 1


# ---------------------------------------------------------------- 10. the plan reaches the GPU
def test_plan_reaches_the_gpu_in_a_fresh_process():
    env = dict(os.environ, GBLS_TRACE_DEDUP="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_dedup_trace.py")], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stderr.splitlines() if ln.startswith("gbls dedup:")]
    assert len(lines) == 1, lines  # the all-distinct batch falls through: no plan, no line
    f = dict(kv.split("=") for kv in lines[0].split()[2:])
    assert (f["sets"], f["segments"], f["groups"], f["pairs"]) == ("64", "1", "3", "4")
    calls = dict(re.findall(r"^(\w+) msgsum_calls=(\d+)$", out.stdout, flags=re.M))
    assert int(calls["grouped"]) > 0 and int(calls["distinct"]) == 0
