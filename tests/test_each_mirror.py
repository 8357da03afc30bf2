"""CPU: the Python mirror of the per-set and per-item calls over span sets, with the engine calls
stubbed: MultiVerifier.verify_each takes the "spans" path exactly when finish would
(_finish_spans: the same qualification, the same arguments) and the "points" path otherwise,
verify_items maps triples to items, split_failed_batch splits by the per-set outcomes, and the
Signature entries marshal the sets as multi_verify_compressed_spans does."""
import pytest

from grandine_amd import _lib as G
from grandine_amd import bls, verifier as V

MSG = bytes(range(32))
SIG = bytes(96)
C0, C1, C3 = list(range(0, 8)), list(range(8, 19)), list(range(30, 35))  # 8, 11 and 5 members
RAW1 = bytes([0b11111101, 0b00001110])  # a Bitlist over C1
SPAN_BITS = [1] * 8 + [1, 0, 1, 1, 1]   # C0 full, C3 without its second member


class Key:  # stands for a bls.PublicKey: the stubbed engine never looks inside
    def __init__(self, i):
        self.i = i


def keys(indices):
    return [Key(i) for i in indices]


@pytest.fixture
def stub(monkeypatch):
    """Registry of 100 keys; committee slots 0, 1, 3 loaded with resident members, slot 2 without.
    Every engine entry records its arguments; the per-set entries answer from `outcomes`."""
    class Calls(list):
        pass

    calls = Calls()
    monkeypatch.setattr(bls.Registry, "_mirrored", 100)
    monkeypatch.setattr(bls.Committees, "_members", {0: tuple(C0), 1: tuple(C1), 2: tuple(C0), 3: tuple(C3)})
    monkeypatch.setattr(bls.Committees, "_resident", {0, 1, 3})

    def record(name, answer):
        def call(*args, **kw):
            calls.append((name,) + args)
            return answer(*args, **kw)
        return staticmethod(call)

    calls.each = None    # per set (sig status, key status, ok); default: all good
    calls.items = None   # per item bool

    def each_spans(msgs, *rest):
        return calls.each or [(0, 0, True)] * len(msgs)

    def each_points(msgs, sigs, keysets):
        return [(st, ok and kst == 0) for st, kst, ok in (calls.each or [(0, 0, True)] * len(msgs))]

    def items_spans(msgs, sigs, base, cbits, fields, lists, offsets, randoms=None, call_flags=0):
        return calls.items or [True] * (len(offsets) - 1)

    monkeypatch.setattr(bls.Signature, "multi_verify_compressed_spans", record("spans", lambda *a: 0))
    monkeypatch.setattr(bls.Signature, "multi_verify_compressed_bits", record("bits", lambda *a: 0))
    monkeypatch.setattr(bls.Signature, "multi_verify_compressed_committees", record("committees", lambda *a: 0))
    monkeypatch.setattr(bls.Signature, "multi_verify_compressed_indexed", record("indices", lambda *a: 0))
    monkeypatch.setattr(bls.Signature, "multi_verify_compressed", record("points", lambda *a: 0))
    monkeypatch.setattr(bls.Signature, "verify_each_spans", record("each_spans", each_spans))
    monkeypatch.setattr(bls.Signature, "verify_items_spans", record("items_spans", items_spans))
    monkeypatch.setattr(bls.Signature, "verify_batch_compressed", record("each_points", each_points))
    return calls


def block(mv, span=True, base=0, named=(0, 3), committees=(C0, C3)):
    mv.verify_aggregate_indexed(MSG, SIG, [40], keys([40]), None)                       # the proposer
    if span:
        mv.verify_aggregate_committees(MSG, SIG, base, list(named), list(committees), SPAN_BITS,
                                       keys(C0 + [30, 32, 33, 34]), None)
    mv.verify_aggregate_committee(MSG, SIG, 1, C1, RAW1, keys([8]), None)               # one committee, SSZ bytes
    mv.verify_aggregate_indexed(MSG, SIG, [41, 42], keys([41, 42]), None)               # no committee


def mixes():
    """(name, builder): every triple mix of tests/test_spans_mirror.py, qualifying or not."""
    def plain(mv):
        block(mv)

    def no_span(mv):
        block(mv, span=False)

    def slot_without_members(mv):
        block(mv, base=0, named=(0, 2), committees=(C0, C0[:5]))

    def other_member_list(mv):
        mv.verify_aggregate_committees(MSG, SIG, 0, [0, 3], [C0, C3[:4] + [50]], SPAN_BITS, keys(C0), None)

    def with_points(mv):
        mv.verify_aggregate_committees(MSG, SIG, 0, [0, 3], [C0, C3], SPAN_BITS, keys(C0), None)
        mv.verify_aggregate(MSG, SIG, keys([3]), None)

    def uncovered(mv):
        mv.verify_aggregate_committees(MSG, SIG, 0, [0, 3], [C0, C3], SPAN_BITS, keys(C0), None)
        mv.verify_aggregate_indexed(MSG, SIG, [200], keys([200]), None)

    def committee_without_members(mv):
        mv.verify_aggregate_committees(MSG, SIG, 0, [0, 3], [C0, C3], SPAN_BITS, keys(C0), None)
        mv.verify_aggregate_committee(MSG, SIG, 2, C0, [1] * 7 + [0], keys(C0[:7]), None)

    def span_alone(mv):
        mv.verify_aggregate_committees(MSG, SIG, 0, [0, 3], [C0, C3], SPAN_BITS, keys(C0), None)

    return [(f.__name__, f) for f in (plain, no_span, slot_without_members, other_member_list, with_points, uncovered,
                                      committee_without_members, span_alone)]


@pytest.mark.parametrize("name,build", mixes(), ids=[n for n, _ in mixes()])
def test_verify_each_takes_spans_exactly_when_finish_does(stub, name, build):
    mv = V.MultiVerifier()
    build(mv)
    mv.finish(randoms=list(range(1, len(mv.triples) + 1)))
    finish_call = stub[-1]
    del stub[:]
    assert mv.last_each_path is None
    assert mv.verify_each() == [True] * len(mv.triples)
    (call,) = stub
    assert (mv.last_each_path == "spans") == (mv.last_path == "spans") == (name in ("plain", "span_alone"))
    if mv.last_path == "spans":
        # the same sets, argument for argument: msgs, sigs, base slots, masks, bit strings, index lists
        assert call[0] == "each_spans" and finish_call[0] == "spans"
        assert call[1:] == finish_call[1:7] and len(call) == 7
    else:
        assert mv.last_each_path == "points" and call[0] == "each_points"
        assert [len(k) for k in call[3]] == [len(t.keys()) for t in mv.triples]


def test_verify_each_arguments_and_outcomes(stub):
    mv = V.MultiVerifier(options=[V.VerifierOption.BlockImport])
    block(mv)
    stub.each = [(0, 0, True), (0, G.BAD_ENCODING, False), (G.BAD_ENCODING, 0, False), (0, 0, False)]
    assert mv.verify_each() == [True, False, False, False]
    assert mv.last_each_path == "spans" and mv.last_each_status == [(0, 0), (0, 1), (1, 0), (0, 0)]
    (name, msgs, sigs, bases, masks, fields, lists), = stub
    assert name == "each_spans" and len(msgs) == len(sigs) == 4
    assert bases == [None, 0, 1, None]
    assert [bytes(m) for m in masks] == [bytes(8), bytes([0b1001]) + bytes(7), bytes([1]) + bytes(7), bytes(8)]
    assert [bytes(f) for f in fields] == [b"", bytes([0xFF, 0b00011101]), RAW1, b""]
    assert [list(v) for v in lists] == [[40], [], [], [41, 42]]
    # a status without a verdict never counts as verified
    stub.each = [(0, 0, True), (0, G.BAD_ENCODING, True), (G.BAD_ENCODING, 0, True), (0, 0, True)]
    assert mv.verify_each() == [True, False, False, True]
    assert V.MultiVerifier().verify_each() == []


def test_verify_each_falls_back_to_points_without_members(stub, monkeypatch):
    mv = V.MultiVerifier()
    block(mv)
    assert mv.verify_each() == [True] * 4 and mv.last_each_path == "spans"
    # the same triples with slot 3 loaded without members
    monkeypatch.setattr(bls.Committees, "_resident", {0, 1})
    del stub[:]
    stub.each = [(0, 0, True), (0, 0, False), (0, 0, True), (1, 0, False)]
    assert mv.verify_each() == [True, False, True, False]
    assert mv.last_each_path == "points" and mv.last_each_status is None
    (name, msgs, sigs, keysets), = stub
    assert name == "each_points" and [[k.i for k in ks] for ks in keysets] == [[40], C0 + [30, 32, 33, 34], [8], [41, 42]]


def test_verify_items_maps_triples_to_items(stub):
    mv = V.MultiVerifier(options=[V.VerifierOption.BlockImport])
    block(mv)
    block(mv)
    owner = [0, 0, 0, 2, 2, 3, 3, 3]   # item 1 has no triple
    stub.items = [True, False, False, True]
    assert mv.verify_items(owner, randoms=list(range(1, 9))) == [True, False, False, True]
    assert mv.last_each_path == "spans"
    (name, msgs, sigs, bases, masks, fields, lists, offsets, randoms, flags), = stub
    assert name == "items_spans" and offsets == [0, 3, 3, 5, 8] and randoms == list(range(1, 9)) and flags == G.CALL_BLOCK
    assert bases == [None, 0, 1, None] * 2 and len(msgs) == len(sigs) == len(masks) == len(fields) == len(lists) == 8
    for bad in ([0, 0, 1], [0, 1, 0, 1, 1, 1, 1, 1], [-1] + [0] * 7):
        with pytest.raises(ValueError):
            mv.verify_items(bad)
    assert V.MultiVerifier().verify_items([]) == []


def test_verify_items_without_members_decides_set_by_set(stub, monkeypatch):
    monkeypatch.setattr(bls.Committees, "_resident", {0, 1})
    mv = V.MultiVerifier()
    block(mv)
    block(mv)
    stub.each = [(0, 0, True)] * 5 + [(0, 0, False)] + [(0, 0, True)] * 2
    assert mv.verify_items([0, 0, 0, 2, 2, 3, 3, 3]) == [True, False, True, False]
    assert mv.last_each_path == "points" and [c[0] for c in stub] == ["each_points"]


def test_split_failed_batch_from_per_set_outcomes(stub):
    """Five gossip aggregates of three sets (selection proof, aggregate-and-proof signature,
    attestation over two committees), one item whose sets cannot be built."""
    def item():
        proof, outer, att = V.Triple(), V.Triple(), V.Triple()
        proof.verify_aggregate_indexed(MSG, SIG, [40], keys([40]))
        outer.verify_aggregate_indexed(MSG, SIG, [40], keys([40]))
        att.verify_aggregate_committees(MSG, SIG, 0, [0, 3], [C0, C3], SPAN_BITS, keys(C0 + [30, 32, 33, 34]))
        return [proof, outer, att]

    items = ["a", "b", "c", "d", "e", "f"]
    triples = [item(), item(), None, item(), item(), item()]
    good = (0, 0, True)
    stub.each = [good] * 3 + [good, good, (0, 0, False)] + [good] * 3 + [(1, 0, False), good, good] + [good, good, (0, 1, False)]
    passed, failing = V.split_failed_batch(items, triples)
    assert (passed, failing) == (["a", "d"], ["b", "c", "e", "f"])
    (call,) = stub
    assert call[0] == "each_spans" and len(call[1]) == 15 and call[3] == [None, None, 0] * 5
    with pytest.raises(ValueError):
        V.split_failed_batch(items, triples[:-1])


def test_signature_entries_marshal_the_sets(monkeypatch):
    got = {}

    def sets(msgs, sigs, com, masks, bits, boff, idx, off, n):
        return dict(com=list(com)[:n], masks=masks.raw[:8 * n], bits=bits.raw[:boff[n]], boff=list(boff)[:n + 1],
                    idx=list(idx)[:off[n]], off=list(off)[:n + 1], n=n)

    class Lib:
        def gbls_verify_each_spans(self, msgs, sigs, com, masks, bits, boff, idx, off, n, st, kst, v):
            got.update(sets(msgs, sigs, com, masks, bits, boff, idx, off, n))
            st[1], kst[2] = 3, 1
            v[0], v[1], v[2] = 0, 5, 5
            return 0

        def gbls_verify_items_spans(self, msgs, sigs, com, masks, bits, boff, idx, off, rands, n, seg, nseg, st, kst, v,
                                    flags):
            got.update(sets(msgs, sigs, com, masks, bits, boff, idx, off, n), rands=list(rands)[:n],
                       seg=list(seg)[:nseg + 1], nseg=nseg, flags=flags)
            kst[2] = 4
            v[0], v[1] = 5, 0
            return 0

        def gbls_last_error(self):
            return 0

    monkeypatch.setattr(G, "lib", lambda *a: Lib())
    args = ([MSG] * 3, [SIG] * 3, [7, None, 2], [bytes([5]) + bytes(7), None, bytes(7) + bytes([0x80])],
            [b"\x1f\x02", b"", b"\x03"], [(), [4, 9], ()])
    want = dict(com=[7, G.NO_COMMITTEE, 2], masks=bytes([5]) + bytes(15) + bytes(7) + bytes([0x80]),
                bits=b"\x1f\x02\x03", boff=[0, 2, 2, 3], idx=[4, 9], off=[0, 0, 2, 2], n=3)
    assert bls.Signature.verify_each_spans(*args) == [(0, 0, True), (3, 0, False), (0, 1, False)]
    assert got == want
    got.clear()
    assert bls.Signature.verify_items_spans(*args, [0, 1, 3], randoms=[3, 4, 5], call_flags=1) == [False, True]
    assert got == dict(want, rands=[3, 4, 5], seg=[0, 1, 3], nseg=2, flags=1)
    verdicts, statuses = bls.Signature.verify_items_spans(*args, [0, 1, 3], randoms=[3, 4, 5], with_statuses=True)
    assert verdicts == [False, True] and statuses == [(0, 0), (0, 0), (0, 4)]
    assert bls.Signature.verify_each_spans([], [], [], [], [], []) == []
    assert bls.Signature.verify_items_spans([], [], [], [], [], [], [0]) == []
    for bad in ([0, 2], [1, 3], [0, 2, 1, 3]):
        with pytest.raises(ValueError):
            bls.Signature.verify_items_spans(*args, bad)
    with pytest.raises(ValueError):
        bls.Signature.verify_each_spans([MSG], [SIG], [0], [bytes(7)], [b"\x03"], [()])
