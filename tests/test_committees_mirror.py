"""CPU: the Python mirror of the cached committee key sums, with the engine calls stubbed:
Triple.verify_aggregate_committee keeps the participants' indices, the slot and the absentees; a
reused Triple keeps nothing stale; MultiVerifier.finish takes the "committees" path only when the
registry and the committee table cover every triple, and sends the shorter list per triple."""
import pytest

from grandine_amd import _lib as G
from grandine_amd import bls, verifier as V

MSG = bytes(range(32))
SIG = bytes(96)


class Key:  # stands for a bls.PublicKey: the stubbed engine never looks inside
    def __init__(self, i):
        self.i = i


def keys(indices):
    return [Key(i) for i in indices]


def committee_triple(slot, committee, bits):
    t = V.Triple()
    t.verify_aggregate_committee(MSG, SIG, slot, committee, bits, keys(v for v, b in zip(committee, bits) if b))
    return t


def test_committee_triple_fields():
    t = committee_triple(7, [10, 11, 12, 13], [1, 0, 1, 1])
    assert (t.slot, t.committee, t.absent, t.indices) == (7, [10, 11, 12, 13], [11], [10, 12, 13])
    assert [k.i for k in t.deferred] == [10, 12, 13]
    with pytest.raises(ValueError):
        V.Triple().verify_aggregate_committee(MSG, SIG, 0, [1, 2], [1], keys([1]))


def test_reused_triple_keeps_nothing_stale():
    t = committee_triple(7, [10, 11, 12, 13], [1, 0, 1, 1])
    t.verify_aggregate(MSG, SIG, keys([5, 6]))
    assert t.indices is None and t.slot is None and t.committee is None and t.absent is None
    assert [k.i for k in t.deferred] == [5, 6]
    t.verify_aggregate_committee(MSG, SIG, 3, [20, 21], [1, 1], keys([20, 21]))
    t.verify_aggregate_indexed(MSG, SIG, [8, 9], keys([8, 9]))
    assert t.indices == [8, 9] and t.slot is None and t.committee is None and t.absent is None
    # ... and an indexed triple reused for a plain aggregate drops its indices
    t.verify_aggregate(MSG, SIG, keys([1]))
    assert t.indices is None


@pytest.fixture
def stub(monkeypatch):
    """Registry of 100 keys, committee slots 0 and 1 loaded; the three engine calls recorded."""
    calls = []
    monkeypatch.setattr(bls.Registry, "_mirrored", 100)
    monkeypatch.setattr(bls.Committees, "_members", {0: tuple(range(0, 8)), 1: tuple(range(8, 16))})

    def record(name):
        def call(*args):
            calls.append((name,) + args)
            return 0
        return staticmethod(call)

    monkeypatch.setattr(bls.Signature, "multi_verify_compressed_committees", record("committees"))
    monkeypatch.setattr(bls.Signature, "multi_verify_compressed_indexed", record("indices"))
    monkeypatch.setattr(bls.Signature, "multi_verify_compressed", record("points"))
    return calls


def test_finish_sends_the_shorter_list(stub):
    mv = V.MultiVerifier()
    c0, c1 = list(range(0, 8)), list(range(8, 16))
    mv.verify_aggregate_committee(MSG, SIG, 0, c0, [1] * 8, keys(c0), None)  # nobody absent
    mv.verify_aggregate_committee(MSG, SIG, 1, c1, [1, 1, 0, 1, 1, 1, 0, 1], keys([8, 9, 11, 12, 13, 15]), None)
    mv.verify_aggregate_committee(MSG, SIG, 1, c1, [0, 0, 1, 0, 0, 0, 1, 0], keys([10, 14]), None)  # 6 absent
    mv.verify_aggregate_committee(MSG, SIG, 0, c0, [1, 1, 1, 1, 0, 0, 0, 0], keys(c0[:4]), None)  # a tie
    mv.verify_aggregate_indexed(MSG, SIG, [40, 41], keys([40, 41]), None)  # no committee
    mv.finish(randoms=[1, 2, 3, 4, 5])
    assert mv.last_path == "committees"
    (name, msgs, sigs, slots, lists, randoms, flags), = stub
    assert name == "committees" and len(msgs) == len(sigs) == 5 and randoms == [1, 2, 3, 4, 5] and flags == 0
    assert slots == [0, 1, None, None, None]
    assert lists == [[], [10, 14], [10, 14], [0, 1, 2, 3], [40, 41]]


def test_finish_falls_back_when_not_covered(stub):
    c0 = list(range(0, 8))

    def batch(slot, committee):
        mv = V.MultiVerifier(options=[V.VerifierOption.BlockImport])
        mv.verify_aggregate_committee(MSG, SIG, slot, committee, [1] * 7 + [0], keys(committee[:7]), None)
        mv.finish(randoms=[9])
        return mv.last_path

    assert batch(0, c0) == "committees" and stub[-1][-1] == G.CALL_BLOCK
    assert batch(5, c0) == "indices"  # a slot that is not loaded
    assert stub[-1][0] == "indices" and stub[-1][3] == [c0[:7]]
    assert batch(1, c0) == "indices"  # a slot loaded with another member list
    bls.Committees.forget()
    assert batch(0, c0) == "indices"
    # the registry does not cover a participant: key points, as before
    mv = V.MultiVerifier()
    mv.verify_aggregate_committee(MSG, SIG, 0, [0, 1, 200], [1, 1, 1], keys([0, 1, 200]), None)
    mv.finish(randoms=[9])
    assert mv.last_path == "points" and stub[-1][0] == "points"
    # without any committee triple the indexed path runs as before
    mv = V.MultiVerifier()
    mv.verify_aggregate_indexed(MSG, SIG, [1, 2], keys([1, 2]), None)
    mv.finish(randoms=[9])
    assert mv.last_path == "indices"


def test_registry_forget_forgets_the_committees(stub):
    assert bls.Committees.covers(0, range(0, 8)) and not bls.Committees.covers(0, range(0, 7))
    assert not bls.Committees.covers(None, range(0, 8))
    bls.Registry.forget()
    assert not bls.Committees.covers(0, range(0, 8))
