"""CPU: the Python mirror of the aggregation-bit sets, with the engine calls stubbed:
Triple.verify_aggregate_committee keeps the aggregation bits as SSZ bytes (bytes passed through, a
sequence of bools packed as a Bitvector); MultiVerifier.finish takes the "bits" path exactly when
every committee triple's slot has resident members and every other triple is registry-indexed, and
passes slots, raw bit bytes and the plain sets' index lists in set order; otherwise it takes the
paths it took before."""
import pytest

from grandine_amd import _lib as G
from grandine_amd import bls, verifier as V

MSG = bytes(range(32))
SIG = bytes(96)
C0, C1 = list(range(0, 8)), list(range(8, 19))  # 8 and 11 members


class Key:  # stands for a bls.PublicKey: the stubbed engine never looks inside
    def __init__(self, i):
        self.i = i


def keys(indices):
    return [Key(i) for i in indices]


def test_triple_keeps_the_bits():
    t = V.Triple()
    assert t.bits is None
    t.verify_aggregate_committee(MSG, SIG, 1, C1, [1, 0, 1, 1, 1, 1, 1, 1, 0, 1, 1], keys([8]))
    assert t.bits == bytes([0b11111101, 0b00000110])  # a Bitvector[11], SSZ bit order
    assert t.absent == [9, 16] and t.indices == [8, 10, 11, 12, 13, 14, 15, 17, 18]
    # bytes are the SSZ encoding, passed through: a Bitlist[..] of 11 bits with its delimiter
    raw = bytes([0b11111101, 0b00001110])
    t.verify_aggregate_committee(MSG, SIG, 1, C1, raw, keys([8]))
    assert t.bits == raw and t.absent == [9, 16] and t.indices == [8, 10, 11, 12, 13, 14, 15, 17, 18]
    # ... of 8 bits: the delimiter has a byte of its own
    t.verify_aggregate_committee(MSG, SIG, 0, C0, bytes([0x0F, 0x01]), keys(C0[:4]))
    assert t.bits == bytes([0x0F, 0x01]) and t.absent == C0[4:] and t.indices == C0[:4]
    with pytest.raises(ValueError):
        V.Triple().verify_aggregate_committee(MSG, SIG, 1, C1, bytes([0xFF]), keys([8]))  # too short for 11 members
    # a reused triple keeps nothing stale
    t.verify_aggregate_indexed(MSG, SIG, [8, 9], keys([8, 9]))
    assert t.bits is None and t.slot is None


@pytest.fixture
def stub(monkeypatch):
    """Registry of 100 keys, committee slots 0 and 1 loaded, slot 0 and 1 with resident members
    unless a test says otherwise; the four engine calls recorded."""
    calls = []
    monkeypatch.setattr(bls.Registry, "_mirrored", 100)
    monkeypatch.setattr(bls.Committees, "_members", {0: tuple(C0), 1: tuple(C1), 2: tuple(C0)})
    monkeypatch.setattr(bls.Committees, "_resident", {0, 1})

    def record(name):
        def call(*args):
            calls.append((name,) + args)
            return 0
        return staticmethod(call)

    monkeypatch.setattr(bls.Signature, "multi_verify_compressed_bits", record("bits"))
    monkeypatch.setattr(bls.Signature, "multi_verify_compressed_committees", record("committees"))
    monkeypatch.setattr(bls.Signature, "multi_verify_compressed_indexed", record("indices"))
    monkeypatch.setattr(bls.Signature, "multi_verify_compressed", record("points"))
    return calls


def block(mv, slot1=1):
    raw1 = bytes([0b11111101, 0b00001110])
    mv.verify_aggregate_indexed(MSG, SIG, [40], keys([40]), None)                       # the proposer
    mv.verify_aggregate_committee(MSG, SIG, 0, C0, [1] * 7 + [0], keys(C0[:7]), None)   # bools
    mv.verify_aggregate_committee(MSG, SIG, slot1, C1 if slot1 == 1 else C0, raw1 if slot1 == 1 else bytes([0xFF]),
                                  keys([8]), None)                                      # SSZ bytes
    mv.verify_aggregate_indexed(MSG, SIG, [41, 42], keys([41, 42]), None)               # no committee
    return raw1


def test_finish_takes_the_bits_path(stub):
    mv = V.MultiVerifier(options=[V.VerifierOption.BlockImport])
    raw1 = block(mv)
    mv.finish(randoms=[1, 2, 3, 4])
    assert mv.last_path == "bits"
    (name, msgs, sigs, slots, fields, lists, randoms, flags), = stub
    assert name == "bits" and len(msgs) == len(sigs) == 4 and randoms == [1, 2, 3, 4] and flags == G.CALL_BLOCK
    assert slots == [None, 0, 1, None]
    assert [bytes(f) for f in fields] == [b"", bytes([0x7F]), raw1, b""]
    assert [list(v) for v in lists] == [[40], [], [], [41, 42]]


def test_finish_keeps_its_paths_otherwise(stub):
    # one committee slot lacks members: the committees path, with the lists it sent before
    mv = V.MultiVerifier()
    block(mv, slot1=2)
    mv.finish(randoms=[1, 2, 3, 4])
    assert mv.last_path == "committees" and [c[0] for c in stub] == ["committees"]
    assert stub[-1][3] == [None, 0, 2, None] and stub[-1][4] == [[40], [7], [], [41, 42]]
    # a resident slot whose member list is not the triple's committee
    mv = V.MultiVerifier()
    mv.verify_aggregate_committee(MSG, SIG, 0, C0[:7] + [50], [1] * 8, keys(C0[:7] + [50]), None)
    mv.finish(randoms=[9])
    assert mv.last_path == "indices"
    # another triple is not registry-indexed (key points only), or names a key past the mirror
    for other in ("points", "uncovered"):
        mv = V.MultiVerifier()
        mv.verify_aggregate_committee(MSG, SIG, 0, C0, [1] * 8, keys(C0), None)
        if other == "points":
            mv.verify_aggregate(MSG, SIG, keys([3]), None)
        else:
            mv.verify_aggregate_indexed(MSG, SIG, [200], keys([200]), None)
        mv.finish(randoms=[9, 9])
        assert mv.last_path == "points", other
    # no committee triple at all
    mv = V.MultiVerifier()
    mv.verify_aggregate_indexed(MSG, SIG, [1, 2], keys([1, 2]), None)
    mv.finish(randoms=[9])
    assert mv.last_path == "indices"
    assert not any(c[0] == "bits" for c in stub)


def test_committees_mirror_tracks_resident_slots(monkeypatch):
    """Committees.set(members=True) calls the new entry and remembers the slots; the default path
    calls gbls_committees_set as before and forgets them."""
    calls = []

    class Lib:
        def gbls_committees_set(self, first, idx, off, n, st):
            calls.append(("set", first, list(idx)[:off[n]], list(off)[:n + 1], n))
            return 0

        def gbls_committees_set_members(self, first, idx, off, n, st):
            calls.append(("set_members", first, list(idx)[:off[n]], list(off)[:n + 1], n))
            st[1] = G.BAD_ENCODING  # the second committee is rejected
            return 0

        def gbls_committees_clear(self):
            return 0

    monkeypatch.setattr(G, "lib", lambda *a: Lib())
    monkeypatch.setattr(bls.Committees, "_members", {})
    monkeypatch.setattr(bls.Committees, "_resident", set())
    assert bls.Committees.set(4, [[1, 2, 3], [4], [5, 6]], members=True) == [0, G.BAD_ENCODING, 0]
    assert calls[-1] == ("set_members", 4, [1, 2, 3, 4, 5, 6], [0, 3, 4, 6], 3)
    assert [bls.Committees.has_members(s) for s in (3, 4, 5, 6, 7, None)] == [False, True, False, True, False, False]
    assert bls.Committees.covers(6, [5, 6]) and not bls.Committees.covers(5, [4])
    assert bls.Committees.set(6, [[5, 6]]) == [0]  # the default: the plain entry, members dropped
    assert calls[-1] == ("set", 6, [5, 6], [0, 2], 1)
    assert bls.Committees.covers(6, [5, 6]) and not bls.Committees.has_members(6) and bls.Committees.has_members(4)
    bls.Committees.clear()
    assert not bls.Committees.has_members(4)
