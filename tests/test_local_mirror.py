"""CPU: the Python mirror of the local key set calls, with the engine calls stubbed:
Triple.verify_singular_bytes keeps the 48 bytes and performs no host decode; MultiVerifier.finish,
verify_each and verify_items let such triples ride along as local sets exactly when the other
triples qualify for "spans" (last_path / last_each_path == "local": the span sets argument for
argument, a LOCAL_KEYS base with a table position per kept key, a key that several triples name in
the table once), and otherwise decode the kept bytes through the engine and take today's path;
the Signature entries marshal the table and return its statuses."""
import pytest

from grandine_amd import _lib as G
from grandine_amd import bls, verifier as V

import test_each_mirror as M
from test_each_mirror import MSG, SIG, keys
from test_each_mirror import stub as each_stub  # noqa: F401  (fixture: the registry, the slots, the earlier entries)

KA, KB = bytes([0xA0]) + bytes(47), bytes([0xB0]) + bytes(47)


@pytest.fixture
def stub(each_stub, monkeypatch):  # noqa: F811
    calls = each_stub
    calls.each_local = None   # (per set (sig status, key status, ok), per table key status)
    calls.items_local = None  # (per item bool, per set (sig status, key status), per table key status)
    calls.decoded = []

    def record(name, answer):
        def call(*args, **kw):
            calls.append((name,) + args)
            return answer(*args, **kw)
        return staticmethod(call)

    def each_local(msgs, sigs, base, cbits, fields, lists, table):
        return calls.each_local or ([(0, 0, True)] * len(msgs), [0] * len(table))

    def items_local(msgs, sigs, base, cbits, fields, lists, table, offsets, randoms=None, call_flags=0,
                    with_statuses=False):
        verdicts, statuses, pst = calls.items_local or ([True] * (len(offsets) - 1), [(0, 0)] * len(msgs), [0] * len(table))
        return (verdicts, statuses, pst) if with_statuses else verdicts

    def try_from(data):
        calls.decoded.append(bytes(data))
        return M.Key(("decoded", bytes(data)))

    monkeypatch.setattr(bls.Signature, "verify_each_local", record("each_local", each_local))
    monkeypatch.setattr(bls.Signature, "verify_items_local", record("items_local", items_local))
    monkeypatch.setattr(bls.PublicKey, "try_from", staticmethod(try_from))
    return calls


def with_deposits(mv, span=True, **kw):
    mv.verify_singular_bytes(MSG, SIG, KA)                                   # a deposit
    M.block(mv, span=span, **kw)
    mv.verify_singular_bytes(MSG, SIG, KB)                                   # an address change
    mv.verify_singular_bytes(MSG, SIG, KA)                                   # the first key again


def test_kept_bytes_are_not_decoded():
    t = V.Triple()
    t.verify_singular_bytes(MSG, SIG, KA)
    assert t.key_bytes == KA and t.deferred is None and t.indices is None and t._key is None
    with pytest.raises(ValueError):
        t.verify_singular_bytes(MSG, SIG, KA[:47])
    t.verify_aggregate(MSG, SIG, keys([1]), None)   # a reused triple keeps nothing of its previous set
    assert t.key_bytes is None


def test_finish_takes_the_local_path_when_the_rest_qualifies(stub):
    mv = V.MultiVerifier(options=[V.VerifierOption.BlockImport])
    with_deposits(mv)
    n = len(mv.triples)
    assert n == 7
    rands = list(range(1, n + 1))
    assert mv.finish(randoms=rands) is None and mv.last_path == "local"
    (call,) = stub
    name, msgs, sigs, base, cbits, fields, lists, table, offsets, randoms, flags = call
    assert name == "items_local" and offsets == [0, n] and randoms == rands and flags == G.CALL_BLOCK
    assert table == [KA, KB] and not stub.decoded                           # each key once, no host decode
    assert base == [G.LOCAL_KEYS, None, 0, 1, None, G.LOCAL_KEYS, G.LOCAL_KEYS]
    assert [list(v) for v in lists] == [[0], [40], [], [], [41, 42], [1], [0]]
    assert cbits[0] == cbits[5] == bytes(8) and fields[0] == fields[5] == b""
    # the other triples exactly as the "spans" path sends them
    del stub[:]
    rest = V.MultiVerifier()
    M.block(rest)
    rest.finish(randoms=[1, 2, 3, 4])
    assert rest.last_path == "spans"
    spans = stub[-1]
    for k in (3, 4, 5, 6):
        assert list(spans[k]) == list(call[k][1:5])


def test_finish_verdicts_and_decoding_errors(stub):
    def run(answer):
        mv = V.MultiVerifier()
        with_deposits(mv)
        stub.items_local = answer
        return mv
    n = 7
    with pytest.raises(V.SignatureInvalid):
        run(([False], [(0, 0)] * n, [0, 0])).finish()
    with pytest.raises(bls.DecompressionFailed):    # a signature that does not decode comes first
        run(([False], [(0, 0)] * 3 + [(G.BAD_ENCODING, 0)] + [(0, 0)] * 3, [0, 3])).finish()
    with pytest.raises(bls.DecompressionFailed):    # then a local key that does not
        run(([False], [(0, 0)] * 6 + [(0, G.BAD_ENCODING)], [0, 3])).finish()
    with pytest.raises(V.SignatureInvalid):          # a rejected span set is a failed batch, as on "spans"
        run(([False], [(0, 0), (0, 0), (0, G.BAD_ENCODING)] + [(0, 0)] * 4, [0, 0])).finish()


@pytest.mark.parametrize("name,build", M.mixes(), ids=[n for n, _ in M.mixes()])
def test_local_exactly_when_the_rest_takes_spans(stub, name, build):
    mv = V.MultiVerifier()
    mv.verify_singular_bytes(MSG, SIG, KA)
    build(mv)
    n = len(mv.triples)
    mv.finish(randoms=list(range(1, n + 1)))
    qualifies = name in ("plain", "span_alone")
    assert (mv.last_path == "local") == qualifies
    assert mv.verify_each() == [True] * n and (mv.last_each_path == "local") == qualifies
    assert mv.verify_items([0] * n) == [True]
    if qualifies:
        assert [c[0] for c in stub] == ["items_local", "each_local", "items_local"] and not stub.decoded
    else:
        # decoded through the engine, once, and today's path: no registry index, so key points
        assert mv.last_path == "points" and mv.last_each_path == "points" and stub.decoded == [KA]
        assert [c[0] for c in stub] == ["points", "each_points", "each_points"]
        assert stub[0][3][0][0].i == ("decoded", KA)


def test_verify_each_and_items_outcomes(stub):
    mv = V.MultiVerifier(options=[V.VerifierOption.BlockImport])
    with_deposits(mv)
    stub.each_local = ([(0, 0, True), (0, 0, True), (0, G.BAD_ENCODING, False), (G.BAD_ENCODING, 0, False), (0, 0, False),
                        (0, G.BAD_ENCODING, False), (0, 0, True)], [0, 3])
    assert mv.verify_each() == [True, True, False, False, False, False, True]
    assert mv.last_each_path == "local" and mv.last_each_status[5] == (0, G.BAD_ENCODING)
    stub.items_local = ([True, False, True], [(0, 0)] * 7, [0, 0])
    del stub[:]
    assert mv.verify_items([0, 0, 0, 1, 1, 2, 2], randoms=[9] * 7) == [True, False, True]
    (call,) = stub
    assert call[0] == "items_local" and call[8] == [0, 3, 5, 7] and call[9] == [9] * 7 and call[10] == G.CALL_BLOCK
    assert mv.last_each_path == "local"
    # without kept bytes nothing changes
    del stub[:]
    mv = V.MultiVerifier()
    M.block(mv)
    assert mv.verify_each() == [True] * 4 and mv.last_each_path == "spans" and stub[0][0] == "each_spans"


def test_signature_entries_marshal_the_table(monkeypatch):
    seen = {}

    class Lib:
        def gbls_verify_each_local(self, msgs, sigs, com, masks, bits, boff, idx, off, pkb, npkb, n, st, kst, v, pst):
            seen["each"] = (bytes(pkb.raw[:48 * npkb]) if npkb else None, npkb, n, [com[i] for i in range(n)],
                            [off[i] for i in range(n + 1)], [idx[i] for i in range(off[n])])
            for i in range(n):
                st[i], kst[i], v[i] = 0, (1 if i == 2 else 0), (5 if i == 2 else 0)
            for j in range(npkb):
                pst[j] = 3 * j
            return 0

        def gbls_verify_items_local(self, msgs, sigs, com, masks, bits, boff, idx, off, pkb, npkb, rands, n, seg, nseg, st,
                                    kst, v, pst, flags):
            seen["items"] = (npkb, n, nseg, [seg[s] for s in range(nseg + 1)], [rands[i] for i in range(n)], flags)
            for i in range(n):
                st[i], kst[i] = 0, 0
            for s in range(nseg):
                v[s] = 5 * (s % 2)
            for j in range(npkb):
                pst[j] = 6
            return 0

    monkeypatch.setattr(G, "lib", lambda *a, **k: Lib())
    args = ([MSG] * 3, [SIG] * 3, [G.LOCAL_KEYS, None, G.LOCAL_KEYS], [bytes(8)] * 3, [b""] * 3, [[1], [7, 8], [0, 1]])
    per_set, pst = bls.Signature.verify_each_local(*args, [KA, KB])
    assert per_set == [(0, 0, True), (0, 0, True), (0, 1, False)] and pst == [0, 3]
    assert seen["each"] == (KA + KB, 2, 3, [G.LOCAL_KEYS, G.NO_COMMITTEE, G.LOCAL_KEYS], [0, 1, 3, 5], [1, 7, 8, 0, 1])
    assert bls.Signature.verify_items_local(*args, [KA, KB], [0, 1, 3], randoms=[3, 4, 5], call_flags=1) == [True, False]
    assert seen["items"] == (2, 3, 2, [0, 1, 3], [3, 4, 5], 1)
    verdicts, statuses, pst = bls.Signature.verify_items_local(*args, [KA, KB], [0, 1, 3], randoms=[3, 4, 5],
                                                               with_statuses=True)
    assert verdicts == [True, False] and statuses == [(0, 0)] * 3 and pst == [6, 6]
    assert bls.Signature.verify_each_local([], [], [], [], [], [], []) == ([], [])
    assert bls.Signature.verify_items_local([], [], [], [], [], [], [], [0]) == []
    with pytest.raises(ValueError):
        bls.Signature.verify_each_local(*args, [KA[:47]])
    with pytest.raises(ValueError):
        bls.Signature.verify_items_local(*args, [KA], [0, 2])
