"""CPU: the Python mirror of the verified folds, with the engine calls stubbed.

* pools.fold_verified_singles against a restatement of aggregate_attestation's loop
  (operation_pools/src/attestation_agg_pool/tasks.rs:189-191, 242-257) over aggregates with random
  bits and singles with distinct positions: the same bits and the same signature as the reference
  loop over the singles that verify; a later single of an already-planned position is returned as
  deferred, not dropped, and is a candidate of the next call if its position is still missing;
* MultiVerifier.verify_each_fold sends triples in the "spans" form, or over registry indices alone,
  to bls.Signature.verify_each_fold (last_each_path == "fold" when groups were sent), refuses
  triples over key points, and leaves verify_each as it was;
* bls.Signature.verify_each_fold marshals the groups as CSR and reads the three fold outputs.

The stubbed engine answers with the Python oracle's arithmetic over small multiples of the G2
generator (the stub decides which singles verify; no pairing is computed here)."""
import random

import pytest

from grandine_amd import _lib as G
from grandine_amd import bls, pools, verifier as V
from oracle import bls12_381 as O

import test_each_mirror as M
from test_each_mirror import MSG, SIG
from test_each_mirror import stub as each_stub  # noqa: F401  (fixture: the registry, the slots, the earlier entries)

INF_BYTES = bytes([0xC0]) + bytes(95)


def mont(a):
    return (a * (1 << 384) % O.P).to_bytes(48, "little")


def raw(pt):
    if pt is None:
        return bytes(192)
    (x0, x1), (y0, y1) = pt
    return mont(x0) + mont(x1) + mont(y0) + mont(y1)


def point(raw_bytes):
    rinv = pow(1 << 384, -1, O.P)
    v = [int.from_bytes(raw_bytes[48 * k:48 * (k + 1)], "little") * rinv % O.P for k in range(4)]
    return None if not any(v) else ((v[0], v[1]), (v[2], v[3]))


def dec(data):
    return O.g2_decompress(bytes(data))[1]


def compress(pt):
    return INF_BYTES if pt is None else O.g2_compress(pt)


@pytest.fixture
def engine(each_stub, monkeypatch):  # noqa: F811
    """bls.Signature.verify_each_fold and Signature.aggregate answered by the oracle.  A signature
    verifies unless its bytes are in calls.invalid."""
    calls = each_stub
    calls.invalid = set()

    def each_fold(msgs, sigs, base, cbits, fields, lists, groups):
        calls.append(("each_fold", list(msgs), list(sigs), list(base), list(cbits), list(fields), [list(v) for v in lists],
                      [list(g) for g in groups]))
        oks = [bytes(s) not in calls.invalid for s in sigs]
        folds = []
        for g in groups:
            members = [s for s in g if oks[s]]
            total = O.aggregate_signatures([dec(bytes(sigs[s])) for s in members])
            folds.append((bls.Signature(raw(total)), len(members), bls.SignatureBytes(compress(total))))
        return [(0, 0, ok) for ok in oks], folds

    def aggregate(self, other):
        calls.append(("add",))
        return bls.Signature(raw(O.g2_add(point(self.raw), point(other.raw))))

    monkeypatch.setattr(bls.Signature, "verify_each_fold", staticmethod(each_fold))
    monkeypatch.setattr(bls.Signature, "aggregate", aggregate)
    return calls


def reference_loop(bits, signature, singles, verifies):
    """InsertAttestationTask over singular attestations that passed verification: per single,
    aggregate_attestation (any_not_in -> |= and aggregate_in_place)."""
    bits = list(bits)
    for pos, _, sig, _ in singles:
        if not verifies(sig):
            continue  # never inserted into the pool
        if not bits[pos]:
            bits[pos] = True
            signature = O.g2_add(signature, dec(sig))
    return bits, signature


@pytest.mark.parametrize("seed", range(6))
def test_fold_verified_singles_matches_the_reference_loop(engine, seed):
    rnd = random.Random(seed)
    size = 24
    bits = [rnd.random() < 0.4 for _ in range(size)]
    start = O.g2_mul(O.G2_GEN, rnd.randrange(1, O.R)) if any(bits) else None
    positions = rnd.sample(range(size), 14)          # distinct positions, some already in the aggregate
    singles = [(pos, MSG, O.g2_compress(O.g2_mul(O.G2_GEN, 1000 * seed + pos + 2)), 10 + pos) for pos in positions]
    engine.invalid = {singles[k][2] for k in rnd.sample(range(len(singles)), 4)}
    agg = pools.Aggregate(size, bls.Signature(raw(start)), bits)
    verified, deferred = pools.fold_verified_singles(agg, singles)
    want_bits, want_sig = reference_loop(bits, start, singles, lambda s: s not in engine.invalid)
    assert agg.bits == want_bits and agg.signature.raw == raw(want_sig) and deferred == []
    candidates = [k for k, (pos, _, _, _) in enumerate(singles) if not bits[pos]]
    assert [k for k, v in enumerate(verified) if v is not None] == candidates
    assert all(verified[k] == (singles[k][2] not in engine.invalid) for k in candidates)
    fold_calls = [c for c in engine if c[0] == "each_fold"]
    if candidates:
        (call,) = fold_calls
        # ONE submission: the candidates as plain sets of one registry index, one group of all
        assert call[2] == [singles[k][2] for k in candidates] and call[3] == [None] * len(candidates)
        assert call[6] == [[singles[k][3]] for k in candidates] and call[7] == [list(range(len(candidates)))]
        # and at most ONE host addition
        assert sum(1 for c in engine if c[0] == "add") == (1 if any(verified[k] for k in candidates) else 0)
    else:
        assert fold_calls == []


def test_a_repeated_position_is_deferred_not_dropped(engine):
    size = 8
    sig = [O.g2_compress(O.g2_mul(O.G2_GEN, k + 2)) for k in range(5)]
    singles = [(1, MSG, sig[0], 11), (4, MSG, sig[1], 14), (1, MSG, sig[2], 11), (6, MSG, sig[3], 16), (4, MSG, sig[4], 14)]
    engine.invalid = {sig[0]}                         # the first single of position 1 does not verify
    agg = pools.Aggregate(size, bls.Signature(bytes(192)), [False] * 5 + [False, True, False])   # position 6 is there
    verified, deferred = pools.fold_verified_singles(agg, singles)
    assert verified == [False, True, None, None, None] and deferred == [2, 4]
    assert agg.bits == [False, False, False, False, True, False, True, False]
    assert agg.signature.raw == raw(dec(sig[1]))
    # the caller sends the deferred ones again: position 1 is still missing, position 4 is not
    again = [singles[k] for k in deferred]
    verified, deferred = pools.fold_verified_singles(agg, again)
    assert verified == [True, None] and deferred == []
    assert agg.bits[1] and agg.signature.raw == raw(O.g2_add(dec(sig[1]), dec(sig[2])))


def test_nothing_to_send_is_no_call(engine):
    agg = pools.Aggregate(4, bls.Signature(bytes(192)), [True] * 4)
    assert pools.fold_verified_singles(agg, [(2, MSG, SIG, 3)]) == ([None], [])
    assert pools.fold_verified_singles(agg, []) == ([], [])
    assert not [c for c in engine if c[0] in ("each_fold", "add")]


def test_a_count_that_disagrees_with_the_verdicts_is_an_error(engine, monkeypatch):
    def lying(msgs, sigs, base, cbits, fields, lists, groups):
        return [(0, 0, True)] * len(msgs), [(bls.Signature(bytes(192)), 0, bls.SignatureBytes(INF_BYTES))]
    monkeypatch.setattr(bls.Signature, "verify_each_fold", staticmethod(lying))
    agg = pools.Aggregate(4, bls.Signature(bytes(192)))
    with pytest.raises(RuntimeError):
        pools.fold_verified_singles(agg, [(2, MSG, SIG, 3)])
    assert agg.bits == [False] * 4


def test_multiverifier_sends_compact_forms_only(engine):
    mv = V.MultiVerifier()
    M.block(mv)                                       # qualifies for "spans"
    n = len(mv.triples)
    oks, folds = mv.verify_each_fold([[0, 3], [], [3, 3]])
    assert oks == [True] * n and mv.last_each_path == "fold" and len(folds) == 3
    assert mv.last_each_status == [(0, 0)] * n
    call = [c for c in engine if c[0] == "each_fold"][-1]
    assert call[7] == [[0, 3], [], [3, 3]] and call[3] == [None, 0, 1, None]
    assert folds[1][1] == 0 and folds[1][2] == INF_BYTES and folds[2][1] == 2
    # the same sets as verify_each sends, argument for argument
    del engine[:]
    assert mv.verify_each() == [True] * n and mv.last_each_path == "spans"
    assert engine[-1][0] == "each_spans" and [list(v) for v in engine[-1][6]] == call[6] and list(engine[-1][3]) == call[3]
    # no groups: the each-call's outputs, and the path says so
    oks, folds = mv.verify_each_fold([])
    assert oks == [True] * n and folds == [] and mv.last_each_path == "spans"
    # registry indices alone (singular attestations, sync-committee messages): plain sets
    mv = V.MultiVerifier()
    mv.verify_aggregate_indexed(MSG, SIG, [7], M.keys([7]), None)
    mv.verify_aggregate_indexed(MSG, SIG, [9], M.keys([9]), None)
    mv.verify_each_fold([[1, 0]])
    call = [c for c in engine if c[0] == "each_fold"][-1]
    assert call[3] == [None, None] and call[4] == [bytes(8)] * 2 and call[5] == [b"", b""] and call[6] == [[7], [9]]
    assert mv.last_each_path == "fold"
    # key points, or an index past the mirrored registry: no fold is built for them
    mv = V.MultiVerifier()
    mv.verify_aggregate(MSG, SIG, M.keys([3]), None)
    with pytest.raises(ValueError):
        mv.verify_each_fold([[0]])
    mv = V.MultiVerifier()
    mv.verify_aggregate_indexed(MSG, SIG, [200], M.keys([200]), None)
    with pytest.raises(ValueError):
        mv.verify_each_fold([[0]])
    assert V.MultiVerifier().verify_each_fold([[], []])[1][0][1] == 0


def test_signature_entry_marshals_the_groups(monkeypatch):
    seen = {}

    class Lib:
        def gbls_verify_each_fold(self, msgs, sigs, com, masks, bits, boff, idx, off, n, fset, foff, nfold, st, kst, v,
                                  out, fb, cnt):
            offs = [foff[g] for g in range(nfold + 1)]
            seen["call"] = (n, nfold, offs, [fset[k] for k in range(offs[-1])], [com[i] for i in range(n)])
            for i in range(n):
                st[i], kst[i], v[i] = 0, 0, (5 if i == 1 else 0)
            for g in range(nfold):
                out[192 * g] = bytes([g + 1])
                fb[96 * g] = bytes([0xC0 if g == 1 else 0x80 + g])
                cnt[g] = 7 * g
            return 0

    monkeypatch.setattr(G, "lib", lambda *a, **k: Lib())
    args = ([MSG] * 3, [SIG] * 3, [None, 4, None], [bytes(8), bytes([1]) + bytes(7), bytes(8)], [b"", b"\x03", b""],
            [[1], [], [7, 8]])
    sets, folds = bls.Signature.verify_each_fold(*args, [[2, 0, 2], [], [1]])
    assert seen["call"] == (3, 3, [0, 3, 3, 4], [2, 0, 2, 1], [G.NO_COMMITTEE, 4, G.NO_COMMITTEE])
    assert sets == [(0, 0, True), (0, 0, False), (0, 0, True)]
    assert [f[1] for f in folds] == [0, 7, 14] and [f[0].raw[0] for f in folds] == [1, 2, 3]
    assert all(len(f[0].raw) == 192 and len(f[2]) == 96 for f in folds) and folds[1][2][0] == 0xC0
    with pytest.raises(ValueError):
        bls.Signature.verify_each_fold(*args, [[3]])          # a group names a set of this call
    assert bls.Signature.verify_each_fold([], [], [], [], [], [], []) == ([], [])
