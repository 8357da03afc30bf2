"""Python mirror of ``helper_functions::verifier`` (/root/reference/helper_functions/src/verifier.rs).

The pluggable batching layer in front of the signature hot path:

* ``Verifier``        -- trait, verifier.rs:16-69 (``IS_NULL``, reserve, verify_singular,
                         verify_aggregate, verify_aggregate_allowing_empty, extend, finish,
                         has_option)
* ``NullVerifier``    -- verifier.rs:121-169 (skips cryptography)
* ``SingleVerifier``  -- verifier.rs:171-244 (verifies each triple immediately)
* ``MultiVerifier``   -- verifier.rs:246-347 (collects triples; ``finish`` runs one
                         random-linear-combination batch on the MI355X engine)
* ``Triple``          -- verifier.rs:349-429 (``verify_aggregate`` DEFERS the key sum: the key
                         list is summed on the device by the submission that verifies it)
* ``VerifierOption``  -- verifier.rs:431-436

Errors follow helper_functions/src/error.rs: ``SignatureInvalid(kind)``; decompression
failures surface as ``bls.DecompressionFailed``.
"""

from __future__ import annotations

import enum
from typing import Iterable, List, Optional

from . import bls


class SignatureKind(enum.Enum):  # helper_functions/src/error.rs:40-74 (subset used here)
    AggregateAndProof = "aggregate and proof"
    Attestation = "attestation"
    Block = "block"
    BlsToExecutionChange = "BLS to execution change"
    ContributionAndProof = "contribution and proof"
    Deposit = "deposit"
    Multi = "multiple signatures"
    Randao = "RANDAO reveal"
    SelectionProof = "selection proof"
    SyncCommitteeMessage = "sync committee message"
    SyncCommitteeContribution = "sync committee contribution"
    VoluntaryExit = "voluntary exit"


class SignatureInvalid(Exception):
    def __init__(self, kind: SignatureKind):
        super().__init__(f"{kind.value} signature is invalid")
        self.kind = kind


class VerifierOption(enum.Enum):
    SkipBlockBaseSignatures = 0
    SkipBlockSyncAggregateSignature = 1
    SkipRandaoVerification = 2
    BlockImport = 3  # the drop-in's one new option: the engine's block-import class (f3)


# MultiVerifier.finish names a committee slot when the absentee list is shorter than this multiple
# of the participant list (1: whichever list is shorter; tools/bench_committees.py measures where
# the absentee form stops winning)
ABSENTEE_FORM_MAX_RATIO = 1
G_LOCAL_KEYS = 0xFFFFFFFE  # GBLS_LOCAL_KEYS (grandine_amd/_lib.LOCAL_KEYS): the base slot of a local key set


class Triple:
    """(message: H256, signature_bytes: SignatureBytes, public_key: PublicKey), or, after
    ``verify_aggregate``, the message, signature and the KEY LIST whose sum is the key."""

    IS_NULL = False
    __slots__ = ("message", "signature_bytes", "_key", "deferred", "indices", "slot", "committee", "absent", "bits",
                 "span_base", "span_cbits", "span_committees", "key_bytes")

    def __init__(self, message: bytes = bytes(32), signature_bytes: bytes = None,
                 public_key: "bls.PublicKey" = None):
        self.message = bytes(message)
        self.signature_bytes = bls.SignatureBytes(signature_bytes if signature_bytes is not None else bytes(96))
        self._key = public_key if public_key is not None else bls.PublicKey.default()
        self.deferred = None  # list of keys once verify_aggregate has run
        self.indices = None   # their validator indices (verify_aggregate_indexed, f1)
        self.slot = None      # the committee table slot (verify_aggregate_committee), with
        self.committee = None  # ... the committee's member indices
        self.absent = None    # ... and the members whose aggregation bit is clear
        self.bits = None      # ... and the aggregation bits as SSZ bytes
        self.span_base = None  # verify_aggregate_committees: the base slot, with
        self.span_cbits = None  # ... committee_bits as its 8 SSZ bytes (bits then spans the named committees)
        self.span_committees = None  # ... and the named committees' member indices, ascending
        self.key_bytes = None  # verify_singular_bytes: the key as its 48 compressed bytes, not decoded on the host

    def verify_singular_bytes(self, message, signature_bytes, pubkey_bytes, signature_kind=None):
        """verify_singular for a key the caller holds only as 48 compressed bytes, with no registry
        entry (a deposit's pubkey, a BLS-to-execution change's from_bls_pubkey, a validator above
        the mirrored registry length): the bytes are KEPT and no host decode is performed.
        MultiVerifier sends them as a local key set (bls.Signature.verify_items_local), decoded on
        the device inside the submission that verifies the triple; on every other path the key is
        decoded through the engine when it is first asked for (public_key, keys)."""
        pubkey_bytes = bytes(pubkey_bytes)
        if len(pubkey_bytes) != 48:
            raise ValueError("a compressed public key is 48 bytes")
        self.message = bytes(message)
        self.signature_bytes = bls.SignatureBytes(bytes(signature_bytes))
        self._key = None
        self.deferred = self.indices = None
        self.slot = self.committee = self.absent = self.bits = None
        self.span_base = self.span_cbits = self.span_committees = None
        self.key_bytes = pubkey_bytes

    def _resolved(self):
        if self._key is None:  # kept bytes: one engine decode (PublicKey::try_from), raises as it does
            self._key = bls.PublicKey.try_from(self.key_bytes)
        return self._key

    def verify_aggregate(self, message, signature_bytes, public_keys, signature_kind=None):
        """verifier.rs:387-405 without the reduce: the keys are kept and summed on the device by
        the submission that verifies this triple (MultiVerifier.finish /
        SingleVerifier.extend)."""
        self.message = bytes(message)
        self.signature_bytes = bls.SignatureBytes(bytes(signature_bytes))
        self._key = bls.PublicKey.default()
        self.deferred = list(public_keys)
        # a reused triple keeps nothing of its previous set (rust/bls_patch/verifier.rs resets
        # its indices the same way)
        self.indices = None
        self.slot = self.committee = self.absent = self.bits = None
        self.span_base = self.span_cbits = self.span_committees = None
        self.key_bytes = None

    def verify_aggregate_indexed(self, message, signature_bytes, validator_indices, public_keys,
                                 signature_kind=None):
        """f1 (r06): verify_aggregate that also keeps the keys' validator indices
        (rust/bls_patch/verifier.rs), so MultiVerifier.finish can name registry slots."""
        self.verify_aggregate(message, signature_bytes, public_keys, signature_kind)
        self.indices = [int(i) for i in validator_indices]

    def verify_aggregate_committee(self, message, signature_bytes, slot, committee, aggregation_bits,
                                   public_keys, signature_kind=None):
        """verify_aggregate_indexed for an attestation of a whole committee: ``committee`` (its
        validator indices, helper_functions/src/accessors.rs:510-531) lives in committee table
        slot ``slot`` (bls.Committees), ``aggregation_bits`` selects the participants and
        ``public_keys`` are the participants' keys.  Keeps the participants' indices, as
        verify_aggregate_indexed does, plus the slot, the committee and the absentees, so that
        MultiVerifier.finish can send whichever list is shorter, and the bits themselves for a slot
        whose members are resident: ``bytes`` are taken as the SSZ encoding (a Bitlist with its
        delimiter or a Bitvector) and passed through, a sequence of bools is packed as a
        Bitvector."""
        committee = [int(i) for i in committee]
        if isinstance(aggregation_bits, (bytes, bytearray)):
            raw = bytes(aggregation_bits)
            if len(raw) < (len(committee) + 7) // 8:
                raise ValueError("one aggregation bit per committee member")
            bits = [bool(raw[j >> 3] >> (j & 7) & 1) for j in range(len(committee))]
        else:
            bits = [bool(b) for b in aggregation_bits]
            if len(bits) != len(committee):
                raise ValueError("one aggregation bit per committee member")
            packed = bytearray((len(bits) + 7) // 8)
            for j, b in enumerate(bits):
                packed[j >> 3] |= int(b) << (j & 7)
            raw = bytes(packed)
        self.verify_aggregate_indexed(message, signature_bytes, [v for v, b in zip(committee, bits) if b],
                                      public_keys, signature_kind)
        self.slot = int(slot)
        self.committee = committee
        self.absent = [v for v, b in zip(committee, bits) if not b]
        self.bits = raw

    def verify_aggregate_committees(self, message, signature_bytes, base_slot, committee_bits, committees,
                                    aggregation_bits, public_keys, signature_kind=None):
        """verify_aggregate_indexed for an attestation over several committees (EIP-7549):
        ``committee_bits`` (8 SSZ bytes, or an iterable of committee indices below 64) names the
        committees, which live in table slots ``base_slot + c``; ``committees`` are the named
        committees' member lists in ascending committee order; ``aggregation_bits`` is the ONE bit
        string over their concatenation (SSZ ``bytes`` passed through, or bools packed as a
        Bitvector); ``public_keys`` are the participants' keys.  Keeps the participants' indices,
        so that every existing path still takes the triple, plus the base slot, the mask and the
        bits for MultiVerifier.finish's "spans" path."""
        if isinstance(committee_bits, (bytes, bytearray)):
            cbits = bytes(committee_bits)
            if len(cbits) != 8:
                raise ValueError("committee_bits is a Bitvector[64]: 8 bytes")
        else:
            packed = bytearray(8)
            for c in committee_bits:
                if not 0 <= int(c) < 64:
                    raise ValueError("a committee index is below 64")
                packed[int(c) >> 3] |= 1 << (int(c) & 7)
            cbits = bytes(packed)
        committees = [[int(i) for i in c] for c in committees]
        if len(committees) != sum(bin(b).count("1") for b in cbits):
            raise ValueError("one member list per named committee")
        flat = [v for c in committees for v in c]
        if isinstance(aggregation_bits, (bytes, bytearray)):
            raw = bytes(aggregation_bits)
            if len(raw) < (len(flat) + 7) // 8:
                raise ValueError("one aggregation bit per member of the named committees")
            bits = [bool(raw[j >> 3] >> (j & 7) & 1) for j in range(len(flat))]
        else:
            bits = [bool(b) for b in aggregation_bits]
            if len(bits) != len(flat):
                raise ValueError("one aggregation bit per member of the named committees")
            packed = bytearray((len(bits) + 7) // 8)
            for j, b in enumerate(bits):
                packed[j >> 3] |= int(b) << (j & 7)
            raw = bytes(packed)
        self.verify_aggregate_indexed(message, signature_bytes, [v for v, b in zip(flat, bits) if b], public_keys,
                                      signature_kind)
        self.span_base = int(base_slot)
        self.span_cbits = cbits
        self.span_committees = committees
        self.bits = raw

    def span_slots(self):
        """The table slots a verify_aggregate_committees triple names, ascending."""
        return [self.span_base + c for c in range(64) if self.span_cbits[c >> 3] >> (c & 7) & 1]

    @property
    def public_key(self) -> "bls.PublicKey":
        """The set's key: the reference's reduce(AggregatePublicKey::default, aggregate) over a
        deferred list (one engine sum), or the resolved key."""
        if self.deferred is None:
            return self._resolved()
        if not self.deferred:
            return bls.PublicKey.default()  # identity of the reduce
        return bls.PublicKey.aggregate_nonempty(self.deferred)

    def keys(self):
        """The engine's key operand: the deferred list, or [the key]."""
        return list(self.deferred) if self.deferred is not None else [self._resolved()]


class Verifier:
    IS_NULL = False

    def reserve(self, additional: int) -> None:
        pass

    def verify_singular(self, message, signature_bytes, cached_public_key, signature_kind):
        raise NotImplementedError

    def verify_aggregate(self, message, signature_bytes, public_keys, signature_kind):
        raise NotImplementedError

    def verify_aggregate_allowing_empty(self, message, signature_bytes, public_keys, signature_kind):
        """verifier.rs:41-58 (eth_fast_aggregate_verify's emptiness rule)."""
        keys = list(public_keys)
        if bls.SignatureBytes(bytes(signature_bytes)).is_empty():
            if keys:
                raise SignatureInvalid(signature_kind)
            return None
        return self.verify_aggregate(message, signature_bytes, keys, signature_kind)

    def extend(self, triples: Iterable[Triple], signature_kind):
        raise NotImplementedError

    def finish(self) -> None:
        raise NotImplementedError

    def has_option(self, option: VerifierOption) -> bool:
        return False


class NullVerifier(Verifier):
    IS_NULL = True

    def verify_singular(self, message, signature_bytes, cached_public_key, signature_kind):
        return None

    def verify_aggregate(self, message, signature_bytes, public_keys, signature_kind):
        return None

    def extend(self, triples, signature_kind):
        return None

    def finish(self):
        return None


class SingleVerifier(Verifier):
    def verify_singular(self, message, signature_bytes, cached_public_key, signature_kind):
        public_key = cached_public_key.decompress()
        self.extend([Triple(message, signature_bytes, public_key)], signature_kind)

    def verify_aggregate(self, message, signature_bytes, public_keys, signature_kind):
        """verifier.rs:193-212: Signature::fast_aggregate_verify."""
        signature = bls.Signature.try_from(signature_bytes)
        if not signature.fast_aggregate_verify(message, list(public_keys)):
            raise SignatureInvalid(signature_kind)

    def extend(self, triples, signature_kind):
        """verifier.rs:215-236 as ONE coalesced device submission: every triple's decompression
        and check together, errors in the reference's order (the first triple whose signature
        does not decode -> DecompressionFailed, the first that does not verify ->
        SignatureInvalid)."""
        triples = list(triples)
        if not triples:
            return None
        outcomes = bls.Signature.verify_batch_compressed(
            [t.message for t in triples], [t.signature_bytes for t in triples], [t.keys() for t in triples])
        for status, ok in outcomes:
            if status != 0:
                raise bls.DecompressionFailed(status)
            if not ok:
                raise SignatureInvalid(signature_kind)
        return None

    def finish(self):
        return None


class MultiVerifier(Verifier):
    def __init__(self, options: Iterable[VerifierOption] = (), triples: Optional[List[Triple]] = None):
        self.triples: List[Triple] = list(triples or [])
        self.options = set(options)
        # "local", "spans", "bits", "committees", "indices" or "points": the key form of the last finish (tests)
        self.last_path = None
        # "local", "spans" or "points": the key form of the last verify_each / verify_items; "fold": verify_each_fold
        # with groups
        self.last_each_path = None
        self.last_each_status = None  # verify_each on "spans": per set (signature status, key status)

    @classmethod
    def from_triples(cls, triples: List[Triple]) -> "MultiVerifier":  # From<Vec<Triple>>
        return cls(triples=triples)

    def verify_singular(self, message, signature_bytes, cached_public_key, signature_kind):
        public_key = cached_public_key.decompress()
        self.triples.append(Triple(message, signature_bytes, public_key))

    def verify_singular_bytes(self, message, signature_bytes, pubkey_bytes, signature_kind=None):
        t = Triple()
        t.verify_singular_bytes(message, signature_bytes, pubkey_bytes, signature_kind)
        self.triples.append(t)

    def verify_aggregate(self, message, signature_bytes, public_keys, signature_kind):
        t = Triple()
        t.verify_aggregate(message, signature_bytes, public_keys, signature_kind)
        self.triples.append(t)

    def extend(self, triples, signature_kind):
        self.triples.extend(triples)

    def verify_aggregate_indexed(self, message, signature_bytes, validator_indices, public_keys, signature_kind):
        t = Triple()
        t.verify_aggregate_indexed(message, signature_bytes, validator_indices, public_keys, signature_kind)
        self.triples.append(t)

    def verify_aggregate_committee(self, message, signature_bytes, slot, committee, aggregation_bits, public_keys,
                                   signature_kind):
        t = Triple()
        t.verify_aggregate_committee(message, signature_bytes, slot, committee, aggregation_bits, public_keys,
                                     signature_kind)
        self.triples.append(t)

    def verify_aggregate_committees(self, message, signature_bytes, base_slot, committee_bits, committees,
                                    aggregation_bits, public_keys, signature_kind=None):
        t = Triple()
        t.verify_aggregate_committees(message, signature_bytes, base_slot, committee_bits, committees,
                                      aggregation_bits, public_keys, signature_kind)
        self.triples.append(t)

    def _span_sets(self):
        """The triples as span sets (base slots, masks, bit strings, index lists), or None when they
        do not qualify: at least one triple came through verify_aggregate_committees, every slot it
        names keeps exactly the members the triple was built from, and the other triples qualify as
        for "bits" (a single-committee triple is then a span with one bit)."""
        if any(t.key_bytes is not None for t in self.triples):
            return None  # (kept key bytes: _local_sets)
        spans = [t for t in self.triples if t.span_base is not None]
        if not spans:
            return None
        for t in spans:
            slots = t.span_slots()
            if not slots or not all(bls.Committees.has_members(s) and bls.Committees.covers(s, c)
                                    for s, c in zip(slots, t.span_committees)):
                return None
        for t in self.triples:
            if t.span_base is not None:
                continue
            if t.slot is not None:
                if not (bls.Committees.has_members(t.slot) and bls.Committees.covers(t.slot, t.committee)):
                    return None
            elif t.indices is None or not bls.Registry.covers(t.indices):
                return None
        one = bytes([1]) + bytes(7)
        base, cbits, fields, lists = [], [], [], []
        for t in self.triples:
            if t.span_base is not None:
                base.append(t.span_base), cbits.append(t.span_cbits), fields.append(t.bits), lists.append(())
            elif t.slot is not None:
                base.append(t.slot), cbits.append(one), fields.append(t.bits), lists.append(())
            else:
                base.append(None), cbits.append(bytes(8)), fields.append(b""), lists.append(t.indices)
        return base, cbits, fields, lists

    def _local_sets(self):
        """The triples as span, plain and LOCAL sets plus the call's key table, or None: at least one
        triple keeps its key bytes (verify_singular_bytes) and the others qualify for "spans".  A
        key that several triples name is in the table once."""
        local = [t for t in self.triples if t.key_bytes is not None]
        if not local:
            return None
        rest = MultiVerifier(triples=[t for t in self.triples if t.key_bytes is None])._span_sets()
        if rest is None:
            return None
        table, at = [], {}
        rest = iter(zip(*rest))
        base, cbits, fields, lists = [], [], [], []
        for t in self.triples:
            if t.key_bytes is None:
                b, c, f, l = next(rest)
            else:
                if t.key_bytes not in at:
                    at[t.key_bytes] = len(table)
                    table.append(t.key_bytes)
                b, c, f, l = G_LOCAL_KEYS, bytes(8), b"", [at[t.key_bytes]]
            base.append(b), cbits.append(c), fields.append(f), lists.append(l)
        return base, cbits, fields, lists, table

    def _finish_local(self, msgs, sigs, randoms, flags):
        """The "local" path, or None when the triples do not qualify (_local_sets): the batch as ONE
        item of verify_items_local.  Returns as multi_verify_compressed: a signature's or a local
        key's decoding error comes first."""
        sets = self._local_sets()
        if sets is None:
            return None
        self.last_path = "local"
        verdicts, statuses, key_statuses = bls.Signature.verify_items_local(
            msgs, sigs, *sets, [0, len(msgs)], randoms, flags, with_statuses=True)
        for st, _ in statuses:
            if st != 0:
                return st
        for st in key_statuses:
            if st != 0:
                return st
        return 0 if verdicts[0] else 5

    def _finish_spans(self, msgs, sigs, randoms, flags):
        """The "spans" path, or None when the triples do not qualify (_span_sets)."""
        sets = self._span_sets()
        if sets is None:
            return None
        self.last_path = "spans"
        return bls.Signature.multi_verify_compressed_spans(msgs, sigs, *sets, randoms, flags)

    def finish(self, randoms=None):
        """verifier.rs:301-323."""
        if not self.triples:
            return None
        # decompression (verifier.rs:309-313) and multi_verify in one device submission
        # key sums of deferred triples (Triple.verify_aggregate) on the device, same submission;
        # f1: registry indices instead of key points when every set has them and the engine's
        # registry mirrors those validators (bls.Registry)
        flags = 0x1 if VerifierOption.BlockImport in self.options else 0
        msgs = [t.message for t in self.triples]
        sigs = [t.signature_bytes for t in self.triples]
        indexed = all(t.indices is not None and bls.Registry.covers(t.indices) for t in self.triples)
        com = [t for t in self.triples if t.slot is not None]
        # attestations over several committees first: base slot, committee_bits and the one bit string
        rc = self._finish_local(msgs, sigs, randoms, flags)
        if rc is None:
            rc = self._finish_spans(msgs, sigs, randoms, flags)
        if rc is not None:
            pass  # sent: last_path == "local" or "spans"
        elif com and all(bls.Committees.has_members(t.slot) and bls.Committees.covers(t.slot, t.committee)
                       for t in com) and all(t.indices is not None and bls.Registry.covers(t.indices)
                                             for t in self.triples if t.slot is None):
            # resident members: a committee triple is its slot and its aggregation bits as they
            # arrived (the engine checks them against the committee and picks the direction), the
            # other triples their registry indices
            self.last_path = "bits"
            rc = bls.Signature.multi_verify_compressed_bits(
                msgs, sigs, [t.slot for t in self.triples], [t.bits if t.slot is not None else b"" for t in self.triples],
                [() if t.slot is not None else t.indices for t in self.triples], randoms, flags)
        elif indexed and com and all(bls.Committees.covers(t.slot, t.committee) and bls.Registry.covers(t.absent)
                                   for t in com):
            # cached committee sums: per committee triple the absentees (key = slot - their sum)
            # or, when they are the longer list, the participants without a slot
            self.last_path = "committees"
            slots, lists = [], []
            for t in self.triples:
                by_absence = t.slot is not None and len(t.absent) < ABSENTEE_FORM_MAX_RATIO * len(t.indices)
                slots.append(t.slot if by_absence else None)
                lists.append(t.absent if by_absence else t.indices)
            rc = bls.Signature.multi_verify_compressed_committees(msgs, sigs, slots, lists, randoms, flags)
        elif indexed:
            self.last_path = "indices"
            rc = bls.Signature.multi_verify_compressed_indexed(msgs, sigs, [t.indices for t in self.triples],
                                                               randoms, flags)
        else:
            self.last_path = "points"
            rc = bls.Signature.multi_verify_compressed(msgs, sigs, [t.keys() for t in self.triples], randoms, flags)
        if rc not in (0, 5):
            raise bls.DecompressionFailed(rc)
        if rc != 0:
            raise SignatureInvalid(SignatureKind.Multi)
        return None

    def verify_each(self) -> List[bool]:
        """f2 (r06, a new method of the drop-in's MultiVerifier): which collected sets verify ON
        THEIR OWN, in ONE device submission (gbls_verify_batch_compressed: every set its own
        check with Signature::verify / fast_aggregate_verify semantics -- the verdict the
        singular path would reach).  A set whose signature does not decode is False.  For a
        caller whose batch failed, so that only the failing items take the singular path
        (split_failed_batch).  Triples that qualify for finish's "spans" path stay in that compact
        form (gbls_verify_each_spans: no key points uploaded, the cached sums reused; a set whose
        key the engine rejects is False); last_each_status then keeps every set's (signature
        status, key status)."""
        if not self.triples:
            return []
        sets = self._local_sets()
        if sets is not None:  # kept key bytes among triples that qualify for "spans": decoded on the device
            self.last_each_path = "local"
            outcomes, _ = bls.Signature.verify_each_local(
                [t.message for t in self.triples], [t.signature_bytes for t in self.triples], *sets)
            self.last_each_status = [(st, kst) for st, kst, _ in outcomes]
            return [st == 0 and kst == 0 and ok for st, kst, ok in outcomes]
        sets = self._span_sets()
        if sets is not None:
            self.last_each_path = "spans"
            outcomes = bls.Signature.verify_each_spans(
                [t.message for t in self.triples], [t.signature_bytes for t in self.triples], *sets)
            self.last_each_status = [(st, kst) for st, kst, _ in outcomes]
            return [st == 0 and kst == 0 and ok for st, kst, ok in outcomes]
        self.last_each_path = "points"
        self.last_each_status = None
        outcomes = bls.Signature.verify_batch_compressed(
            [t.message for t in self.triples], [t.signature_bytes for t in self.triples],
            [t.keys() for t in self.triples])
        return [status == 0 and ok for status, ok in outcomes]

    def _fold_sets(self):
        """The triples as the sets of the fold call: finish's "spans" form, or -- singular
        attestations and sync-committee messages, no committee named at all -- every triple the plain
        list of its registry indices.  None when they do not qualify."""
        sets = self._span_sets()
        if sets is not None:
            return sets
        if any(t.key_bytes is not None or t.span_base is not None or t.slot is not None or t.indices is None
               or not bls.Registry.covers(t.indices) for t in self.triples):
            return None
        n = len(self.triples)
        return [None] * n, [bytes(8)] * n, [b""] * n, [t.indices for t in self.triples]

    def verify_each_fold(self, groups: Iterable[Sequence[int]]):
        """verify_each which also aggregates what passed (gbls_verify_each_fold): ``groups[g]`` lists
        triples of this verifier, and the signatures of those that verify on their own are summed on
        the device, behind the verdicts, in the same submission -- the aggregate_in_place loop of
        aggregate_attestation (operation_pools/src/attestation_agg_pool/tasks.rs:242-257) without
        decoding a signature a second time.  Returns (one bool per triple, per group (Signature,
        count, SignatureBytes)); count == 0: nothing of the group passed, the sum is infinity.
        Only for triples in the compact forms (finish's "spans" path, or registry indices alone): a
        fold over key points is not built, and asking for one is an error."""
        grp = [list(g) for g in groups]
        if not self.triples:
            if any(grp):
                raise ValueError("a group names triples of this verifier")
            empty = (bls.Signature(), 0, bls.SignatureBytes.empty())
            return [], [empty for _ in grp]
        sets = self._fold_sets()
        if sets is None:
            raise ValueError("verify_each_fold needs triples in the spans form or over registry indices")
        self.last_each_path = "fold" if grp else "spans"
        outcomes, folds = bls.Signature.verify_each_fold(
            [t.message for t in self.triples], [t.signature_bytes for t in self.triples], *sets, grp)
        self.last_each_status = [(st, kst) for st, kst, _ in outcomes]
        return [st == 0 and kst == 0 and ok for st, kst, ok in outcomes], folds

    def verify_items(self, item_of_triple: Iterable[int], randoms=None) -> List[bool]:
        """Which ITEMS verify, in ONE device submission (gbls_verify_items_spans): triple k belongs
        to item item_of_triple[k] (nondecreasing, items numbered from 0; an item without a triple
        is False), and each item is its own random-linear-combination batch -- a gossip aggregate
        as its three sets, or the blocks of the block verification pool.  For triples that qualify
        for finish's "spans" path; others are decided set by set over key points (verify_each),
        an item passing when all of its sets do."""
        owner = [int(k) for k in item_of_triple]
        if len(owner) != len(self.triples) or any(a > b for a, b in zip(owner, owner[1:])) or (owner and owner[0] < 0):
            raise ValueError("one nondecreasing item number per triple")
        nitems = owner[-1] + 1 if owner else 0
        offsets = [sum(1 for k in owner if k < s) for s in range(nitems + 1)]
        if not self.triples:
            return []
        flags = 0x1 if VerifierOption.BlockImport in self.options else 0
        sets = self._local_sets()
        if sets is not None:
            self.last_each_path = "local"
            return bls.Signature.verify_items_local(
                [t.message for t in self.triples], [t.signature_bytes for t in self.triples], *sets, offsets, randoms,
                flags)
        sets = self._span_sets()
        if sets is None:
            each = self.verify_each()  # last_each_path == "points"
            return [offsets[s] < offsets[s + 1] and all(each[offsets[s]:offsets[s + 1]]) for s in range(nitems)]
        self.last_each_path = "spans"
        return bls.Signature.verify_items_spans(
            [t.message for t in self.triples], [t.signature_bytes for t in self.triples], *sets, offsets, randoms, flags)

    def has_option(self, option: VerifierOption) -> bool:
        return option in self.options


def split_failed_batch(items: List, item_triples: List[Optional[List[Triple]]]):
    """The drop-in's fallback after a failed gossip batch (rust/bls_patch/attestation_verifier.rs,
    replacing /root/reference/p2p/src/attestation_verifier.rs:231-238 and 379-384, where every
    item of the failed batch is re-verified one by one on the CPU).

    item_triples[k]: the signature sets of item k IN ORDER (an attestation has one; an aggregate
    three: selection proof, aggregate-and-proof signature, attestation), or None when they cannot
    be built (the singular path then reports why).  One submission (MultiVerifier.verify_each)
    decides every set; returns (passed, failing): the items whose sets all verify keep their batch
    results, only the failing ones go to the singular path."""
    if len(items) != len(item_triples):
        raise ValueError("one triple list per item")
    owner, triples = [], []
    for k, ts in enumerate(item_triples):
        for t in ts or []:
            owner.append(k)
            triples.append(t)
    verified = MultiVerifier(triples=triples).verify_each()
    bad = [ts is None for ts in item_triples]
    for k, ok in zip(owner, verified):
        if not ok:
            bad[k] = True
    passed = [it for it, b in zip(items, bad) if not b]
    failing = [it for it, b in zip(items, bad) if b]
    return passed, failing
