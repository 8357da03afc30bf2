"""Python mirror of the reference ``bls`` crate (/root/reference/bls/src), backed by the
MI355X engine through the C ABI (include/grandine_bls_gpu.h).

Names, argument meaning and error behaviour follow the crate:

* ``PublicKey``  -- bls/src/public_key.rs (try_from validates; aggregate / aggregate_nonempty)
* ``Signature``  -- bls/src/signature.rs (verify, fast_aggregate_verify, multi_verify, aggregate)
* ``SecretKey``  -- bls/src/secret_key.rs (try_from, to_public_key, sign)
* ``CachedPublicKey`` -- bls/src/cached_public_key.rs (decompress once, cache)
* ``Error.DecompressionFailed(BLST_ERROR)`` / ``Error.NoPublicKeysToAggregate`` -- bls/src/error.rs

Points are held as the engine's 96/192-byte affine encodings (blst_p1_affine /
blst_p2_affine layout, Montgomery limbs, all-zero = infinity).
"""

from __future__ import annotations

import ctypes
import secrets
from typing import Iterable, List, Sequence

from . import _lib as G

DOMAIN_SEPARATION_TAG = b"BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_"  # bls/src/consts.rs:1
CURVE_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


class Error(Exception):
    """bls::Error (bls/src/error.rs:7-14)."""


class DecompressionFailed(Error):
    def __init__(self, code: int):
        super().__init__(f"decompression failed: {code}")
        self.code = code


class NoPublicKeysToAggregate(Error):
    def __init__(self):
        super().__init__("no public keys to aggregate")


Error.DecompressionFailed = DecompressionFailed
Error.NoPublicKeysToAggregate = NoPublicKeysToAggregate


# ----------------------------------------------------------------------------- bytes types
class PublicKeyBytes(bytes):
    SIZE = 48

    def __new__(cls, data: bytes = bytes(48)):
        if len(data) != 48:
            raise ValueError("PublicKeyBytes must be 48 bytes")
        return super().__new__(cls, data)


class SignatureBytes(bytes):
    SIZE = 96

    def __new__(cls, data: bytes = bytes(96)):
        if len(data) != 96:
            raise ValueError("SignatureBytes must be 96 bytes")
        return super().__new__(cls, data)

    @classmethod
    def empty(cls) -> "SignatureBytes":
        """bls/src/signature_bytes.rs:46-56: 0xc0 followed by zeros."""
        return cls(b"\xc0" + bytes(95))

    def is_empty(self) -> bool:
        return self == SignatureBytes.empty()


class SecretKeyBytes(bytes):
    def __new__(cls, data: bytes):
        if len(data) != 32:
            raise ValueError("SecretKeyBytes must be 32 bytes")
        return super().__new__(cls, data)


# ----------------------------------------------------------------------------- engine policy
POLICY_NO_COALESCE = G.INIT_NO_COALESCE
POLICY_PER_CHECK = G.INIT_PER_CHECK
POLICY_DEDUP = G.INIT_DEDUP


def set_policy(flags: int) -> int:
    """gbls_set_policy: sets the engine's policy bits outright and returns the previous ones.
    `set_policy(POLICY_DEDUP)` makes every batch verification group its sets by message (one
    hash_to_G2 and one pairing per distinct message; verdicts unchanged)."""
    return int(G.load_library().gbls_set_policy(int(flags)))  # needs no device


# ----------------------------------------------------------------------------- batched helpers
def decompress_public_keys(items: Sequence[bytes], validate: bool = True):
    """Batched PublicKey::try_from: returns [(status, affine96 or None)]."""
    n = len(items)
    if n == 0:
        return []
    L = G.lib()
    inb = G.buf(b"".join(bytes(x) for x in items))
    out = ctypes.create_string_buffer(96 * n)
    st = G.i32_array(n)
    G.check(L.gbls_g1_decompress(inb, n, int(validate), out, st), "gbls_g1_decompress")
    raw = out.raw
    return [(st[i], raw[96 * i:96 * (i + 1)] if st[i] == G.SUCCESS else None) for i in range(n)]


def decompress_signatures(items: Sequence[bytes]):
    """Batched Signature::try_from (on-curve check only): [(status, affine192 or None)]."""
    n = len(items)
    if n == 0:
        return []
    L = G.lib()
    inb = G.buf(b"".join(bytes(x) for x in items))
    out = ctypes.create_string_buffer(192 * n)
    st = G.i32_array(n)
    G.check(L.gbls_g2_decompress(inb, n, out, st), "gbls_g2_decompress")
    raw = out.raw
    return [(st[i], raw[192 * i:192 * (i + 1)] if st[i] == G.SUCCESS else None) for i in range(n)]


# ----------------------------------------------------------------------------- PublicKey
class PublicKey:
    """bls::PublicKey (bls/src/public_key.rs)."""

    __slots__ = ("raw",)

    def __init__(self, raw: bytes = bytes(96)):
        self.raw = bytes(raw)

    @classmethod
    def default(cls) -> "PublicKey":  # blst default = all-zero = infinity
        return cls()

    @classmethod
    def try_from(cls, data: bytes) -> "PublicKey":
        """public_key.rs:16-31: uncompress, then validate (rejects infinity / non-G1)."""
        st, raw = decompress_public_keys([PublicKeyBytes(bytes(data))], validate=True)[0]
        if st != G.SUCCESS:
            raise DecompressionFailed(st)
        return cls(raw)

    def to_bytes(self) -> PublicKeyBytes:
        L = G.lib()
        out = ctypes.create_string_buffer(48)
        G.check(L.gbls_g1_compress(G.buf(self.raw), 1, out), "gbls_g1_compress")
        return PublicKeyBytes(out.raw)

    def is_infinity(self) -> bool:
        return not any(self.raw)

    def aggregate(self, other: "PublicKey") -> "PublicKey":
        return PublicKey.aggregate_nonempty([self, other])

    def aggregate_in_place(self, other: "PublicKey") -> None:
        self.raw = self.aggregate(other).raw

    @staticmethod
    def aggregate_nonempty(public_keys: Iterable["PublicKey"]) -> "PublicKey":
        """public_key.rs:34-40 (eth_aggregate_pubkeys)."""
        keys = list(public_keys)
        if not keys:
            raise NoPublicKeysToAggregate()
        L = G.lib()
        out = ctypes.create_string_buffer(96)
        rc = L.gbls_g1_aggregate(G.buf(b"".join(k.raw for k in keys)), len(keys), out)
        if rc != G.SUCCESS:
            raise G.EngineUnavailable(f"gbls_g1_aggregate rc={rc}")
        return PublicKey(out.raw)

    def __eq__(self, other):
        return isinstance(other, PublicKey) and self.raw == other.raw

    def __hash__(self):
        return hash(self.raw)


AggregatePublicKey = PublicKey


class CachedPublicKey:
    """bls::CachedPublicKey: bytes + a lazily decompressed key (cached_public_key.rs:11-108)."""

    def __init__(self, data: bytes, decompressed: PublicKey = None):
        self.bytes = PublicKeyBytes(bytes(data))
        self._pk = decompressed

    def decompress(self) -> PublicKey:
        if self._pk is None:
            self._pk = PublicKey.try_from(self.bytes)
        return self._pk


# ----------------------------------------------------------------------------- Signature
class Signature:
    """bls::Signature (bls/src/signature.rs)."""

    __slots__ = ("raw",)

    def __init__(self, raw: bytes = bytes(192)):
        self.raw = bytes(raw)

    @classmethod
    def default(cls) -> "Signature":  # signature.rs:20-27
        return cls.try_from(SignatureBytes.empty())

    @classmethod
    def try_from(cls, data: bytes) -> "Signature":
        st, raw = decompress_signatures([SignatureBytes(bytes(data))])[0]
        if st != G.SUCCESS:
            raise DecompressionFailed(st)
        return cls(raw)

    def to_bytes(self) -> SignatureBytes:
        L = G.lib()
        out = ctypes.create_string_buffer(96)
        G.check(L.gbls_g2_compress(G.buf(self.raw), 1, out), "gbls_g2_compress")
        return SignatureBytes(out.raw)

    def verify(self, message: bytes, public_key: PublicKey) -> bool:
        """signature.rs:47-60."""
        L = G.lib()
        m = bytes(message)
        return L.gbls_verify(G.buf(self.raw), G.buf(m), len(m), G.buf(public_key.raw)) == G.SUCCESS

    def aggregate(self, other: "Signature") -> "Signature":
        L = G.lib()
        out = ctypes.create_string_buffer(192)
        G.check(L.gbls_g2_aggregate(G.buf(self.raw + other.raw), 2, out), "gbls_g2_aggregate")
        return Signature(out.raw)

    def aggregate_in_place(self, other: "Signature") -> None:
        self.raw = self.aggregate(other).raw

    def fast_aggregate_verify(self, message: bytes, public_keys: Iterable[PublicKey]) -> bool:
        """signature.rs:77-93."""
        keys = list(public_keys)
        L = G.lib()
        m = bytes(message)
        return L.gbls_fast_aggregate_verify(G.buf(self.raw), G.buf(m), len(m),
                                            G.buf(b"".join(k.raw for k in keys)), len(keys)) == G.SUCCESS

    @staticmethod
    def multi_verify(messages: Iterable[bytes], signatures: Iterable["Signature"],
                     public_keys: Iterable[PublicKey], randoms: Sequence[int] = None) -> bool:
        """signature.rs:95-129: random nonzero 64-bit scalars (ThreadRng -> secrets)."""
        msgs = [bytes(m) for m in messages]
        sigs = list(signatures)
        pks = list(public_keys)
        n = len(sigs)
        if n == 0 or len(msgs) != n or len(pks) != n:
            return False
        if any(len(m) != 32 for m in msgs):
            # the engine's batch path takes 32-byte signing roots (H256), as MultiVerifier does
            raise ValueError("multi_verify messages must be 32-byte signing roots")
        if randoms is None:
            randoms = [secrets.randbits(64) or 1 for _ in range(n)]
        L = G.lib()
        return L.gbls_multi_verify(G.buf(b"".join(msgs)), G.buf(b"".join(s.raw for s in sigs)),
                                   G.buf(b"".join(p.raw for p in pks)), G.u64_array(randoms), n) == G.SUCCESS

    @staticmethod
    def multi_verify_compressed(messages: Iterable[bytes], signature_bytes: Iterable[bytes],
                                public_keys: Iterable, randoms: Sequence[int] = None,
                                call_flags: int = 0) -> int:
        """MultiVerifier::finish's decompress + multi_verify (verifier.rs:301-323) as one device
        submission (gbls_multi_verify_compressed_ex): 0 = valid, 5 = VERIFY_FAIL, otherwise the
        first signature's decompression status (finish's Err(DecompressionFailed)).  Each set's
        key is a PublicKey or a list of them, summed on the device inside the same submission
        (a deferred Triple::verify_aggregate, verifier.rs:387-405)."""
        msgs = [bytes(m) for m in messages]
        sigs = [bytes(s) for s in signature_bytes]
        keys = [list(k) if isinstance(k, (list, tuple)) else [k] for k in public_keys]
        n = len(sigs)
        if n == 0 or len(msgs) != n or len(keys) != n:
            return G.VERIFY_FAIL
        if any(len(m) != 32 for m in msgs) or any(len(s) != 96 for s in sigs):
            raise ValueError("messages must be 32-byte signing roots and signatures 96 bytes")
        if randoms is None:
            randoms = [secrets.randbits(64) or 1 for _ in range(n)]
        off = [0]
        for k in keys:
            off.append(off[-1] + len(k))
        L = G.lib()
        st = G.i32_array(n)
        return L.gbls_multi_verify_compressed_ex(
            G.buf(b"".join(msgs)), G.buf(b"".join(sigs)), G.buf(b"".join(p.raw for k in keys for p in k)),
            None, G.u32_array(off), G.u64_array(randoms), n, st, call_flags)

    @staticmethod
    def multi_verify_compressed_indexed(messages: Iterable[bytes], signature_bytes: Iterable[bytes],
                                        validator_indices: Iterable[Sequence[int]], randoms: Sequence[int] = None,
                                        call_flags: int = 0) -> int:
        """multi_verify_compressed with each set's keys named by REGISTRY INDICES (f1: the engine
        gathers and sums the registry's keys on the device; 4 bytes per key instead of 96).
        Returns as multi_verify_compressed; an index past the registry fails its set."""
        msgs = [bytes(m) for m in messages]
        sigs = [bytes(s) for s in signature_bytes]
        idx = [list(v) for v in validator_indices]
        n = len(sigs)
        if n == 0 or len(msgs) != n or len(idx) != n:
            return G.VERIFY_FAIL
        if any(len(m) != 32 for m in msgs) or any(len(s) != 96 for s in sigs):
            raise ValueError("messages must be 32-byte signing roots and signatures 96 bytes")
        if randoms is None:
            randoms = [secrets.randbits(64) or 1 for _ in range(n)]
        off = [0]
        for v in idx:
            off.append(off[-1] + len(v))
        flat = [i for v in idx for i in v]
        L = G.lib()
        st = G.i32_array(n)
        return L.gbls_multi_verify_compressed_ex(
            G.buf(b"".join(msgs)), G.buf(b"".join(sigs)), None, G.u32_array(flat or [0]), G.u32_array(off),
            G.u64_array(randoms), n, st, call_flags)

    @staticmethod
    def multi_verify_compressed_committees(messages: Iterable[bytes], signature_bytes: Iterable[bytes],
                                           committee_slots: Iterable[int],
                                           validator_indices: Iterable[Sequence[int]],
                                           randoms: Sequence[int] = None, call_flags: int = 0) -> int:
        """multi_verify_compressed_indexed over cached committee sums
        (gbls_multi_verify_committees): set i's key is committee slot ``committee_slots[i]`` MINUS
        the registry keys ``validator_indices[i]`` (its absent members), or, when the slot is
        ``None``, the plain sum of those keys.  Returns as multi_verify_compressed."""
        msgs = [bytes(m) for m in messages]
        sigs = [bytes(s) for s in signature_bytes]
        com = [G.NO_COMMITTEE if c is None else int(c) for c in committee_slots]
        idx = [list(v) for v in validator_indices]
        n = len(sigs)
        if n == 0 or len(msgs) != n or len(idx) != n or len(com) != n:
            return G.VERIFY_FAIL
        if any(len(m) != 32 for m in msgs) or any(len(s) != 96 for s in sigs):
            raise ValueError("messages must be 32-byte signing roots and signatures 96 bytes")
        if randoms is None:
            randoms = [secrets.randbits(64) or 1 for _ in range(n)]
        off = [0]
        for v in idx:
            off.append(off[-1] + len(v))
        flat = [i for v in idx for i in v]
        L = G.lib()
        st = G.i32_array(n)
        return L.gbls_multi_verify_committees(
            G.buf(b"".join(msgs)), G.buf(b"".join(sigs)), G.u32_array(com), G.u32_array(flat or [0]),
            G.u32_array(off), G.u64_array(randoms), n, st, call_flags)

    @staticmethod
    def multi_verify_compressed_bits(messages: Iterable[bytes], signature_bytes: Iterable[bytes],
                                     committee_slots: Iterable[int], bitfields: Iterable[bytes],
                                     validator_indices: Iterable[Sequence[int]],
                                     randoms: Sequence[int] = None, call_flags: int = 0) -> int:
        """multi_verify_compressed_committees with the sets given as they arrive
        (gbls_multi_verify_bits): set i names committee slot ``committee_slots[i]``, loaded with its
        members (Committees.set(..., members=True)), and carries its SSZ aggregation bits
        ``bitfields[i]`` (a Bitlist with its delimiter, or a Bitvector); its key is the sum of the
        members whose bit is set.  A set whose slot is ``None`` is the plain sum of the registry
        keys ``validator_indices[i]`` and has no bits.  Returns as multi_verify_compressed."""
        msgs = [bytes(m) for m in messages]
        sigs = [bytes(s) for s in signature_bytes]
        com = [G.NO_COMMITTEE if c is None else int(c) for c in committee_slots]
        fields = [bytes(b or b"") for b in bitfields]
        idx = [list(v or ()) for v in validator_indices]
        n = len(sigs)
        if n == 0 or len(msgs) != n or len(idx) != n or len(com) != n or len(fields) != n:
            return G.VERIFY_FAIL
        if any(len(m) != 32 for m in msgs) or any(len(s) != 96 for s in sigs):
            raise ValueError("messages must be 32-byte signing roots and signatures 96 bytes")
        if randoms is None:
            randoms = [secrets.randbits(64) or 1 for _ in range(n)]
        off, boff = [0], [0]
        for v, b in zip(idx, fields):
            off.append(off[-1] + len(v))
            boff.append(boff[-1] + len(b))
        flat = [i for v in idx for i in v]
        L = G.lib()
        st = G.i32_array(n)
        return L.gbls_multi_verify_bits(
            G.buf(b"".join(msgs)), G.buf(b"".join(sigs)), G.u32_array(com), G.buf(b"".join(fields)),
            G.u32_array(boff), G.u32_array(flat or [0]), G.u32_array(off), G.u64_array(randoms), n, st, call_flags)

    @staticmethod
    def multi_verify_compressed_spans(messages: Iterable[bytes], signature_bytes: Iterable[bytes],
                                      base_slots: Iterable[int], committee_bits: Iterable[bytes],
                                      bitfields: Iterable[bytes], validator_indices: Iterable[Sequence[int]],
                                      randoms: Sequence[int] = None, call_flags: int = 0) -> int:
        """multi_verify_compressed_bits for attestations over several committees
        (gbls_multi_verify_spans): set i names the committees ``base_slots[i] + c`` for every set
        bit c of ``committee_bits[i]`` (8 SSZ bytes), each loaded with its members, and carries ONE
        bit string ``bitfields[i]`` over their concatenation.  A set whose base slot is ``None`` is
        the plain sum of the registry keys ``validator_indices[i]``, with neither mask nor bits.
        Returns as multi_verify_compressed."""
        msgs = [bytes(m) for m in messages]
        sigs = [bytes(s) for s in signature_bytes]
        com = [G.NO_COMMITTEE if c is None else int(c) for c in base_slots]
        masks = [bytes(b or bytes(8)) for b in committee_bits]
        fields = [bytes(b or b"") for b in bitfields]
        idx = [list(v or ()) for v in validator_indices]
        n = len(sigs)
        if n == 0 or len(msgs) != n or len(idx) != n or len(com) != n or len(fields) != n or len(masks) != n:
            return G.VERIFY_FAIL
        if any(len(m) != 32 for m in msgs) or any(len(s) != 96 for s in sigs) or any(len(b) != 8 for b in masks):
            raise ValueError("messages must be 32-byte signing roots, signatures 96 bytes, committee_bits 8 bytes")
        if randoms is None:
            randoms = [secrets.randbits(64) or 1 for _ in range(n)]
        off, boff = [0], [0]
        for v, b in zip(idx, fields):
            off.append(off[-1] + len(v))
            boff.append(boff[-1] + len(b))
        flat = [i for v in idx for i in v]
        L = G.lib()
        st = G.i32_array(n)
        return L.gbls_multi_verify_spans(
            G.buf(b"".join(msgs)), G.buf(b"".join(sigs)), G.u32_array(com), G.buf(b"".join(masks)),
            G.buf(b"".join(fields)), G.u32_array(boff), G.u32_array(flat or [0]), G.u32_array(off),
            G.u64_array(randoms), n, st, call_flags)

    @staticmethod
    def _span_sets(messages, signature_bytes, base_slots, committee_bits, bitfields, validator_indices):
        """The sets of multi_verify_compressed_spans as the C arguments (msgs, sigs, com, cbits, bits,
        bits_off, pk_idx, pk_off) and their number."""
        msgs = [bytes(m) for m in messages]
        sigs = [bytes(s) for s in signature_bytes]
        com = [G.NO_COMMITTEE if c is None else int(c) for c in base_slots]
        masks = [bytes(b or bytes(8)) for b in committee_bits]
        fields = [bytes(b or b"") for b in bitfields]
        idx = [list(v or ()) for v in validator_indices]
        n = len(sigs)
        if len(msgs) != n or len(idx) != n or len(com) != n or len(fields) != n or len(masks) != n:
            raise ValueError("one message, base slot, committee_bits, bit string and index list per signature")
        if any(len(m) != 32 for m in msgs) or any(len(s) != 96 for s in sigs) or any(len(b) != 8 for b in masks):
            raise ValueError("messages must be 32-byte signing roots, signatures 96 bytes, committee_bits 8 bytes")
        off, boff = [0], [0]
        for v, b in zip(idx, fields):
            off.append(off[-1] + len(v))
            boff.append(boff[-1] + len(b))
        flat = [i for v in idx for i in v]
        return (G.buf(b"".join(msgs)), G.buf(b"".join(sigs)), G.u32_array(com), G.buf(b"".join(masks)),
                G.buf(b"".join(fields)), G.u32_array(boff), G.u32_array(flat or [0]), G.u32_array(off)), n

    @staticmethod
    def verify_each_spans(messages: Iterable[bytes], signature_bytes: Iterable[bytes], base_slots: Iterable[int],
                          committee_bits: Iterable[bytes], bitfields: Iterable[bytes],
                          validator_indices: Iterable[Sequence[int]]) -> List:
        """verify_batch_compressed over the sets of multi_verify_compressed_spans
        (gbls_verify_each_spans): every set its own check, ONE coalesced submission.  Per set:
        (signature status, key status, ok) -- the decompression status, the status of the set's key
        (nonzero: a malformed attestation, not an invalid signature) and whether it verifies."""
        args, n = Signature._span_sets(messages, signature_bytes, base_slots, committee_bits, bitfields,
                                       validator_indices)
        if n == 0:
            return []
        L = G.lib()
        st, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
        G.check(L.gbls_verify_each_spans(*args, n, st, kst, v), "gbls_verify_each_spans")
        return [(st[i], kst[i], v[i] == G.SUCCESS) for i in range(n)]

    @staticmethod
    def verify_each_fold(messages: Iterable[bytes], signature_bytes: Iterable[bytes], base_slots: Iterable[int],
                         committee_bits: Iterable[bytes], bitfields: Iterable[bytes],
                         validator_indices: Iterable[Sequence[int]], groups: Iterable[Sequence[int]]):
        """verify_each_spans which also sums the signatures that passed (gbls_verify_each_fold):
        ``groups[g]`` lists sets of this call (a set may be in several groups, and more than once in
        one).  Returns (per set (signature status, key status, ok), per group (Signature, count,
        SignatureBytes)): the sum of the decoded signatures of the group's sets that verified, how
        many occurrences entered it (0: nothing passed) and the sum compressed.  The sums are
        computed on the device behind the verdicts, in the same submission."""
        args, n = Signature._span_sets(messages, signature_bytes, base_slots, committee_bits, bitfields,
                                       validator_indices)
        grp = [[int(s) for s in g] for g in groups]
        if any(s < 0 or s >= n for g in grp for s in g):
            raise ValueError("a group names sets of this call")
        nfold = len(grp)
        if n == 0 and nfold == 0:
            return [], []
        foff = [0]
        for g in grp:
            foff.append(foff[-1] + len(g))
        flat = [s for g in grp for s in g]
        L = G.lib()
        st, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(n)
        out = ctypes.create_string_buffer(G.P2_BYTES * max(nfold, 1))
        fb = ctypes.create_string_buffer(96 * max(nfold, 1))
        cnt = G.u32_array([0] * nfold)
        G.check(L.gbls_verify_each_fold(*args, n, G.u32_array(flat or [0]), G.u32_array(foff), nfold, st, kst, v,
                                        out, fb, cnt), "gbls_verify_each_fold")
        sets = [(st[i], kst[i], v[i] == G.SUCCESS) for i in range(n)]
        folds = [(Signature(out.raw[G.P2_BYTES * g:G.P2_BYTES * (g + 1)]), cnt[g],
                  SignatureBytes(fb.raw[96 * g:96 * (g + 1)])) for g in range(nfold)]
        return sets, folds

    @staticmethod
    def verify_items_spans(messages: Iterable[bytes], signature_bytes: Iterable[bytes], base_slots: Iterable[int],
                           committee_bits: Iterable[bytes], bitfields: Iterable[bytes],
                           validator_indices: Iterable[Sequence[int]], item_offsets: Sequence[int],
                           randoms: Sequence[int] = None, call_flags: int = 0, with_statuses: bool = False):
        """Several independent multi_verify batches over such sets in ONE coalesced submission
        (gbls_verify_items_spans): sets item_offsets[s] .. item_offsets[s + 1] form item s.  Returns
        one bool per item; with_statuses: (those, per set (signature status, key status))."""
        args, n = Signature._span_sets(messages, signature_bytes, base_slots, committee_bits, bitfields,
                                       validator_indices)
        seg = [int(o) for o in item_offsets]
        nseg = len(seg) - 1
        if nseg < 0 or seg[0] != 0 or seg[-1] != n or any(a > b for a, b in zip(seg, seg[1:])):
            raise ValueError("item offsets run from 0 to the number of sets, nondecreasing")
        if n == 0 or nseg == 0:
            return ([False] * nseg, []) if with_statuses else [False] * nseg
        if randoms is None:
            randoms = [secrets.randbits(64) or 1 for _ in range(n)]
        if len(randoms) != n:
            raise ValueError("one scalar per set")
        L = G.lib()
        st, kst, v = G.i32_array(n), G.i32_array(n), G.i32_array(nseg)
        G.check(L.gbls_verify_items_spans(*args, G.u64_array(randoms), n, G.u32_array(seg), nseg, st, kst, v,
                                          call_flags), "gbls_verify_items_spans")
        verdicts = [v[s] == G.SUCCESS for s in range(nseg)]
        return (verdicts, [(st[i], kst[i]) for i in range(n)]) if with_statuses else verdicts

    @staticmethod
    def _local_table(local_keys):
        """A call's local key table as the C arguments (pkb, npkb)."""
        keys = [bytes(k) for k in local_keys]
        if any(len(k) != 48 for k in keys):
            raise ValueError("local keys are 48 compressed bytes")
        return (G.buf(b"".join(keys)) if keys else None), len(keys)

    @staticmethod
    def verify_each_local(messages: Iterable[bytes], signature_bytes: Iterable[bytes], base_slots: Iterable[int],
                          committee_bits: Iterable[bytes], bitfields: Iterable[bytes],
                          validator_indices: Iterable[Sequence[int]], local_keys: Iterable[bytes]):
        """verify_each_spans with a call-local table of compressed keys (gbls_verify_each_local): a
        set whose base slot is ``G.LOCAL_KEYS`` sums the keys ``local_keys[p]`` for the positions p
        of ``validator_indices[i]``; the keys are decoded on the device inside the same submission.
        Returns (per set (signature status, key status, ok), per local key its decoding status)."""
        args, n = Signature._span_sets(messages, signature_bytes, base_slots, committee_bits, bitfields,
                                       validator_indices)
        pkb, npkb = Signature._local_table(local_keys)
        if n == 0 and npkb == 0:
            return [], []
        L = G.lib()
        st, kst, v, pst = G.i32_array(n), G.i32_array(n), G.i32_array(n), G.i32_array(npkb)
        G.check(L.gbls_verify_each_local(*args, pkb, npkb, n, st, kst, v, pst), "gbls_verify_each_local")
        return [(st[i], kst[i], v[i] == G.SUCCESS) for i in range(n)], [pst[j] for j in range(npkb)]

    @staticmethod
    def verify_items_local(messages: Iterable[bytes], signature_bytes: Iterable[bytes], base_slots: Iterable[int],
                           committee_bits: Iterable[bytes], bitfields: Iterable[bytes],
                           validator_indices: Iterable[Sequence[int]], local_keys: Iterable[bytes],
                           item_offsets: Sequence[int], randoms: Sequence[int] = None, call_flags: int = 0,
                           with_statuses: bool = False):
        """verify_items_spans with a call-local table of compressed keys (gbls_verify_items_local;
        local sets as in verify_each_local).  Returns one bool per item; with_statuses: (those, per
        set (signature status, key status), per local key its decoding status)."""
        args, n = Signature._span_sets(messages, signature_bytes, base_slots, committee_bits, bitfields,
                                       validator_indices)
        pkb, npkb = Signature._local_table(local_keys)
        seg = [int(o) for o in item_offsets]
        nseg = len(seg) - 1
        if nseg < 0 or seg[0] != 0 or seg[-1] != n or any(a > b for a, b in zip(seg, seg[1:])):
            raise ValueError("item offsets run from 0 to the number of sets, nondecreasing")
        if (n == 0 or nseg == 0) and npkb == 0:
            return ([False] * nseg, [], []) if with_statuses else [False] * nseg
        if randoms is None:
            randoms = [secrets.randbits(64) or 1 for _ in range(n)]
        if len(randoms) != n:
            raise ValueError("one scalar per set")
        L = G.lib()
        st, kst, v, pst = G.i32_array(n), G.i32_array(n), G.i32_array(nseg), G.i32_array(npkb)
        G.check(L.gbls_verify_items_local(*args, pkb, npkb, G.u64_array(randoms), n, G.u32_array(seg), nseg, st, kst,
                                          v, pst, call_flags), "gbls_verify_items_local")
        verdicts = [v[s] == G.SUCCESS for s in range(nseg)]
        if not with_statuses:
            return verdicts
        return verdicts, [(st[i], kst[i]) for i in range(n)], [pst[j] for j in range(npkb)]

    @staticmethod
    def verify_batch_compressed(messages: Iterable[bytes], signature_bytes: Iterable[bytes],
                                public_keys: Iterable) -> List:
        """SingleVerifier::extend's try_from + verify per triple (verifier.rs:215-236) as ONE
        coalesced device submission (gbls_verify_batch_compressed).  Per check: a decompression
        status (0 = decoded, else its BLST_ERROR) and whether it verifies; keys as in
        multi_verify_compressed (a list = fast_aggregate_verify over it)."""
        msgs = [bytes(m) for m in messages]
        sigs = [bytes(s) for s in signature_bytes]
        keys = [list(k) if isinstance(k, (list, tuple)) else [k] for k in public_keys]
        n = len(sigs)
        if len(msgs) != n or len(keys) != n:
            raise ValueError("one message and one key set per signature")
        if n == 0:
            return []
        if any(len(m) != 32 for m in msgs) or any(len(s) != 96 for s in sigs):
            raise ValueError("messages must be 32-byte signing roots and signatures 96 bytes")
        off = [0]
        for k in keys:
            off.append(off[-1] + len(k))
        L = G.lib()
        st, v = G.i32_array(n), G.i32_array(n)
        G.check(L.gbls_verify_batch_compressed(
            G.buf(b"".join(msgs)), G.buf(b"".join(sigs)), G.buf(b"".join(p.raw for k in keys for p in k) or bytes(96)),
            G.u32_array(off), n, st, v), "gbls_verify_batch_compressed")
        return [(st[i], v[i] == G.SUCCESS) for i in range(n)]

    def __eq__(self, other):
        return isinstance(other, Signature) and self.raw == other.raw

    def __hash__(self):
        return hash(self.raw)


AggregateSignature = Signature


# ----------------------------------------------------------------------------- SecretKey
class SecretKey:
    """bls::SecretKey (bls/src/secret_key.rs): 32-byte big-endian scalar, 0 < sk < r."""

    __slots__ = ("_b",)

    def __init__(self, b: bytes):
        self._b = bytes(b)

    @classmethod
    def try_from(cls, data: bytes) -> "SecretKey":
        data = bytes(data)
        k = int.from_bytes(data, "big") if len(data) == 32 else 0
        if len(data) != 32 or k == 0 or k >= CURVE_ORDER:
            raise DecompressionFailed(G.BAD_ENCODING)
        return cls(data)

    def to_bytes(self) -> SecretKeyBytes:
        return SecretKeyBytes(self._b)

    def to_public_key(self) -> PublicKey:
        L = G.lib()
        out = ctypes.create_string_buffer(96)
        G.check(L.gbls_sk_to_pk(G.buf(self._b), 1, out), "gbls_sk_to_pk")
        return PublicKey(out.raw)

    def sign(self, message: bytes) -> Signature:
        L = G.lib()
        m = bytes(message)
        out = ctypes.create_string_buffer(192)
        G.check(L.gbls_sign(G.buf(self._b), G.buf(m), G.u32_array([0, len(m)]), 1, out), "gbls_sign")
        return Signature(out.raw)

    def __eq__(self, other):
        return isinstance(other, SecretKey) and self._b == other._b

    def __repr__(self):
        return "SecretKey([REDACTED])"


def sign_batch(secret_keys: Sequence[bytes], messages: Sequence[bytes]) -> List[Signature]:
    """Batched SecretKey::sign on the device (fixture / workload generation)."""
    n = len(secret_keys)
    L = G.lib()
    msgs = [bytes(m) for m in messages]
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    out = ctypes.create_string_buffer(192 * max(n, 1))
    G.check(L.gbls_sign(G.buf(b"".join(secret_keys)), G.buf(b"".join(msgs)), G.u32_array(off), n, out),
            "gbls_sign")
    return [Signature(out.raw[192 * i:192 * (i + 1)]) for i in range(n)]


def public_keys_batch(secret_keys: Sequence[bytes]) -> List[PublicKey]:
    n = len(secret_keys)
    L = G.lib()
    out = ctypes.create_string_buffer(96 * max(n, 1))
    G.check(L.gbls_sk_to_pk(G.buf(b"".join(secret_keys)), n, out), "gbls_sk_to_pk")
    return [PublicKey(out.raw[96 * i:96 * (i + 1)]) for i in range(n)]


class Registry:
    """Mirror of ``bls::gpu::registry`` (rust/bls_patch/gpu.rs, f1): the engine's device-resident
    copy of a FINALIZED validator list (indices name the same key on every fork only up to the
    finalized state).  ``mirror_finalized`` loads the new tail of the list with one
    gbls_registry_set; ``covers`` says whether a batch may name registry slots instead of key
    points."""

    _mirrored = 0

    @classmethod
    def mirror_finalized(cls, keys: Sequence[bytes]) -> int:
        n = len(keys) - cls._mirrored
        if n <= 0:
            return cls._mirrored
        tail = b"".join(bytes(k) for k in keys[cls._mirrored:])
        L = G.lib()
        st = G.i32_array(n)
        G.check(L.gbls_registry_set(cls._mirrored, G.buf(tail), n, st), "gbls_registry_set")
        cls._mirrored = len(keys)
        return cls._mirrored

    @classmethod
    def mirrored(cls) -> int:
        return cls._mirrored

    @classmethod
    def covers(cls, indices: Iterable[int]) -> bool:
        return all(0 <= int(i) < cls._mirrored for i in indices)

    @classmethod
    def forget(cls) -> None:
        """Tests: the process's engine registry was overwritten by someone else."""
        cls._mirrored = 0
        Committees.forget()  # cached sums are snapshots of the overwritten keys


class Committees:
    """The engine's cached committee key sums (include/grandine_bls_gpu_committees.h): slot s holds
    the sum of one committee's registry keys, loaded once per epoch (the sync committee once per
    period), so that a set's key is the slot minus its few ABSENT members.  The mirror remembers
    each loaded slot's member list; ``covers`` says whether a triple may name the slot.  With
    ``members=True`` the engine keeps the member lists as well (include/grandine_bls_gpu_bits.h), so
    that a set is the slot and its aggregation bits; ``has_members`` says which slots those are."""

    _members = {}  # slot -> tuple of validator indices, for slots loaded with status SUCCESS
    _resident = set()  # the slots among them whose member lists the engine keeps

    @classmethod
    def set(cls, first: int, committees: Sequence[Sequence[int]], members: bool = False) -> List[int]:
        """gbls_committees_set: committees[c] (validator indices) into slot first + c.  Returns
        the per-committee statuses; only SUCCESS slots are remembered (the others are invalid).
        members=True: gbls_committees_set_members, the slots keep their member lists on the device;
        else the slots' resident members, if any, are dropped."""
        coms = [[int(i) for i in c] for c in committees]
        off = [0]
        for c in coms:
            off.append(off[-1] + len(c))
        L = G.lib()
        st = G.i32_array(len(coms))
        for c in range(len(coms)):
            cls._members.pop(first + c, None)
            cls._resident.discard(first + c)
        call = L.gbls_committees_set_members if members else L.gbls_committees_set
        G.check(call(first, G.u32_array([i for c in coms for i in c] or [0]), G.u32_array(off),
                     len(coms), st), "gbls_committees_set_members" if members else "gbls_committees_set")
        for c, com in enumerate(coms):
            if st[c] == G.SUCCESS:
                cls._members[first + c] = tuple(com)
                if members:
                    cls._resident.add(first + c)
        return [st[c] for c in range(len(coms))]

    @classmethod
    def has_members(cls, slot: int) -> bool:
        """True when ``slot`` was loaded with members=True (and not rewritten without since)."""
        return slot is not None and int(slot) in cls._resident

    @classmethod
    def size(cls) -> int:
        return int(G.lib().gbls_committees_size())

    @classmethod
    def clear(cls) -> None:
        cls._members = {}
        cls._resident = set()
        G.check(G.lib().gbls_committees_clear(), "gbls_committees_clear")

    @classmethod
    def covers(cls, slot: int, members: Iterable[int]) -> bool:
        """True when ``slot`` was loaded with exactly this member list."""
        return slot is not None and cls._members.get(int(slot)) == tuple(int(i) for i in members)

    @classmethod
    def forget(cls) -> None:
        """Tests: the process's engine table was cleared or overwritten by someone else."""
        cls._members = {}
        cls._resident = set()


class MessageCache:
    """The engine's message line cache (include/grandine_bls_gpu_msgcache.h): per device, a
    device-resident table from a 32-byte message to its 68 Miller line events, so that a batch
    verification whose messages were verified before skips hash_to_G2 and line generation for
    them.  Off until ``configure(slots)``; 19 584 bytes per slot per device.  None of the calls
    needs a device (the memory comes with the first served verification)."""

    MAX_SLOTS = 1 << 20
    BYTES_PER_SLOT = 68 * 72 * 4

    @classmethod
    def configure(cls, slots: int) -> None:
        """gbls_msgcache_configure: the capacity in entries per device; 0 switches the cache off."""
        slots = int(slots)
        if not 0 <= slots <= cls.MAX_SLOTS:
            raise ValueError("message cache slots must be in [0, 2^20]")
        G.check(G.load_library().gbls_msgcache_configure(slots), "gbls_msgcache_configure")

    @classmethod
    def slots(cls) -> int:
        return int(G.load_library().gbls_msgcache_slots())

    @classmethod
    def clear(cls) -> None:
        """Drops every entry and keeps the capacity."""
        G.check(G.load_library().gbls_msgcache_clear(), "gbls_msgcache_clear")

    @classmethod
    def stats(cls) -> dict:
        """gbls_msgcache_stats as a dict: lookups, hits, misses, published, evictions, bypassed
        (counters since the process started) and entries (now)."""
        out = (ctypes.c_uint64 * 8)()
        G.check(G.load_library().gbls_msgcache_stats(out), "gbls_msgcache_stats")
        return {name: int(out[i]) for i, name in enumerate(G.MSGCACHE_STATS) if name != "reserved"}

    @classmethod
    def prefetch(cls, messages) -> list:
        """gbls_msgcache_prefetch: enters the 32-byte ``messages`` (signing roots the node derived
        itself -- the caller vouches for them) on every engine device, without any signature.
        Returns one status per message: ``G.PREFETCH_ENTERED``, ``PREFETCH_PRESENT`` or
        ``PREFETCH_SKIPPED`` (cache off, or no slot to spare).  Needs the engine unless the cache is
        off."""
        messages = [bytes(m) for m in messages]
        if any(len(m) != 32 for m in messages):
            raise ValueError("prefetch takes 32-byte messages")
        n = len(messages)
        status = G.i32_array(n)
        L = G.load_library()
        rc = L.gbls_msgcache_prefetch(G.buf(b"".join(messages)), n, status)
        if rc != G.SUCCESS:
            raise G.EngineUnavailable("gbls_msgcache_prefetch failed: rc=%d err=%d" % (rc, L.gbls_last_error()))
        return [int(status[i]) for i in range(n)]

    @classmethod
    def serve_checks(cls, on: bool) -> bool:
        """gbls_msgcache_serve_checks: per-check calls (verify, fast_aggregate_verify, the
        ``*_verify_batch`` calls, verify_each_*) are planned by message and served by the cache
        while on.  Off by default, process-wide and sticky.  Returns the previous setting."""
        return bool(G.load_library().gbls_msgcache_serve_checks(1 if on else 0))

    @classmethod
    def checks_stats(cls) -> dict:
        """gbls_msgcache_checks_stats as a dict: prefetched, check_lookups, check_hits,
        check_published (counters since the process started)."""
        out = (ctypes.c_uint64 * 4)()
        G.check(G.load_library().gbls_msgcache_checks_stats(out), "gbls_msgcache_checks_stats")
        return {name: int(out[i]) for i, name in enumerate(G.MSGCACHE_CHECKS_STATS)}

    @classmethod
    def memory_bytes(cls, slots: int) -> int:
        """Device memory per engine device at this capacity, spare slots included."""
        slots = int(slots)
        return 0 if slots == 0 else (slots + min(max(slots // 4, 64), 4096)) * cls.BYTES_PER_SLOT
