//! Safe wrappers of `include/grandine_bls_gpu_each.h`: per-set and per-item verdicts over the span
//! sets of `spans`, merged with concurrent callers by the engine's coalescer.
//!
//! After a failed gossip batch `verify_each_spans` says which sets verify on their own without
//! returning to explicit key points; `verify_items_spans` verifies several independent batches
//! (the blocks of the block verification pool, or gossip aggregates as 3-set items) in one
//! submission.  Both report, per set, the signature's decoding status and the key's status, so that
//! a malformed attestation is told from an invalid signature.
//! Slices are checked before every call, engine errors are values (`EngineError`), as in `spans`.

use blst::BLST_ERROR;

use crate::{blst_error, ffi, ffi_each, status, CallClass, EngineError, EngineResult};

pub use crate::ffi_committees::GBLS_NO_COMMITTEE as NO_COMMITTEE;

/// What the engine found about one set beside its verdict.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct SetStatus {
    /// `Signature::try_from` of the set's signature bytes
    pub signature: BLST_ERROR,
    /// the set's key: `BLST_SUCCESS` for a valid key and for one that cancels to infinity,
    /// `BLST_BAD_ENCODING` for a malformed span set or a bad registry index,
    /// `BLST_AGGR_TYPE_MISMATCH` for an empty plain list
    pub key: BLST_ERROR,
}

/// `offsets` describes `n` ranges of `items`: n + 1 nondecreasing values from 0 to items.len().
fn ranges_ok<T>(items: &[T], offsets: &[u32], n: usize) -> bool {
    offsets.len() == n + 1
        && offsets.first() == Some(&0)
        && offsets.windows(2).all(|w| w[0] <= w[1])
        && usize::try_from(offsets[n]).is_ok_and(|last| last == items.len())
}

/// Both range lists of a batch of `bases.len()` sets, one mask per set, and each set of one kind:
/// a span set has bits and no indices, a `NO_COMMITTEE` set indices, no bits and an empty mask.
fn sets_ok(
    bases: &[u32],
    masks: &[[u8; 8]],
    bits: &[u8],
    bit_offsets: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
) -> bool {
    let n = bases.len();
    masks.len() == n
        && ranges_ok(bits, bit_offsets, n)
        && ranges_ok(indices, index_offsets, n)
        && bases.iter().enumerate().all(|(i, &s)| {
            if s == NO_COMMITTEE {
                bit_offsets[i] == bit_offsets[i + 1] && masks[i] == [0u8; 8]
            } else {
                index_offsets[i] == index_offsets[i + 1]
            }
        })
}

fn set_statuses(signatures: Vec<i32>, keys: Vec<i32>) -> Vec<SetStatus> {
    signatures
        .into_iter()
        .zip(keys)
        .map(|(s, k)| SetStatus { signature: blst_error(s), key: blst_error(k) })
        .collect()
}

/// Every set its own check (`Signature::verify` / `fast_aggregate_verify` semantics) in one
/// submission: per set whether it verifies, and its statuses.  A set whose signature does not
/// decode, or whose key the engine rejects, is `false`; it never changes a neighbour's outcome.
pub fn verify_each_spans(
    messages: &[[u8; 32]],
    signatures: &[[u8; 96]],
    bases: &[u32],
    masks: &[[u8; 8]],
    bits: &[u8],
    bit_offsets: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
) -> EngineResult<Vec<(bool, SetStatus)>> {
    let n = messages.len();
    if signatures.len() != n
        || bases.len() != n
        || !ranges_ok(bits, bit_offsets, n)
        || !sets_ok(bases, masks, bits, bit_offsets, indices, index_offsets)
    {
        return Err(EngineError::Argument);
    }
    let mut sig_statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let mut key_statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let mut verdicts = vec![ffi::GBLS_VERIFY_FAIL; n];
    // SAFETY: live slices of n elements each, `bits` of bit_offsets[n] bytes, `indices` of
    // index_offsets[n] entries, both offset lists of n + 1 (checked above); the three outputs have
    // n slots each.
    let rc = unsafe {
        ffi_each::gbls_verify_each_spans(
            messages.as_ptr(),
            signatures.as_ptr(),
            bases.as_ptr(),
            masks.as_ptr(),
            bits.as_ptr(),
            bit_offsets.as_ptr(),
            indices.as_ptr(),
            index_offsets.as_ptr(),
            n,
            sig_statuses.as_mut_ptr(),
            key_statuses.as_mut_ptr(),
            verdicts.as_mut_ptr(),
        )
    };
    status(rc)?;
    Ok(verdicts
        .into_iter()
        .map(|v| v == ffi::GBLS_SUCCESS)
        .zip(set_statuses(sig_statuses, key_statuses))
        .collect())
}

/// Several independent `multi_verify` batches in one submission: sets
/// `item_offsets[s] .. item_offsets[s + 1]` form item `s`.  Returns one verdict per item and the
/// statuses of every set.  An empty item is `false`.
#[allow(clippy::too_many_arguments)]
pub fn verify_items_spans(
    messages: &[[u8; 32]],
    signatures: &[[u8; 96]],
    bases: &[u32],
    masks: &[[u8; 8]],
    bits: &[u8],
    bit_offsets: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
    scalars: &[u64],
    item_offsets: &[u32],
    class: CallClass,
) -> EngineResult<(Vec<bool>, Vec<SetStatus>)> {
    let n = messages.len();
    if item_offsets.is_empty()
        || signatures.len() != n
        || bases.len() != n
        || scalars.len() != n
        || scalars.contains(&0)
        || !ranges_ok(messages, item_offsets, item_offsets.len() - 1)
        || !sets_ok(bases, masks, bits, bit_offsets, indices, index_offsets)
    {
        return Err(EngineError::Argument);
    }
    let items = item_offsets.len() - 1;
    let mut sig_statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let mut key_statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let mut verdicts = vec![ffi::GBLS_VERIFY_FAIL; items];
    let flags = match class {
        CallClass::Normal => 0,
        CallClass::BlockImport => ffi::GBLS_CALL_BLOCK,
    };
    // SAFETY: live slices of n elements each, `bits` of bit_offsets[n] bytes, `indices` of
    // index_offsets[n] entries, both offset lists of n + 1, `item_offsets` of items + 1 values
    // ending at n (checked above); the status outputs have n slots each, `verdicts` has `items`.
    let rc = unsafe {
        ffi_each::gbls_verify_items_spans(
            messages.as_ptr(),
            signatures.as_ptr(),
            bases.as_ptr(),
            masks.as_ptr(),
            bits.as_ptr(),
            bit_offsets.as_ptr(),
            indices.as_ptr(),
            index_offsets.as_ptr(),
            scalars.as_ptr(),
            n,
            item_offsets.as_ptr(),
            items,
            sig_statuses.as_mut_ptr(),
            key_statuses.as_mut_ptr(),
            verdicts.as_mut_ptr(),
            flags,
        )
    };
    status(rc)?;
    Ok((
        verdicts.into_iter().map(|v| v == ffi::GBLS_SUCCESS).collect(),
        set_statuses(sig_statuses, key_statuses),
    ))
}
