//! Safe wrappers of `include/grandine_bls_gpu_spans.h`: span sets, attestations over several
//! committees.
//!
//! Since EIP-7549 an attestation is (`committee_bits`, `aggregation_bits`, signature): the mask
//! names up to 64 committees of the slot, the one bit string is the concatenation of their bits in
//! ascending committee order.  With the slot's committees in consecutive table slots (loaded by
//! `bits::committees_set_members`), a set is the base slot, the mask's 8 SSZ bytes and the string
//! as it arrived.  Unlike a single-committee set of `bits`, a named committee without a participant
//! rejects its set.  Checking `committee_index < committees_per_slot` stays with the caller.
//! Slices are checked before every call, engine errors are values (`EngineError`), as in `bits`.

use core::ffi::c_int;

use blst::BLST_ERROR;

use crate::{blst_error, ffi, ffi_spans, last_error, status, CallClass, EngineError, EngineResult, P1};

pub use crate::ffi_committees::GBLS_NO_COMMITTEE as NO_COMMITTEE;

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

/// Per set: the sum, over the committees `bases[i] + c` named by `masks[i]`, of the members whose
/// bit is set in `bits[bit_offsets[i] .. bit_offsets[i + 1]]`, or, for `NO_COMMITTEE`, the sum of
/// the registry keys of its index range.  `Err` for a set whose mask is empty, whose bits do not
/// fit its committees, one of whose committees has no participant or keeps no members, or whose
/// indices are invalid.
pub fn g1_aggregate_spans(
    bases: &[u32],
    masks: &[[u8; 8]],
    bits: &[u8],
    bit_offsets: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
) -> EngineResult<Vec<Result<P1, BLST_ERROR>>> {
    let n = bases.len();
    if !ranges_ok(bits, bit_offsets, n) || !sets_ok(bases, masks, bits, bit_offsets, indices, index_offsets) {
        return Err(EngineError::Argument);
    }
    let mut keys = vec![P1::default(); n];
    let mut statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    // SAFETY: live slices: `bases` and `masks` of n entries, `bit_offsets` and `index_offsets` of
    // n + 1, `bits` of bit_offsets[n] bytes and `indices` of index_offsets[n] entries (checked
    // above); `keys` and `statuses` have n slots each.
    let rc = unsafe {
        ffi_spans::gbls_g1_aggregate_spans(
            bases.as_ptr(),
            masks.as_ptr(),
            bits.as_ptr(),
            bit_offsets.as_ptr(),
            indices.as_ptr(),
            index_offsets.as_ptr(),
            n,
            keys.as_mut_ptr(),
            statuses.as_mut_ptr(),
        )
    };
    status(rc)?;
    Ok(keys
        .into_iter()
        .zip(statuses)
        .map(|(k, s)| if s == ffi::GBLS_SUCCESS { Ok(k) } else { Err(blst_error(s)) })
        .collect())
}

/// `MultiVerifier::finish` as one submission over such sets: a block's attestations as (base slot,
/// `committee_bits`, `aggregation_bits`), the sync aggregate as a span with one bit, the proposer,
/// RANDAO and exit signatures as `NO_COMMITTEE` sets with their registry indices.  `Ok(Err(e))`:
/// the first signature that does not decode; `Ok(Ok(v))`: the verdict.  A set the engine rejects
/// fails the batch (a verdict, not an error).
#[allow(clippy::too_many_arguments)]
pub fn multi_verify_spans(
    messages: &[[u8; 32]],
    signatures: &[[u8; 96]],
    bases: &[u32],
    masks: &[[u8; 8]],
    bits: &[u8],
    bit_offsets: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
    scalars: &[u64],
    class: CallClass,
) -> EngineResult<Result<bool, BLST_ERROR>> {
    let n = messages.len();
    if n == 0
        || signatures.len() != n
        || bases.len() != n
        || scalars.len() != n
        || scalars.contains(&0)
        || !ranges_ok(bits, bit_offsets, n)
        || !sets_ok(bases, masks, bits, bit_offsets, indices, index_offsets)
    {
        return Err(EngineError::Argument);
    }
    let mut statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let flags = match class {
        CallClass::Normal => 0,
        CallClass::BlockImport => ffi::GBLS_CALL_BLOCK,
    };
    // SAFETY: live slices of n elements each, `bits` of bit_offsets[n] bytes, `indices` of
    // index_offsets[n] entries, both offset lists of n + 1 (checked above).
    let rc: c_int = unsafe {
        ffi_spans::gbls_multi_verify_spans(
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
            statuses.as_mut_ptr(),
            flags,
        )
    };
    if let Some(e) = last_error() {
        return Err(e);
    }
    Ok(match rc {
        ffi::GBLS_SUCCESS => Ok(true),
        ffi::GBLS_VERIFY_FAIL => Ok(false),
        decode => Err(blst_error(decode)),
    })
}
