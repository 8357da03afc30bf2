//! Safe wrappers of `include/grandine_bls_gpu_bits.h`: aggregation-bit sets over resident committee
//! members.
//!
//! An attestation arrives as (committee, aggregation bits, signature).  With the committee's member
//! list resident on the device beside its cached key sum, a set is the committee's slot and the
//! SSZ bytes of its bits as they arrived: the engine checks the bits against the committee and
//! chooses between summing the participants and subtracting the absentees.  Slices are checked
//! before every call, engine errors are values (`EngineError`), as in the wrappers of `lib.rs`.

use core::ffi::c_int;

use blst::BLST_ERROR;

use crate::{blst_error, ffi, ffi_bits, last_error, status, CallClass, EngineError, EngineResult, P1};

pub use crate::ffi_committees::GBLS_NO_COMMITTEE as NO_COMMITTEE;

/// `offsets` describes `n` ranges of `items`: n + 1 nondecreasing values from 0 to items.len().
fn ranges_ok<T>(items: &[T], offsets: &[u32], n: usize) -> bool {
    offsets.len() == n + 1
        && offsets.first() == Some(&0)
        && offsets.windows(2).all(|w| w[0] <= w[1])
        && usize::try_from(offsets[n]).is_ok_and(|last| last == items.len())
}

/// Both range lists of a batch of `slots.len()` sets, and each set of one kind: a committee set
/// has bits and no indices, a `NO_COMMITTEE` set indices and no bits.
fn sets_ok(slots: &[u32], bits: &[u8], bit_offsets: &[u32], indices: &[u32], index_offsets: &[u32]) -> bool {
    let n = slots.len();
    ranges_ok(bits, bit_offsets, n)
        && ranges_ok(indices, index_offsets, n)
        && slots.iter().enumerate().all(|(i, &s)| {
            if s == NO_COMMITTEE {
                bit_offsets[i] == bit_offsets[i + 1]
            } else {
                index_offsets[i] == index_offsets[i + 1]
            }
        })
}

/// `committees::committees_set` that also keeps each slot's member list on the device, so that
/// sets may name the slot with their aggregation bits.  Per committee: `Ok(())`, or why the slot
/// is invalid; an invalid slot keeps no members.
pub fn committees_set_members(
    first: usize,
    indices: &[u32],
    offsets: &[u32],
) -> EngineResult<Vec<Result<(), BLST_ERROR>>> {
    let Some(ncom) = offsets.len().checked_sub(1) else {
        return Err(EngineError::Argument);
    };
    if !ranges_ok(indices, offsets, ncom) {
        return Err(EngineError::Argument);
    }
    let mut statuses = vec![ffi::GBLS_BAD_ENCODING; ncom];
    // SAFETY: `offsets` is a live slice of ncom + 1 entries, `indices` of offsets[ncom] entries
    // (checked above) and `statuses` of ncom slots.
    let rc = unsafe {
        ffi_bits::gbls_committees_set_members(
            first,
            indices.as_ptr(),
            offsets.as_ptr(),
            ncom,
            statuses.as_mut_ptr(),
        )
    };
    status(rc)?;
    Ok(statuses.into_iter().map(|s| if s == ffi::GBLS_SUCCESS { Ok(()) } else { Err(blst_error(s)) }).collect())
}

/// The number of members the engine keeps for `slot`; 0 when it keeps none (the slot was loaded
/// without members, rewritten, cleared, or never written).
#[must_use]
pub fn committees_members(slot: usize) -> usize {
    // SAFETY: a plain value argument; the library guards its table with its own lock.
    unsafe { ffi_bits::gbls_committees_members(slot) }
}

/// Per set: the sum of the members of committee `slots[i]` whose bit is set in
/// `bits[bit_offsets[i] .. bit_offsets[i + 1]]` (SSZ bytes, Bitlist or Bitvector), or, for
/// `NO_COMMITTEE`, the sum of the registry keys of its index range.  `Err` for a set whose bits do
/// not fit its committee, whose slot keeps no members, or whose indices are invalid.
pub fn g1_aggregate_bits(
    slots: &[u32],
    bits: &[u8],
    bit_offsets: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
) -> EngineResult<Vec<Result<P1, BLST_ERROR>>> {
    let n = slots.len();
    if !ranges_ok(bits, bit_offsets, n) || !sets_ok(slots, bits, bit_offsets, indices, index_offsets) {
        return Err(EngineError::Argument);
    }
    let mut keys = vec![P1::default(); n];
    let mut statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    // SAFETY: live slices: `slots` of n entries, `bit_offsets` and `index_offsets` of n + 1,
    // `bits` of bit_offsets[n] bytes and `indices` of index_offsets[n] entries (checked above);
    // `keys` and `statuses` have n slots each.
    let rc = unsafe {
        ffi_bits::gbls_g1_aggregate_bits(
            slots.as_ptr(),
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

/// `MultiVerifier::finish` as one submission over such sets: the attestations and the sync
/// aggregate as (slot, bits), the proposer, RANDAO and exit signatures as `NO_COMMITTEE` sets with
/// their registry indices.  `Ok(Err(e))`: the first signature that does not decode; `Ok(Ok(v))`:
/// the verdict.  Bits that do not fit their committee fail the set (a verdict, not an error).
#[allow(clippy::too_many_arguments)]
pub fn multi_verify_bits(
    messages: &[[u8; 32]],
    signatures: &[[u8; 96]],
    slots: &[u32],
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
        || slots.len() != n
        || scalars.len() != n
        || scalars.contains(&0)
        || !ranges_ok(bits, bit_offsets, n)
        || !sets_ok(slots, bits, bit_offsets, indices, index_offsets)
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
        ffi_bits::gbls_multi_verify_bits(
            messages.as_ptr(),
            signatures.as_ptr(),
            slots.as_ptr(),
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
