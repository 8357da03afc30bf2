//! Safe wrappers of `include/grandine_bls_gpu_committees.h`: cached committee key sums.
//!
//! A committee is fixed for an epoch (the sync committee for a period) and named by every
//! aggregator, block and sync aggregate of that time, and participation is high: with the
//! committee's whole key sum cached on the device, a set's key is that sum MINUS its few absent
//! members.  Slices are checked before every call, engine errors are values (`EngineError`), as in
//! the wrappers of `lib.rs`.

use core::ffi::c_int;

use blst::BLST_ERROR;

use crate::{blst_error, ffi, ffi_committees, last_error, status, CallClass, EngineError, EngineResult, P1};

pub use crate::ffi_committees::GBLS_NO_COMMITTEE as NO_COMMITTEE;

/// `offsets` describes `n` ranges of `items`: n + 1 nondecreasing values from 0 to items.len().
fn ranges_ok(items: &[u32], offsets: &[u32], n: usize) -> bool {
    offsets.len() == n + 1
        && offsets.first() == Some(&0)
        && offsets.windows(2).all(|w| w[0] <= w[1])
        && usize::try_from(offsets[n]).is_ok_and(|last| last == items.len())
}

/// Loads committee table slots `first ..`: slot `first + c` holds the sum of the registry keys
/// `indices[offsets[c] .. offsets[c + 1]]`, a snapshot of the registry at this call.  Per
/// committee: `Ok(())`, or why the slot is invalid (an empty committee, an index that names no
/// valid registry key); a set naming an invalid slot fails.
pub fn committees_set(
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
        ffi_committees::gbls_committees_set(
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

/// The number of committee table slots (0 before any `committees_set`, and after a registry
/// rewrite, which clears the table).
#[must_use]
pub fn committees_size() -> usize {
    // SAFETY: no arguments; the library guards its table with its own lock.
    unsafe { ffi_committees::gbls_committees_size() }
}

/// Drops every cached sum.
pub fn committees_clear() -> EngineResult<()> {
    // SAFETY: no arguments; the library guards its table with its own lock.
    let rc = unsafe { ffi_committees::gbls_committees_clear() };
    status(rc)
}

/// Per set: the key `committee[slots[i]] - sum of registry[indices[range i]]`, or the range's plain
/// sum when `slots[i]` is `NO_COMMITTEE`; `Err` for a set whose slot or indices are invalid.
pub fn g1_aggregate_committees(
    slots: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
) -> EngineResult<Vec<Result<P1, BLST_ERROR>>> {
    let n = slots.len();
    if !ranges_ok(indices, index_offsets, n) {
        return Err(EngineError::Argument);
    }
    let mut keys = vec![P1::default(); n];
    let mut statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    // SAFETY: live slices: `slots` of n entries, `index_offsets` of n + 1, `indices` of
    // index_offsets[n] (checked above); `keys` and `statuses` have n slots each.
    let rc = unsafe {
        ffi_committees::gbls_g1_aggregate_committees(
            slots.as_ptr(),
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

/// `MultiVerifier::finish` as one submission over cached committee sums: set i's key is committee
/// slot `slots[i]` minus the registry keys of its range (its absent members), or the range's sum
/// for `NO_COMMITTEE`.  `Ok(Err(e))`: the first signature that does not decode; `Ok(Ok(v))`: the
/// verdict.  An invalid slot or index fails its set (a verdict, not an error).
pub fn multi_verify_committees(
    messages: &[[u8; 32]],
    signatures: &[[u8; 96]],
    slots: &[u32],
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
        || !ranges_ok(indices, index_offsets, n)
    {
        return Err(EngineError::Argument);
    }
    let mut statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let flags = match class {
        CallClass::Normal => 0,
        CallClass::BlockImport => ffi::GBLS_CALL_BLOCK,
    };
    // SAFETY: live slices of n elements each, `indices` of index_offsets[n] entries and
    // `index_offsets` of n + 1 (checked above).
    let rc: c_int = unsafe {
        ffi_committees::gbls_multi_verify_committees(
            messages.as_ptr(),
            signatures.as_ptr(),
            slots.as_ptr(),
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
