//! Safe wrappers of `include/grandine_bls_gpu_local.h`: the calls of `each` with a call-local table
//! of compressed public keys, decoded on the device inside the submission.
//!
//! A set whose base is `LOCAL_KEYS` sums the table positions of its index range.  This is the form
//! of a deposit's pubkey (`validate_deposits`: `verify_items_local` with one item is the optimistic
//! batch, `verify_each_local` the per-deposit fallback), of a BLS-to-execution change's
//! `from_bls_pubkey`, and of a validator above the mirrored registry length.  Beside the verdicts
//! and the statuses of `each`, every call reports `PublicKey::try_from`'s outcome per table key.
//! Slices are checked before every call, engine errors are values (`EngineError`), as in `each`.

use blst::BLST_ERROR;

use crate::{blst_error, each::SetStatus, ffi, ffi_local, status, CallClass, EngineError, EngineResult, P1};

pub use crate::ffi_committees::GBLS_NO_COMMITTEE as NO_COMMITTEE;
pub use crate::ffi_local::GBLS_LOCAL_KEYS as LOCAL_KEYS;

/// `offsets` describes `n` ranges of `items`: n + 1 nondecreasing values from 0 to items.len().
fn ranges_ok<T>(items: &[T], offsets: &[u32], n: usize) -> bool {
    offsets.len() == n + 1
        && offsets.first() == Some(&0)
        && offsets.windows(2).all(|w| w[0] <= w[1])
        && usize::try_from(offsets[n]).is_ok_and(|last| last == items.len())
}

/// Both range lists of a batch of `bases.len()` sets, one mask per set, each set of one kind (a
/// span set has bits and no indices; a `NO_COMMITTEE` or `LOCAL_KEYS` set indices, no bits and an
/// empty mask), and a key table whose length fits 32 bits.
fn sets_ok(
    bases: &[u32],
    masks: &[[u8; 8]],
    bits: &[u8],
    bit_offsets: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
    keys: &[[u8; 48]],
) -> bool {
    let n = bases.len();
    masks.len() == n
        && u32::try_from(keys.len()).is_ok()
        && ranges_ok(bits, bit_offsets, n)
        && ranges_ok(indices, index_offsets, n)
        && bases.iter().enumerate().all(|(i, &s)| {
            if s == NO_COMMITTEE || s == LOCAL_KEYS {
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

fn key_statuses(raw: Vec<i32>) -> Vec<BLST_ERROR> {
    raw.into_iter().map(blst_error).collect()
}

/// The keys of the sets (all-zero with a nonzero status for a rejected set), and the decoding
/// status of every table key.
#[allow(clippy::type_complexity)]
pub fn aggregate_local(
    bases: &[u32],
    masks: &[[u8; 8]],
    bits: &[u8],
    bit_offsets: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
    keys: &[[u8; 48]],
) -> EngineResult<(Vec<(P1, BLST_ERROR)>, Vec<BLST_ERROR>)> {
    let n = bases.len();
    if !sets_ok(bases, masks, bits, bit_offsets, indices, index_offsets, keys) {
        return Err(EngineError::Argument);
    }
    let mut out = vec![P1::default(); n];
    let mut statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let mut table = vec![ffi::GBLS_BAD_ENCODING; keys.len()];
    // SAFETY: live slices: n bases and masks, `bits` of bit_offsets[n] bytes, `indices` of
    // index_offsets[n] entries, both offset lists of n + 1, keys.len() table keys (checked above);
    // `out` and `statuses` have n slots, `table` has keys.len().
    let rc = unsafe {
        ffi_local::gbls_g1_aggregate_local(
            bases.as_ptr(),
            masks.as_ptr(),
            bits.as_ptr(),
            bit_offsets.as_ptr(),
            indices.as_ptr(),
            index_offsets.as_ptr(),
            keys.as_ptr(),
            keys.len(),
            n,
            out.as_mut_ptr(),
            statuses.as_mut_ptr(),
            table.as_mut_ptr(),
        )
    };
    status(rc)?;
    Ok((out.into_iter().zip(statuses.into_iter().map(blst_error)).collect(), key_statuses(table)))
}

/// `each::verify_each_spans` over span, plain and local sets: per set whether it verifies and its
/// statuses, and the decoding status of every table key.
#[allow(clippy::too_many_arguments, clippy::type_complexity)]
pub fn verify_each_local(
    messages: &[[u8; 32]],
    signatures: &[[u8; 96]],
    bases: &[u32],
    masks: &[[u8; 8]],
    bits: &[u8],
    bit_offsets: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
    keys: &[[u8; 48]],
) -> EngineResult<(Vec<(bool, SetStatus)>, Vec<BLST_ERROR>)> {
    let n = messages.len();
    if signatures.len() != n
        || bases.len() != n
        || !ranges_ok(bits, bit_offsets, n)
        || !sets_ok(bases, masks, bits, bit_offsets, indices, index_offsets, keys)
    {
        return Err(EngineError::Argument);
    }
    let mut sig_statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let mut set_key_statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let mut verdicts = vec![ffi::GBLS_VERIFY_FAIL; n];
    let mut table = vec![ffi::GBLS_BAD_ENCODING; keys.len()];
    // SAFETY: live slices of n elements each, `bits` of bit_offsets[n] bytes, `indices` of
    // index_offsets[n] entries, both offset lists of n + 1, keys.len() table keys (checked above);
    // the three set outputs have n slots each, `table` has keys.len().
    let rc = unsafe {
        ffi_local::gbls_verify_each_local(
            messages.as_ptr(),
            signatures.as_ptr(),
            bases.as_ptr(),
            masks.as_ptr(),
            bits.as_ptr(),
            bit_offsets.as_ptr(),
            indices.as_ptr(),
            index_offsets.as_ptr(),
            keys.as_ptr(),
            keys.len(),
            n,
            sig_statuses.as_mut_ptr(),
            set_key_statuses.as_mut_ptr(),
            verdicts.as_mut_ptr(),
            table.as_mut_ptr(),
        )
    };
    status(rc)?;
    Ok((
        verdicts
            .into_iter()
            .map(|v| v == ffi::GBLS_SUCCESS)
            .zip(set_statuses(sig_statuses, set_key_statuses))
            .collect(),
        key_statuses(table),
    ))
}

/// `each::verify_items_spans` over span, plain and local sets: one verdict per item, the statuses
/// of every set, and the decoding status of every table key.
#[allow(clippy::too_many_arguments, clippy::type_complexity)]
pub fn verify_items_local(
    messages: &[[u8; 32]],
    signatures: &[[u8; 96]],
    bases: &[u32],
    masks: &[[u8; 8]],
    bits: &[u8],
    bit_offsets: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
    keys: &[[u8; 48]],
    scalars: &[u64],
    item_offsets: &[u32],
    class: CallClass,
) -> EngineResult<(Vec<bool>, Vec<SetStatus>, Vec<BLST_ERROR>)> {
    let n = messages.len();
    if item_offsets.is_empty()
        || signatures.len() != n
        || bases.len() != n
        || scalars.len() != n
        || scalars.contains(&0)
        || !ranges_ok(messages, item_offsets, item_offsets.len() - 1)
        || !sets_ok(bases, masks, bits, bit_offsets, indices, index_offsets, keys)
    {
        return Err(EngineError::Argument);
    }
    let items = item_offsets.len() - 1;
    let mut sig_statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let mut set_key_statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let mut verdicts = vec![ffi::GBLS_VERIFY_FAIL; items];
    let mut table = vec![ffi::GBLS_BAD_ENCODING; keys.len()];
    let flags = match class {
        CallClass::Normal => 0,
        CallClass::BlockImport => ffi::GBLS_CALL_BLOCK,
    };
    // SAFETY: live slices of n elements each, `bits` of bit_offsets[n] bytes, `indices` of
    // index_offsets[n] entries, both offset lists of n + 1, `item_offsets` of items + 1 values
    // ending at n, keys.len() table keys (checked above); the status outputs have n slots each,
    // `verdicts` has `items`, `table` has keys.len().
    let rc = unsafe {
        ffi_local::gbls_verify_items_local(
            messages.as_ptr(),
            signatures.as_ptr(),
            bases.as_ptr(),
            masks.as_ptr(),
            bits.as_ptr(),
            bit_offsets.as_ptr(),
            indices.as_ptr(),
            index_offsets.as_ptr(),
            keys.as_ptr(),
            keys.len(),
            scalars.as_ptr(),
            n,
            item_offsets.as_ptr(),
            items,
            sig_statuses.as_mut_ptr(),
            set_key_statuses.as_mut_ptr(),
            verdicts.as_mut_ptr(),
            table.as_mut_ptr(),
            flags,
        )
    };
    status(rc)?;
    Ok((
        verdicts.into_iter().map(|v| v == ffi::GBLS_SUCCESS).collect(),
        set_statuses(sig_statuses, set_key_statuses),
        key_statuses(table),
    ))
}
