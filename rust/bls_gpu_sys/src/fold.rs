//! Safe wrapper of `include/grandine_bls_gpu_fold.h`: verified folds.
//!
//! `verify_each_fold` is `each::verify_each_spans` which also takes GROUPS of its own sets and
//! returns, per group, the sum of the signatures whose set verified -- computed on the device behind
//! the verdicts, in the same submission, so that no signature is decoded a second time.  It serves
//! `aggregate_attestation` (operation_pools/src/attestation_agg_pool/tasks.rs:242-257), the message
//! loops of the sync-committee pool (operation_pools/src/sync_committee_agg_pool/pool.rs:114,190)
//! and the aggregator duty (validator/src/validator.rs:2937).
//! Only the each-call has a fold: it subgroup-checks every signature, so everything in a sum is in
//! G2 (`Signature::multi_verify`, behind the items call, does not).
//! Slices are checked before the call, engine errors are values (`EngineError`), as in `each`.

use crate::each::{SetStatus, NO_COMMITTEE};
use crate::{blst_error, ffi, ffi_fold, status, EngineError, EngineResult, P2};

/// What one group's fold gave.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct Fold {
    /// the sum of the decoded signatures of the group's sets that verified (all-zero: infinity)
    pub sum: P2,
    /// how many occurrences entered the sum; 0 says that nothing passed
    pub count: u32,
    /// the sum compressed (`0xc0` followed by zeros for infinity, as `SignatureBytes::empty`)
    pub bytes: [u8; 96],
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

/// The groups: `group_offsets` describes ranges of `group_sets`, every entry names a set below `n`,
/// and the group count fits 32 bits.
fn groups_ok(group_sets: &[u32], group_offsets: &[u32], n: usize) -> bool {
    !group_offsets.is_empty()
        && u32::try_from(group_offsets.len()).is_ok()
        && ranges_ok(group_sets, group_offsets, group_offsets.len() - 1)
        && group_sets.iter().all(|&s| usize::try_from(s).is_ok_and(|s| s < n))
}

/// Every set its own check, as `each::verify_each_spans`, and per group
/// `group_sets[group_offsets[g] .. group_offsets[g + 1]]` the sum of the signatures of its sets that
/// verified.  A set may be in several groups and more than once in one (each occurrence adds once);
/// a set that fails for any reason is in no sum.  `group_offsets == [0]` asks for no group.
#[allow(clippy::too_many_arguments)]
pub fn verify_each_fold(
    messages: &[[u8; 32]],
    signatures: &[[u8; 96]],
    bases: &[u32],
    masks: &[[u8; 8]],
    bits: &[u8],
    bit_offsets: &[u32],
    indices: &[u32],
    index_offsets: &[u32],
    group_sets: &[u32],
    group_offsets: &[u32],
) -> EngineResult<(Vec<(bool, SetStatus)>, Vec<Fold>)> {
    let n = messages.len();
    if signatures.len() != n
        || bases.len() != n
        || !sets_ok(bases, masks, bits, bit_offsets, indices, index_offsets)
        || !groups_ok(group_sets, group_offsets, n)
    {
        return Err(EngineError::Argument);
    }
    let groups = group_offsets.len() - 1;
    let mut sig_statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let mut key_statuses = vec![ffi::GBLS_BAD_ENCODING; n];
    let mut verdicts = vec![ffi::GBLS_VERIFY_FAIL; n];
    let mut sums = vec![P2::default(); groups];
    let mut counts = vec![0_u32; groups];
    let mut bytes = vec![[0_u8; 96]; groups];
    // SAFETY: live slices of n elements each, `bits` of bit_offsets[n] bytes, `indices` of
    // index_offsets[n] entries, both offset lists of n + 1, `group_offsets` of groups + 1 values
    // ending at group_sets.len(), every group entry below n (checked above); the three per-set
    // outputs have n slots each, the three per-group outputs `groups` slots each.
    let rc = unsafe {
        ffi_fold::gbls_verify_each_fold(
            messages.as_ptr(),
            signatures.as_ptr(),
            bases.as_ptr(),
            masks.as_ptr(),
            bits.as_ptr(),
            bit_offsets.as_ptr(),
            indices.as_ptr(),
            index_offsets.as_ptr(),
            n,
            group_sets.as_ptr(),
            group_offsets.as_ptr(),
            groups,
            sig_statuses.as_mut_ptr(),
            key_statuses.as_mut_ptr(),
            verdicts.as_mut_ptr(),
            sums.as_mut_ptr(),
            bytes.as_mut_ptr(),
            counts.as_mut_ptr(),
        )
    };
    status(rc)?;
    let sets = verdicts
        .into_iter()
        .zip(sig_statuses.into_iter().zip(key_statuses))
        .map(|(v, (s, k))| (v == ffi::GBLS_SUCCESS, SetStatus { signature: blst_error(s), key: blst_error(k) }))
        .collect();
    let folds = sums
        .into_iter()
        .zip(counts)
        .zip(bytes)
        .map(|((sum, count), bytes)| Fold { sum, count, bytes })
        .collect();
    Ok((sets, folds))
}
