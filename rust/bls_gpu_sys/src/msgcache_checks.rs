//! Safe wrappers of `include/grandine_bls_gpu_msgcache_checks.h`: the message line cache serves
//! per-check calls (`Signature::verify`, `fast_aggregate_verify`, `SingleVerifier::extend`, the
//! per-set calls) while `msgcache_serve_checks(true)`, and `msgcache_prefetch` enters roots the
//! node knows before any signature arrives.
//!
//! The caller vouches for prefetched roots: the cache otherwise enters a message only after a
//! verification that carried it passed, so that a peer's junk never evicts an entry, and prefetch
//! bypasses that rule.  Prefetch only roots the node derived itself.  Engine errors are values
//! (`EngineError`), as in `lib.rs`.

use crate::{ffi_msgcache_checks, status, EngineResult};

/// What `msgcache_prefetch` did with one message.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Prefetch {
    /// entered by this call
    Entered,
    /// was an entry already (its recency is refreshed)
    Present,
    /// not entered: cache off, no spare slot, no evictable entry
    Skipped,
}

/// `gbls_msgcache_checks_stats`: counters since the process started.
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct MsgCacheChecksStats {
    /// messages a prefetch call reported entered
    pub prefetched: u64,
    /// distinct messages looked up by served per-check submissions
    pub check_lookups: u64,
    pub check_hits: u64,
    pub check_published: u64,
}

/// Enters `msgs` on every engine device and waits for it; one status per message.  With the cache
/// off every status is `Skipped` and no device is needed.
pub fn msgcache_prefetch(msgs: &[[u8; 32]]) -> EngineResult<Vec<Prefetch>> {
    let mut st = vec![ffi_msgcache_checks::GBLS_PREFETCH_SKIPPED; msgs.len()];
    // SAFETY: `msgs` and `st` are live slices of `msgs.len()` elements each; the call reads the
    // former and writes the latter, and keeps neither pointer.
    let rc = unsafe { ffi_msgcache_checks::gbls_msgcache_prefetch(msgs.as_ptr(), msgs.len(), st.as_mut_ptr()) };
    status(rc)?;
    Ok(st
        .into_iter()
        .map(|s| match s {
            ffi_msgcache_checks::GBLS_PREFETCH_ENTERED => Prefetch::Entered,
            ffi_msgcache_checks::GBLS_PREFETCH_PRESENT => Prefetch::Present,
            _ => Prefetch::Skipped,
        })
        .collect())
}

/// Serves per-check calls from the cache (or stops doing so); process-wide and sticky, off by
/// default.  Returns the previous setting.
pub fn msgcache_serve_checks(on: bool) -> bool {
    // SAFETY: a scalar argument; the setting is an atomic of the library.
    let prev = unsafe { ffi_msgcache_checks::gbls_msgcache_serve_checks(i32::from(on)) };
    prev != 0
}

/// Reads the counters.
pub fn msgcache_checks_stats() -> EngineResult<MsgCacheChecksStats> {
    let mut out = [0u64; 4];
    // SAFETY: `out` is a live array of the four values the call writes.
    let rc = unsafe { ffi_msgcache_checks::gbls_msgcache_checks_stats(out.as_mut_ptr()) };
    status(rc)?;
    Ok(MsgCacheChecksStats {
        prefetched: out[0],
        check_lookups: out[1],
        check_hits: out[2],
        check_published: out[3],
    })
}
