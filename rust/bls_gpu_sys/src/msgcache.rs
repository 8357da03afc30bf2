//! Safe wrappers of `include/grandine_bls_gpu_msgcache.h`: the message line cache.
//!
//! Per engine device, a device-resident table from a 32-byte message to its 68 Miller line events:
//! a batch verification whose messages were verified before skips hash_to_G2 and line generation
//! for them.  Off until `msgcache_configure(slots)`; 19 584 bytes per slot per device.  Verdicts are
//! what they are without the cache.  Engine errors are values (`EngineError`), as in `lib.rs`.

use crate::{ffi_msgcache, status, EngineError, EngineResult};

pub use crate::ffi_msgcache::GBLS_MSGCACHE_MAX_SLOTS as MAX_SLOTS;

/// `gbls_msgcache_stats`: counters since the process started, and the entries now.
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct MsgCacheStats {
    pub lookups: u64,
    pub hits: u64,
    pub misses: u64,
    pub published: u64,
    pub evictions: u64,
    /// messages computed but not cached: no spare slot, or a sliced submission
    pub bypassed: u64,
    pub entries: u64,
}

/// Sets the capacity in entries per engine device; 0 switches the cache off (the default).
pub fn msgcache_configure(slots: usize) -> EngineResult<()> {
    if slots > MAX_SLOTS {
        return Err(EngineError::Argument);
    }
    // SAFETY: a scalar argument; the library guards its tables with its own lock.
    let rc = unsafe { ffi_msgcache::gbls_msgcache_configure(slots) };
    status(rc)
}

/// The configured capacity per device.
#[must_use]
pub fn msgcache_slots() -> usize {
    // SAFETY: no arguments; the library guards its configuration with its own lock.
    unsafe { ffi_msgcache::gbls_msgcache_slots() }
}

/// Drops every entry and keeps the capacity.
pub fn msgcache_clear() -> EngineResult<()> {
    // SAFETY: no arguments; the library guards its tables with its own lock.
    let rc = unsafe { ffi_msgcache::gbls_msgcache_clear() };
    status(rc)
}

/// Reads the counters.
pub fn msgcache_stats() -> EngineResult<MsgCacheStats> {
    let mut out = [0u64; 8];
    // SAFETY: `out` is a live array of the eight values the call writes.
    let rc = unsafe { ffi_msgcache::gbls_msgcache_stats(out.as_mut_ptr()) };
    status(rc)?;
    Ok(MsgCacheStats {
        lookups: out[0],
        hits: out[1],
        misses: out[2],
        published: out[3],
        evictions: out[4],
        bypassed: out[5],
        entries: out[6],
    })
}
