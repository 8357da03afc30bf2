//! Raw bindings of `include/grandine_bls_gpu_msgcache_checks.h`: the message line cache for
//! per-check calls, and prefetch.
//!
//! Every prototype of that header is declared here with the same name, argument order and meaning
//! (`tests/test_msgcache_checks_abi.py` parses both files and checks them against each other).  The
//! conventions of `ffi.rs` hold: a failure is `GBLS_VERIFY_FAIL` with `gbls_last_error()` set.
//! `gbls_msgcache_serve_checks` and `gbls_msgcache_checks_stats` need no device;
//! `gbls_msgcache_prefetch` needs the engine unless the cache is off.

use core::ffi::c_int;

/// Entered by this call.
pub const GBLS_PREFETCH_ENTERED: i32 = 0;
/// Was an entry already (its recency is refreshed).
pub const GBLS_PREFETCH_PRESENT: i32 = 1;
/// Not entered: cache off, no spare slot, no evictable entry.
pub const GBLS_PREFETCH_SKIPPED: i32 = 2;

extern "C" {
    pub fn gbls_msgcache_prefetch(msgs: *const [u8; 32], n: usize, status: *mut i32) -> c_int;
    pub fn gbls_msgcache_serve_checks(on: c_int) -> c_int;
    pub fn gbls_msgcache_checks_stats(out: *mut u64) -> c_int;
}
