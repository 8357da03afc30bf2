//! Raw bindings of `include/grandine_bls_gpu_msgcache.h`: the message line cache.
//!
//! Every prototype of that header is declared here with the same name, argument order and meaning
//! (`tests/test_msgcache_abi.py` parses both files and checks them against each other).  The
//! conventions of `ffi.rs` hold: a failure is `GBLS_VERIFY_FAIL` with `gbls_last_error()` set.
//! None of the four needs a device.

use core::ffi::c_int;

/// The largest capacity `gbls_msgcache_configure` accepts.
pub const GBLS_MSGCACHE_MAX_SLOTS: usize = 1 << 20;

extern "C" {
    pub fn gbls_msgcache_configure(slots: usize) -> c_int;
    pub fn gbls_msgcache_slots() -> usize;
    pub fn gbls_msgcache_clear() -> c_int;
    pub fn gbls_msgcache_stats(out: *mut u64) -> c_int;
}
