//! Raw bindings of `include/grandine_bls_gpu_committees.h`: cached committee key sums.
//!
//! Every prototype of that header is declared here with the same name, argument order and meaning
//! (`tests/test_committees_abi.py` parses both files and checks them against each other).  The
//! conventions of `ffi.rs` hold: status codes mirror `BLST_ERROR`, any device or driver failure is
//! fail-closed (`GBLS_VERIFY_FAIL`, `gbls_last_error()` set).

use core::ffi::c_int;

use crate::ffi::gbls_p1_affine;

/// `com[i]` of a set that names no committee: its key is the plain sum of its index list.
pub const GBLS_NO_COMMITTEE: u32 = 0xffffffff;

extern "C" {
    pub fn gbls_committees_set(
        first: usize,
        idx: *const u32,
        off: *const u32,
        ncom: usize,
        status: *mut i32,
    ) -> c_int;
    pub fn gbls_committees_size() -> usize;
    pub fn gbls_committees_clear() -> c_int;
    pub fn gbls_g1_aggregate_committees(
        com: *const u32,
        pk_idx: *const u32,
        pk_off: *const u32,
        n: usize,
        out: *mut gbls_p1_affine,
        status: *mut i32,
    ) -> c_int;
    pub fn gbls_multi_verify_committees(
        msgs: *const [u8; 32],
        sigs: *const [u8; 96],
        com: *const u32,
        pk_idx: *const u32,
        pk_off: *const u32,
        rands: *const u64,
        n: usize,
        sig_status: *mut i32,
        call_flags: u32,
    ) -> c_int;
}
