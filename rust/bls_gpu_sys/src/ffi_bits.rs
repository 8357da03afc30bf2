//! Raw bindings of `include/grandine_bls_gpu_bits.h`: aggregation-bit sets over resident committee
//! members.
//!
//! Every prototype of that header is declared here with the same name, argument order and meaning
//! (`tests/test_bits_abi.py` parses both files and checks them against each other).  The
//! conventions of `ffi.rs` hold: status codes mirror `BLST_ERROR`, any device or driver failure is
//! fail-closed (`GBLS_VERIFY_FAIL`, `gbls_last_error()` set).

use core::ffi::c_int;

use crate::ffi::gbls_p1_affine;

extern "C" {
    pub fn gbls_committees_set_members(
        first: usize,
        idx: *const u32,
        off: *const u32,
        ncom: usize,
        status: *mut i32,
    ) -> c_int;
    pub fn gbls_committees_members(slot: usize) -> usize;
    pub fn gbls_g1_aggregate_bits(
        com: *const u32,
        bits: *const u8,
        bits_off: *const u32,
        pk_idx: *const u32,
        pk_off: *const u32,
        n: usize,
        out: *mut gbls_p1_affine,
        status: *mut i32,
    ) -> c_int;
    pub fn gbls_multi_verify_bits(
        msgs: *const [u8; 32],
        sigs: *const [u8; 96],
        com: *const u32,
        bits: *const u8,
        bits_off: *const u32,
        pk_idx: *const u32,
        pk_off: *const u32,
        rands: *const u64,
        n: usize,
        sig_status: *mut i32,
        call_flags: u32,
    ) -> c_int;
}
