//! Raw bindings of `include/grandine_bls_gpu_local.h`: local key sets, compressed public keys
//! decoded inside the submission.
//!
//! Every prototype of that header is declared here with the same name, argument order and meaning
//! (`tests/test_local_abi.py` parses both files and checks them against each other).  The
//! conventions of `ffi.rs` hold: status codes mirror `BLST_ERROR`, any device or driver failure is
//! fail-closed (`GBLS_VERIFY_FAIL`, `gbls_last_error()` set).

use core::ffi::c_int;

use crate::ffi::gbls_p1_affine;

/// `com[i]` of a local set: its `pk_off` range holds positions into the call's key table.
pub const GBLS_LOCAL_KEYS: u32 = 0xFFFF_FFFE;

extern "C" {
    pub fn gbls_g1_aggregate_local(
        com: *const u32,
        cbits: *const [u8; 8],
        bits: *const u8,
        bits_off: *const u32,
        pk_idx: *const u32,
        pk_off: *const u32,
        pkb: *const [u8; 48],
        npkb: usize,
        n: usize,
        out: *mut gbls_p1_affine,
        status: *mut i32,
        pkb_status: *mut i32,
    ) -> c_int;
    pub fn gbls_verify_each_local(
        msgs: *const [u8; 32],
        sigs: *const [u8; 96],
        com: *const u32,
        cbits: *const [u8; 8],
        bits: *const u8,
        bits_off: *const u32,
        pk_idx: *const u32,
        pk_off: *const u32,
        pkb: *const [u8; 48],
        npkb: usize,
        n: usize,
        sig_status: *mut i32,
        key_status: *mut i32,
        verdicts: *mut i32,
        pkb_status: *mut i32,
    ) -> c_int;
    pub fn gbls_verify_items_local(
        msgs: *const [u8; 32],
        sigs: *const [u8; 96],
        com: *const u32,
        cbits: *const [u8; 8],
        bits: *const u8,
        bits_off: *const u32,
        pk_idx: *const u32,
        pk_off: *const u32,
        pkb: *const [u8; 48],
        npkb: usize,
        rands: *const u64,
        n: usize,
        seg_off: *const u32,
        nseg: usize,
        sig_status: *mut i32,
        key_status: *mut i32,
        verdicts: *mut i32,
        pkb_status: *mut i32,
        call_flags: u32,
    ) -> c_int;
}
