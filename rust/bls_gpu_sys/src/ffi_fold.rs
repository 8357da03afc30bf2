//! Raw bindings of `include/grandine_bls_gpu_fold.h`: verified folds, the each-call over span sets
//! which also sums, per group of its own sets, the signatures that passed.
//!
//! The header's prototype is declared here with the same name, argument order and meaning
//! (`tests/test_fold_abi.py` parses both files and checks them against each other).  The
//! conventions of `ffi.rs` hold: status codes mirror `BLST_ERROR`, any device or driver failure is
//! fail-closed (`GBLS_VERIFY_FAIL`, `gbls_last_error()` set, every output at its pre-fill).

use core::ffi::c_int;

use crate::ffi::gbls_p2_affine;

extern "C" {
    pub fn gbls_verify_each_fold(
        msgs: *const [u8; 32],
        sigs: *const [u8; 96],
        com: *const u32,
        cbits: *const [u8; 8],
        bits: *const u8,
        bits_off: *const u32,
        pk_idx: *const u32,
        pk_off: *const u32,
        n: usize,
        fold_set: *const u32,
        fold_off: *const u32,
        nfold: usize,
        sig_status: *mut i32,
        key_status: *mut i32,
        verdicts: *mut i32,
        fold_out: *mut gbls_p2_affine,
        fold_bytes: *mut [u8; 96],
        fold_count: *mut u32,
    ) -> c_int;
}
