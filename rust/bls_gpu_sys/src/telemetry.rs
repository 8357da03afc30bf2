//! Safe wrappers of `include/grandine_bls_gpu_telemetry.h`: engine telemetry.
//!
//! What the engine did with each call: how long it was held behind a block import, sat in a
//! collection window, queued for a leader, waited for a context, a staging slot, the device; how
//! many callers and sets each submission carried; how much device and pinned memory the engine
//! holds.  Off (level 0) by default; `engine()` switches it on when `GBLS_TELEMETRY` is 1 or 2.
//! A node's metrics service reads [`snapshot`] and [`memory`] when it is scraped, beside
//! `bls::gpu::cpu_fallbacks()`; the phases refine the attestation verifier's batch-time histograms.
//! None of these needs a device.  Engine errors are values (`EngineError`), as in `lib.rs`.

use core::ffi::{c_int, CStr};

use crate::{ffi_telemetry, status, EngineResult};

pub use crate::ffi_telemetry::{
    gbls_telemetry_cell as Cell, gbls_telemetry_engine_memory as EngineMemory, gbls_telemetry_hist as Hist,
    gbls_telemetry_record as Record, gbls_telemetry_snapshot as Snapshot, GBLS_TELEMETRY_TRACE_CAPACITY as TRACE_CAPACITY,
};

/// What is recorded: nothing, counters and host-clock phases, or device time per shard as well.
#[derive(Clone, Copy, Debug, PartialEq, Eq, PartialOrd, Ord)]
pub enum Level {
    Off = 0,
    Phases = 1,
    DeviceTime = 2,
}

impl Level {
    fn from_raw(raw: c_int) -> Self {
        match raw {
            i32::MIN..=0 => Self::Off,
            1 => Self::Phases,
            _ => Self::DeviceTime,
        }
    }
}

/// Sets the level (process-wide, sticky) and returns the previous one.
pub fn enable(level: Level) -> Level {
    // SAFETY: a plain integer in and out; the level is one atomic in the library.
    let prev = unsafe { ffi_telemetry::gbls_telemetry_enable(level as c_int) };
    Level::from_raw(prev)
}

/// The level named by the environment variable `GBLS_TELEMETRY` (1 or 2), if any.
#[must_use]
pub fn level_from_env() -> Option<Level> {
    match std::env::var("GBLS_TELEMETRY").ok()?.trim() {
        "1" => Some(Level::Phases),
        "2" => Some(Level::DeviceTime),
        _ => None,
    }
}

/// Every counter and histogram, per class and kind (boxed: 72 KiB).
pub fn snapshot() -> EngineResult<Box<Snapshot>> {
    let mut out = Box::<Snapshot>::default();
    // SAFETY: `out` is a live, exclusively borrowed struct of exactly the size passed.
    let rc = unsafe { ffi_telemetry::gbls_telemetry_read(&mut *out, core::mem::size_of::<Snapshot>()) };
    status(rc)?;
    Ok(out)
}

/// Zeroes the counters and histograms and empties the trace.
pub fn reset() {
    // SAFETY: no arguments; the counters are atomics in the library.
    unsafe { ffi_telemetry::gbls_telemetry_reset() }
}

/// Drains the trace: the unread shard records, oldest first (at most `TRACE_CAPACITY`), and the
/// number of records lost since the previous drain.
#[must_use]
pub fn trace() -> (Vec<Record>, u64) {
    let mut records = vec![Record::default(); TRACE_CAPACITY];
    let mut dropped = 0u64;
    // SAFETY: `records` holds `records.len()` live elements and `dropped` is a live u64; the call
    // writes at most that many records and returns how many.
    let n = unsafe { ffi_telemetry::gbls_telemetry_trace(records.as_mut_ptr(), records.len(), &mut dropped) };
    records.truncate(n.min(TRACE_CAPACITY));
    (records, dropped)
}

/// The memory gauges of every engine device, computed now; empty before the engine is open.
pub fn memory() -> EngineResult<Vec<EngineMemory>> {
    let mut out = Box::<ffi_telemetry::gbls_telemetry_memory_info>::default();
    let size = core::mem::size_of::<ffi_telemetry::gbls_telemetry_memory_info>();
    // SAFETY: `out` is a live, exclusively borrowed struct of exactly the size passed.
    let rc = unsafe { ffi_telemetry::gbls_telemetry_memory(&mut *out, size) };
    status(rc)?;
    let engines = (out.engines as usize).min(out.engine.len());
    Ok(out.engine[..engines].to_vec())
}

fn names(name: unsafe extern "C" fn(c_int) -> *const core::ffi::c_char) -> Vec<&'static str> {
    let mut out = Vec::new();
    for i in 0.. {
        // SAFETY: the name functions take any index and return NULL past the end, else a pointer
        // to a NUL-terminated string constant of the library, which lives as long as the process.
        let s = unsafe {
            let p = name(i);
            if p.is_null() {
                break;
            }
            CStr::from_ptr(p)
        };
        out.push(s.to_str().unwrap_or(""));
    }
    out
}

/// The names of the phases, in the order of `Cell::phase`.
#[must_use]
pub fn phase_names() -> Vec<&'static str> {
    names(ffi_telemetry::gbls_telemetry_phase_name)
}

/// The names of the kinds, in the order of `Snapshot::cell[class]`.
#[must_use]
pub fn kind_names() -> Vec<&'static str> {
    names(ffi_telemetry::gbls_telemetry_kind_name)
}

/// The names of the classes, in the order of `Snapshot::cell`.
#[must_use]
pub fn class_names() -> Vec<&'static str> {
    names(ffi_telemetry::gbls_telemetry_class_name)
}
