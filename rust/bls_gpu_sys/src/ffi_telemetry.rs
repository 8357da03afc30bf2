//! Raw bindings of `include/grandine_bls_gpu_telemetry.h`: engine telemetry -- per-call phases,
//! merge sizes, a trace of the most recent shards and the memory the engine holds.
//!
//! The header's prototypes and structs are declared here with the same names, field order and
//! meaning (`tests/test_telemetry_abi.py` parses both files and checks them against each other).
//! Every struct starts with `size`: the caller passes the size of ITS struct, the library fills at
//! most that many bytes and stores how many it filled.

use core::ffi::{c_char, c_int};

pub const GBLS_TELEMETRY_CLASSES: usize = 2;
pub const GBLS_TELEMETRY_KINDS: usize = 9;
pub const GBLS_TELEMETRY_PHASES: usize = 13;
pub const GBLS_TELEMETRY_CALLER_PHASES: usize = 5;
pub const GBLS_TELEMETRY_BUCKETS: usize = 32;
pub const GBLS_TELEMETRY_BINS: usize = 24;
pub const GBLS_TELEMETRY_TRACE_CAPACITY: usize = 1024;
pub const GBLS_TELEMETRY_MAX_ENGINES: usize = 16;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct gbls_telemetry_hist {
    pub count: u64,
    pub sum_ns: u64,
    pub max_ns: u64,
    pub bucket: [u64; GBLS_TELEMETRY_BUCKETS],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct gbls_telemetry_cell {
    pub calls: u64,
    pub sets: u64,
    pub rejected: u64,
    pub engine_errors: u64,
    pub submissions: u64,
    pub shards: u64,
    pub callers: u64,
    pub submitted_sets: u64,
    pub fresh_contexts: u64,
    pub staging_waits: u64,
    pub growths: u64,
    pub reserved: u64,
    pub callers_bin: [u64; GBLS_TELEMETRY_BINS],
    pub sets_bin: [u64; GBLS_TELEMETRY_BINS],
    pub phase: [gbls_telemetry_hist; GBLS_TELEMETRY_PHASES],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct gbls_telemetry_snapshot {
    pub size: u32,
    pub level: u32,
    pub trace_written: u64,
    pub trace_dropped: u64,
    pub cell: [[gbls_telemetry_cell; GBLS_TELEMETRY_KINDS]; GBLS_TELEMETRY_CLASSES],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct gbls_telemetry_record {
    pub id: u64,
    pub submission: u64,
    pub cls: u32,
    pub kind: u32,
    pub callers: u32,
    pub segments: u32,
    pub sets: u64,
    pub shard_sets: u64,
    pub engine: u32,
    pub fresh: u32,
    pub context: u64,
    pub first_arrival_ns: u64,
    pub lead_ns: u64,
    pub lease_ns: u64,
    pub first_event_ns: u64,
    pub enqueued_ns: u64,
    pub synced_ns: u64,
    pub staging_wait_ns: u64,
    pub staging_waits: u32,
    pub growths: u32,
    pub device_ns: u64,
    pub lag_ns: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct gbls_telemetry_engine_memory {
    pub hip_device: u32,
    pub reserved: u32,
    pub contexts_leased: [u64; GBLS_TELEMETRY_CLASSES],
    pub contexts_idle: [u64; GBLS_TELEMETRY_CLASSES],
    pub workspace_bytes: [u64; GBLS_TELEMETRY_CLASSES],
    pub registry_bytes: u64,
    pub committee_bytes: u64,
    pub member_bytes: u64,
    pub linecache_bytes: u64,
    pub pinned_live_bytes: u64,
    pub pinned_retired_bytes: u64,
    pub pinned_retired_buffers: u64,
    pub device_free_bytes: u64,
    pub device_total_bytes: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct gbls_telemetry_memory_info {
    pub size: u32,
    pub engines: u32,
    pub engine: [gbls_telemetry_engine_memory; GBLS_TELEMETRY_MAX_ENGINES],
}

extern "C" {
    pub fn gbls_telemetry_enable(level: c_int) -> c_int;
    pub fn gbls_telemetry_read(out: *mut gbls_telemetry_snapshot, size: usize) -> c_int;
    pub fn gbls_telemetry_reset();
    pub fn gbls_telemetry_trace(records: *mut gbls_telemetry_record, max: usize, dropped: *mut u64) -> usize;
    pub fn gbls_telemetry_memory(out: *mut gbls_telemetry_memory_info, size: usize) -> c_int;
    pub fn gbls_telemetry_phase_name(i: c_int) -> *const c_char;
    pub fn gbls_telemetry_kind_name(i: c_int) -> *const c_char;
    pub fn gbls_telemetry_class_name(i: c_int) -> *const c_char;
}
