"""CPU: the boundary of the local key set calls (include/grandine_bls_gpu_local.h).

* the header's three prototypes agree in argument count and types with
  rust/bls_gpu_sys/src/ffi_local.rs, and in names with grandine_amd/_lib.EXPORTS_LOCAL; no other
  header and no other export list holds the names; the value of GBLS_LOCAL_KEYS is the same in the
  header, the Rust text, the Python layer and the engine's own header;
* the built library exports all three, with the header's argument counts;
* tests/native/abi_local_c99.c includes the header in a -std=c99 -Wall -Wextra -Werror -pedantic
  translation unit and calls all three; without a GPU every call fails closed (GBLS_VERIFY_FAIL,
  GBLS_ERR_NO_DEVICE, verdicts at GBLS_VERIFY_FAIL, keys all-zero, every status array -- the
  table's too -- at GBLS_BAD_ENCODING);
* every `unsafe` block of rust/bls_gpu_sys/src/local.rs carries a SAFETY note, no safe signature
  takes a raw pointer, and every wrapper validates its ranges.
"""
import os
import re
import subprocess

import pytest

from grandine_amd import _lib as G

import test_each_abi as A

ROOT = A.ROOT
INC, SRC, LIBDIR = A.INC, A.SRC, A.LIBDIR
HDR = os.path.join(INC, "grandine_bls_gpu_local.h")

NAMES = ["gbls_g1_aggregate_local", "gbls_verify_each_local", "gbls_verify_items_local"]
KEYSRC = ["*const u32", "*const [u8; 8]", "*const u8", "*const u32", "*const u32", "*const u32", "*const [u8; 48]", "usize"]
SETS = ["*const [u8; 32]", "*const [u8; 96]"] + KEYSRC
OUTS = ["*mut i32", "*mut i32", "*mut i32", "*mut i32"]
SCALAR = dict(A.SCALAR, gbls_p1_affine="gbls_p1_affine")


def c_type(arg):
    m = re.match(r"(const\s+)?(\w+)\s*\(\*\s*\w+\)\[(\d+)\]$", arg)
    if m:
        return "*%s [%s; %s]" % ("const" if m.group(1) else "mut", SCALAR[m.group(2)], m.group(3))
    m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*\w+$", arg)
    assert m, arg
    return ("*%s " % ("const" if m.group(1) else "mut") if m.group(3) else "") + SCALAR[m.group(2)]


def c_prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^([a-z][\w \*]*?\b)(gbls_\w+)\s*\(([^;]*?)\);", txt, flags=re.M | re.S):
        args = " ".join(args.split())
        out[name] = (SCALAR[ret.strip()], [c_type(a) for a in A.split_args(args)])
    return out


def rust_prototypes():
    txt = open(os.path.join(SRC, "ffi_local.rs")).read()
    block = txt[txt.index('extern "C" {'):]
    out = {}
    for name, args, ret in re.findall(r"pub fn (gbls_\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", block, flags=re.S):
        args = " ".join(args.split()).rstrip(",")
        out[name] = (ret.strip() if ret else None, [a.split(":", 1)[1].strip() for a in A.split_args(args) if a])
    return out


def test_header_rust_and_python_agree():
    c, r = c_prototypes(), rust_prototypes()
    assert sorted(c) == NAMES and sorted(r) == NAMES
    for name in NAMES:
        assert c[name] == r[name], (name, c[name], r[name])
    assert sorted(G.EXPORTS_LOCAL) == NAMES
    others = (set(G.EXPORTS) | set(G.EXPORTS_COMMITTEES) | set(G.EXPORTS_MSGCACHE) | set(G.EXPORTS_BITS) |
              set(G.EXPORTS_SPANS) | set(G.EXPORTS_EACH))
    assert not others & set(NAMES)
    assert c["gbls_g1_aggregate_local"] == ("c_int", KEYSRC + ["usize", "*mut gbls_p1_affine", "*mut i32", "*mut i32"])
    assert c["gbls_verify_each_local"] == ("c_int", SETS + ["usize"] + OUTS)
    assert c["gbls_verify_items_local"] == ("c_int", SETS + ["*const u64", "usize", "*const u32", "usize"] + OUTS + ["u32"])


def test_one_value_names_a_local_set():
    hdr = open(HDR).read()
    assert re.search(r"^#define GBLS_LOCAL_KEYS 0xFFFFFFFEu$", hdr, flags=re.M)
    assert "pub const GBLS_LOCAL_KEYS: u32 = 0xFFFF_FFFE;" in open(os.path.join(SRC, "ffi_local.rs")).read()
    assert G.LOCAL_KEYS == 0xFFFFFFFE == G.NO_COMMITTEE - 1
    csrc = os.path.join(ROOT, "grandine_amd", "csrc")
    assert "constexpr uint32_t kLocalKeys = 0xfffffffeu;" in open(os.path.join(csrc, "gbls_local.h")).read()
    assert "constexpr uint32_t kLocalSet = 0xfffffffeu;" in open(os.path.join(csrc, "gbls_sched.h")).read()
    # the switch between the decode kernel's two forms is a named constant the GPU tests read
    assert re.search(r"^constexpr uint32_t kLocalWaveMax = \d+;", open(os.path.join(csrc, "gbls_local.h")).read(), flags=re.M)


def test_other_headers_declare_none_of_them():
    for other in os.listdir(INC):
        if other != "grandine_bls_gpu_local.h":
            txt = open(os.path.join(INC, other)).read()
            assert not any(n in txt for n in NAMES) and "GBLS_LOCAL_KEYS" not in txt, other
    hdr = open(HDR).read()
    assert '#include "grandine_bls_gpu_each.h"' in hdr
    # the earlier headers' entries are theirs alone: not spelled here, not even in a comment
    assert not any(n in hdr for n in G.EXPORTS_SPANS + G.EXPORTS_BITS + G.EXPORTS_EACH)
    for word in ("pre-fill", "PublicKey::try_from", "decoded once", "GBLS_ERR_ARG", "GBLS_AGGR_TYPE_MISMATCH",
                 "GBLS_PK_IS_INFINITY", "GBLS_POINT_NOT_IN_GROUP", "may be\n * NULL", "never changes a neighbour",
                 "does\n * not fit 32 bits", "whole table on every shard"):
        assert word in hdr, word


def test_library_exports_every_symbol():
    L = G.load_library()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(c_prototypes()[name][1]), name


def test_lib_rs_declares_the_modules():
    lib = open(os.path.join(SRC, "lib.rs")).read()
    assert re.search(r"^pub mod local;$", lib, flags=re.M) and re.search(r"^pub mod ffi_local;$", lib, flags=re.M)


def test_safe_wrappers():
    txt = open(os.path.join(SRC, "local.rs")).read()
    assert txt.count("unsafe {") == txt.count("// SAFETY:") == 3
    sigs = re.findall(r"\bpub fn (\w+)\s*\(([^{]*?)\{", txt, flags=re.S)
    assert sorted(n for n, _ in sigs) == ["aggregate_local", "verify_each_local", "verify_items_local"]
    for name, sig in sigs:
        assert "*const" not in sig and "*mut" not in sig, name
    assert "*const" not in txt and "*mut" not in txt
    c = c_prototypes()
    for name in NAMES:  # each entry is called once, with the header's argument count
        assert txt.count("ffi_local::%s(" % name) == 1, name
        m = re.search(r"ffi_local::%s\((.*?)\)\s*\}?;?\n" % name, txt, flags=re.S)
        assert m, name
        args = [a for a in A.split_args(" ".join(m.group(1).split()).rstrip(",")) if a.strip()]
        assert len(args) == len(c[name][1]), (name, args)
    for name in ("aggregate_local", "verify_each_local", "verify_items_local"):
        body = txt.split("pub fn %s(" % name, 1)[1].split("\npub fn ", 1)[0]
        assert "sets_ok(" in body and "EngineError::Argument" in body and "status(rc)" in body, name
        assert "keys.len()" in body and "GBLS_BAD_ENCODING; keys.len()]" in body, name   # the table's statuses
    assert "u32::try_from(keys.len()).is_ok()" in txt and "s == NO_COMMITTEE || s == LOCAL_KEYS" in txt
    body = txt.split("pub fn verify_items_local(", 1)[1]
    assert "ranges_ok(messages, item_offsets" in body and "scalars.contains(&0)" in body
    # the patched bodies stay unwired
    patch = os.path.join(ROOT, "rust", "bls_patch")
    for dirpath, _, files in os.walk(patch):
        for f in files:
            assert "local::" not in open(os.path.join(dirpath, f), errors="replace").read(), f


@pytest.fixture(scope="module")
def c99_run(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgrandine_bls.so")), "library not built"
    exe = str(tmp_path_factory.mktemp("abi") / "abi_local_c99")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC,
                           os.path.join(ROOT, "tests", "native", "abi_local_c99.c"),
                           "-L", LIBDIR, "-lgrandine_bls", "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def test_c99_consumer_calls_every_entry(c99_run):
    assert set(NAMES) <= set(c99_run)


def test_c99_consumer_fails_closed(c99_run):
    """Without a device: GBLS_VERIFY_FAIL with GBLS_ERR_NO_DEVICE and the pre-fill.  With one: the
    registry and the committee table are empty and the table's all-zero keys do not decode, so every
    key is rejected, the all-zero signatures do not decode, and every verdict is GBLS_VERIFY_FAIL in
    a call that succeeds."""
    device = c99_run["gbls_init"][0] == "0"
    for name in NAMES:
        assert c99_run[name] == (["0", "0"] if device else ["5", "100"]), (name, c99_run[name])
    assert c99_run["keys_status"] == ["1", "1", "1"] and c99_run["keys_nonzero_bytes"] == ["0"]
    for call in ("keys", "each", "items"):
        assert c99_run[call + "_pkb_status"] == ["1", "1"]
    for call, nv in (("each", 3), ("items", 2)):
        assert c99_run[call + "_verdicts"] == ["5"] * nv
        assert c99_run[call + "_key_status"] == ["1", "1", "1"]
        if device:
            assert "0" not in c99_run[call + "_sig_status"]
        else:
            assert c99_run[call + "_sig_status"] == ["1", "1", "1"]
