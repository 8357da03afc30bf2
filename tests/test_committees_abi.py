"""CPU: the boundary of the cached committee key sums (include/grandine_bls_gpu_committees.h).

* the header's five prototypes and its constant agree in argument count and types with
  rust/bls_gpu_sys/src/ffi_committees.rs, and in names with grandine_amd/_lib.EXPORTS_COMMITTEES;
  the main header and _lib.EXPORTS stay as they are;
* the built library exports all five;
* tests/native/abi_committees_c99.c includes the header in a -std=c99 -Wall -Wextra -Werror
  -pedantic translation unit and calls every entry; without a GPU every call fails closed
  (GBLS_VERIFY_FAIL, GBLS_ERR_NO_DEVICE, failure-filled outputs, size 0);
* every `unsafe` block of rust/bls_gpu_sys/src/committees.rs carries a SAFETY note and no safe
  signature takes a raw pointer.
"""
import os
import re
import subprocess

import pytest

from grandine_amd import _lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "grandine_bls_gpu_committees.h")
MAIN_HDR = os.path.join(ROOT, "include", "grandine_bls_gpu.h")
SRC = os.path.join(ROOT, "rust", "bls_gpu_sys", "src")
LIBDIR = os.path.join(ROOT, "grandine_amd", "lib")

NAMES = ["gbls_committees_clear", "gbls_committees_set", "gbls_committees_size", "gbls_g1_aggregate_committees",
         "gbls_multi_verify_committees"]
SCALAR = {"size_t": "usize", "int": "c_int", "uint32_t": "u32", "int32_t": "i32", "uint64_t": "u64",
          "uint8_t": "u8", "gbls_p1_affine": "gbls_p1_affine"}


def split_args(args):
    parts, depth, cur = [], 0, ""
    for ch in args:
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return parts + [cur.strip()]


def c_type(arg):
    m = re.match(r"(const\s+)?(\w+)\s*\(\*\s*\w+\)\[(\d+)\]$", arg)  # const uint8_t (*msgs)[32]
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
        out[name] = (SCALAR[ret.strip()], [] if args == "void" else [c_type(a) for a in split_args(args)])
    return out


def rust_prototypes():
    txt = open(os.path.join(SRC, "ffi_committees.rs")).read()
    block = txt[txt.index('extern "C" {'):]
    out = {}
    for name, args, ret in re.findall(r"pub fn (gbls_\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", block, flags=re.S):
        args = " ".join(args.split()).rstrip(",")
        types = [a.split(":", 1)[1].strip() for a in split_args(args) if a] if args.strip() else []
        out[name] = (ret.strip() if ret else None, types)
    return out


def test_header_rust_and_python_agree():
    c, r = c_prototypes(), rust_prototypes()
    assert sorted(c) == NAMES
    assert sorted(r) == NAMES
    for name in NAMES:
        assert c[name] == r[name], (name, c[name], r[name])
    assert sorted(G.EXPORTS_COMMITTEES) == NAMES
    assert not set(G.EXPORTS) & set(NAMES)
    assert c["gbls_multi_verify_committees"][1][-1] == "u32" and len(c["gbls_multi_verify_committees"][1]) == 9


def test_constant_agrees():
    m = re.search(r"#define GBLS_NO_COMMITTEE (0x[0-9a-f]+)u", open(HDR).read())
    r = re.search(r"pub const GBLS_NO_COMMITTEE: u32 = (0x[0-9a-f]+);", open(os.path.join(SRC, "ffi_committees.rs")).read())
    assert m and r
    assert int(m.group(1), 16) == int(r.group(1), 16) == G.NO_COMMITTEE == 0xFFFFFFFF


def test_main_header_declares_none_of_them():
    """The main header's prototype set is pinned one-to-one to three other files; the new entries
    live in their own header, which includes it."""
    main = open(MAIN_HDR).read()
    assert not any(n in main for n in NAMES) and "GBLS_NO_COMMITTEE" not in main
    assert '#include "grandine_bls_gpu.h"' in open(HDR).read()


def test_library_exports_every_symbol():
    L = G.load_library()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(c_prototypes()[name][1]), name
    assert L.gbls_committees_size.restype is G._sz


def test_lib_rs_declares_the_modules():
    lib = open(os.path.join(SRC, "lib.rs")).read()
    assert re.search(r"^pub mod committees;$", lib, flags=re.M) and re.search(r"^pub mod ffi_committees;$", lib, flags=re.M)


def test_safe_wrappers():
    txt = open(os.path.join(SRC, "committees.rs")).read()
    assert txt.count("unsafe {") == txt.count("// SAFETY:") == 5
    sigs = re.findall(r"\bpub fn (\w+)\s*\(([^{]*?)\{", txt, flags=re.S)
    assert sorted(n for n, _ in sigs) == ["committees_clear", "committees_set", "committees_size",
                                          "g1_aggregate_committees", "multi_verify_committees"]
    for name, sig in sigs:
        assert "*const" not in sig and "*mut" not in sig, name
    c = c_prototypes()
    for name in NAMES:  # each entry is called once, with the header's argument count
        m = re.search(r"ffi_committees::%s\((.*?)\)\s*\}?;?\n" % name, txt, flags=re.S)
        assert m, name
        args = [a for a in split_args(" ".join(m.group(1).split()).rstrip(",")) if a.strip()]
        assert len(args) == len(c[name][1]), (name, args)
    # slices are validated and engine errors read back
    for name in ("committees_set", "g1_aggregate_committees", "multi_verify_committees"):
        body = txt.split("pub fn %s(" % name, 1)[1].split("\npub fn ", 1)[0]
        assert "ranges_ok(" in body and "EngineError::Argument" in body, name
        assert "status(rc)" in body or "last_error()" in body, name
    assert "status(rc)" in txt.split("pub fn committees_clear(", 1)[1]


@pytest.fixture(scope="module")
def c99_run(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgrandine_bls.so")), "library not built"
    exe = str(tmp_path_factory.mktemp("abi") / "abi_committees_c99")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "abi_committees_c99.c"),
                           "-L", LIBDIR, "-lgrandine_bls", "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def test_c99_consumer_calls_every_entry(c99_run):
    assert set(NAMES) <= set(c99_run)


def test_c99_consumer_fails_closed_without_device(c99_run):
    if c99_run["gbls_init"][0] == "0":
        pytest.skip("a device is present: the fail-closed leg is for GPU-less hosts")
    for name in NAMES:
        if name != "gbls_committees_size":
            assert c99_run[name] == ["5", "100"], (name, c99_run[name])  # GBLS_VERIFY_FAIL, GBLS_ERR_NO_DEVICE
    assert c99_run["gbls_committees_size"] == ["0"]
    assert c99_run["set_status"] == ["1"] and c99_run["key_status"] == ["1"] and c99_run["sig_status"] == ["1"]
    assert c99_run["key_zero"] == ["1"]
