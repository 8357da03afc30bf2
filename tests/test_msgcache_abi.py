"""CPU: the boundary of the message line cache (include/grandine_bls_gpu_msgcache.h).

* the header's four prototypes agree in argument count and types with
  rust/bls_gpu_sys/src/ffi_msgcache.rs, and in names with grandine_amd/_lib.EXPORTS_MSGCACHE; the
  main header and _lib.EXPORTS stay as they are;
* the built library exports all four;
* tests/native/abi_msgcache_c99.c includes the header in a -std=c99 -Wall -Wextra -Werror -pedantic
  translation unit and calls every entry; without a GPU configure, clear and stats succeed with
  zero counters and a verification call still fails closed with GBLS_ERR_NO_DEVICE;
* every `unsafe` block of rust/bls_gpu_sys/src/msgcache.rs carries a SAFETY note and no safe
  signature takes a raw pointer.
"""
import os
import re
import subprocess

import pytest

from grandine_amd import _lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "grandine_bls_gpu_msgcache.h")
MAIN_HDR = os.path.join(ROOT, "include", "grandine_bls_gpu.h")
SRC = os.path.join(ROOT, "rust", "bls_gpu_sys", "src")
LIBDIR = os.path.join(ROOT, "grandine_amd", "lib")

NAMES = ["gbls_msgcache_clear", "gbls_msgcache_configure", "gbls_msgcache_slots", "gbls_msgcache_stats"]
SCALAR = {"size_t": "usize", "int": "c_int", "uint64_t": "u64"}


def c_type(arg):
    m = re.match(r"(\w+)\s+\w+\[(\d+)\]$", arg)  # uint64_t out[8]: a pointer to the first of 8
    if m:
        return "*mut " + SCALAR[m.group(1)]
    m = re.match(r"(\w+)\s+\w+$", arg)
    assert m, arg
    return SCALAR[m.group(1)]


def c_prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^([a-z][\w \*]*?\b)(gbls_\w+)\s*\(([^;]*?)\);", txt, flags=re.M | re.S):
        args = " ".join(args.split())
        out[name] = (SCALAR[ret.strip()], [] if args == "void" else [c_type(a.strip()) for a in args.split(",")])
    return out


def rust_prototypes():
    txt = open(os.path.join(SRC, "ffi_msgcache.rs")).read()
    block = txt[txt.index('extern "C" {'):]
    out = {}
    for name, args, ret in re.findall(r"pub fn (gbls_\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", block, flags=re.S):
        args = " ".join(args.split()).rstrip(",")
        out[name] = (ret.strip() if ret else None, [a.split(":", 1)[1].strip() for a in args.split(",") if a.strip()])
    return out


def test_header_rust_and_python_agree():
    c, r = c_prototypes(), rust_prototypes()
    assert sorted(c) == NAMES
    assert sorted(r) == NAMES
    for name in NAMES:
        assert c[name] == r[name], (name, c[name], r[name])
    assert c["gbls_msgcache_configure"] == ("c_int", ["usize"]) and c["gbls_msgcache_stats"] == ("c_int", ["*mut u64"])
    assert c["gbls_msgcache_slots"] == ("usize", []) and c["gbls_msgcache_clear"] == ("c_int", [])
    assert sorted(G.EXPORTS_MSGCACHE) == NAMES
    assert not set(G.EXPORTS) & set(NAMES) and not set(G.EXPORTS_COMMITTEES) & set(NAMES)
    assert len(G.MSGCACHE_STATS) == 8 and G.MSGCACHE_STATS[-1] == "reserved"
    rs = open(os.path.join(SRC, "ffi_msgcache.rs")).read()
    assert re.search(r"pub const GBLS_MSGCACHE_MAX_SLOTS: usize = 1 << 20;", rs)


def test_header_states_cost_scope_and_grouping():
    txt = " ".join(open(HDR).read().split())
    assert "19 584 bytes per slot" in txt.replace("* ", "") and "80 MB" in txt
    for phrase in ("_device entry points", "single checks", "event slices", "always planned by message", "2^20"):
        assert phrase in txt.replace("* ", ""), phrase


def test_main_header_declares_none_of_them():
    main = open(MAIN_HDR).read()
    assert "msgcache" not in main
    assert '#include "grandine_bls_gpu.h"' in open(HDR).read()


def test_library_exports_every_symbol():
    L = G.load_library()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(c_prototypes()[name][1]), name
    assert L.gbls_msgcache_slots.restype is G._sz


def test_lib_rs_declares_the_modules():
    lib = open(os.path.join(SRC, "lib.rs")).read()
    assert re.search(r"^pub mod msgcache;$", lib, flags=re.M) and re.search(r"^pub mod ffi_msgcache;$", lib, flags=re.M)


def test_safe_wrappers():
    txt = open(os.path.join(SRC, "msgcache.rs")).read()
    assert txt.count("unsafe {") == txt.count("// SAFETY:") == 4
    sigs = re.findall(r"\bpub fn (\w+)\s*\(([^{]*?)\{", txt, flags=re.S)
    assert sorted(n for n, _ in sigs) == ["msgcache_clear", "msgcache_configure", "msgcache_slots", "msgcache_stats"]
    for name, sig in sigs:
        assert "*const" not in sig and "*mut" not in sig, name
    for name in NAMES:  # each entry is called once
        assert len(re.findall(r"ffi_msgcache::%s\(" % name, txt)) == 1, name
    for name in ("msgcache_configure", "msgcache_clear", "msgcache_stats"):
        assert "status(rc)" in txt.split("pub fn %s(" % name, 1)[1].split("\npub fn ", 1)[0], name
    assert "EngineError::Argument" in txt.split("pub fn msgcache_configure(", 1)[1].split("\npub fn ", 1)[0]


@pytest.fixture(scope="module")
def c99_run(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgrandine_bls.so")), "library not built"
    exe = str(tmp_path_factory.mktemp("abi") / "abi_msgcache_c99")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "abi_msgcache_c99.c"),
                           "-L", LIBDIR, "-lgrandine_bls", "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def test_c99_consumer_calls_every_entry(c99_run):
    assert set(NAMES) <= set(c99_run)
    # the four need no device: the same answers with and without one
    assert c99_run["slots_default"] == ["0"]
    assert c99_run["too_many"] == ["5", "102"]  # GBLS_VERIFY_FAIL, GBLS_ERR_ARG
    assert c99_run["gbls_msgcache_configure"] == ["0", "0"] and c99_run["gbls_msgcache_slots"] == ["4096"]
    assert c99_run["gbls_msgcache_clear"] == ["0", "0"] and c99_run["gbls_msgcache_stats"] == ["0", "0"]
    assert c99_run["off_again"] == ["0", "0"] and c99_run["slots_off"] == ["0"]
    assert c99_run["stats"][6:] == ["0", "0"]  # nothing verified: no entries; reserved is 0


def test_c99_consumer_without_device(c99_run):
    if c99_run["gbls_init"][0] == "0":
        pytest.skip("a device is present: the fail-closed leg is for GPU-less hosts")
    assert c99_run["gbls_multi_verify"] == ["5", "100"]  # GBLS_VERIFY_FAIL, GBLS_ERR_NO_DEVICE
    assert c99_run["stats"] == ["0"] * 8
