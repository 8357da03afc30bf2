"""CPU: the boundary of include/grandine_bls_gpu_msgcache_checks.h (per-check calls served by the
message line cache, and prefetch).

* the header's three prototypes agree in argument count and types with
  rust/bls_gpu_sys/src/ffi_msgcache_checks.rs, and in names with
  grandine_amd/_lib.EXPORTS_MSGCACHE_CHECKS; the msgcache header and EXPORTS_MSGCACHE stay as they are;
* the built library exports all three;
* tests/native/abi_msgcache_checks_c99.c includes the header in a -std=c99 -Wall -Wextra -Werror
  -pedantic translation unit and calls every entry; without a GPU serve_checks and checks_stats
  succeed, prefetch with the cache off answers SKIPPED and prefetch with the cache on fails closed
  with GBLS_ERR_NO_DEVICE;
* every `unsafe` block of rust/bls_gpu_sys/src/msgcache_checks.rs carries a SAFETY note and no safe
  signature takes a raw pointer;
* bls.MessageCache's three new methods, with the engine stubbed.
"""
import ctypes
import os
import re
import subprocess

import pytest

from grandine_amd import _lib as G
from grandine_amd import bls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "grandine_bls_gpu_msgcache_checks.h")
BASE_HDR = os.path.join(ROOT, "include", "grandine_bls_gpu_msgcache.h")
SRC = os.path.join(ROOT, "rust", "bls_gpu_sys", "src")
LIBDIR = os.path.join(ROOT, "grandine_amd", "lib")

NAMES = ["gbls_msgcache_checks_stats", "gbls_msgcache_prefetch", "gbls_msgcache_serve_checks"]
SCALAR = {"size_t": "usize", "int": "c_int", "uint64_t": "u64", "int32_t": "i32"}


def c_type(arg):
    m = re.match(r"const uint8_t \(\*\w+\)\[32\]$", arg)  # an array of 32-byte messages
    if m:
        return "*const [u8; 32]"
    m = re.match(r"(\w+)\s+\w+\[(\d+)\]$", arg)  # uint64_t out[4]: a pointer to the first of 4
    if m:
        return "*mut " + SCALAR[m.group(1)]
    m = re.match(r"(\w+) \*\w+$", arg)
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
    txt = open(os.path.join(SRC, "ffi_msgcache_checks.rs")).read()
    block = txt[txt.index('extern "C" {'):]
    out = {}
    for name, args, ret in re.findall(r"pub fn (gbls_\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", block, flags=re.S):
        args = " ".join(args.split()).rstrip(",")
        out[name] = (ret.strip() if ret else None, [a.split(":", 1)[1].strip() for a in args.split(",") if a.strip()])
    return out


def test_header_rust_and_python_agree():
    c, r = c_prototypes(), rust_prototypes()
    assert sorted(c) == NAMES and sorted(r) == NAMES
    for name in NAMES:
        assert c[name] == r[name], (name, c[name], r[name])
    assert c["gbls_msgcache_prefetch"] == ("c_int", ["*const [u8; 32]", "usize", "*mut i32"])
    assert c["gbls_msgcache_serve_checks"] == ("c_int", ["c_int"])
    assert c["gbls_msgcache_checks_stats"] == ("c_int", ["*mut u64"])
    assert sorted(G.EXPORTS_MSGCACHE_CHECKS) == NAMES
    assert not set(G.EXPORTS_MSGCACHE) & set(NAMES) and not set(G.EXPORTS) & set(NAMES)
    assert G.MSGCACHE_CHECKS_STATS == ("prefetched", "check_lookups", "check_hits", "check_published")
    hdr, rs = open(HDR).read(), open(os.path.join(SRC, "ffi_msgcache_checks.rs")).read()
    for k, name in enumerate(("ENTERED", "PRESENT", "SKIPPED")):
        assert re.search(r"#define GBLS_PREFETCH_%s %d\b" % (name, k), hdr)
        assert re.search(r"pub const GBLS_PREFETCH_%s: i32 = %d;" % (name, k), rs)
        assert getattr(G, "PREFETCH_" + name) == k


def test_header_states_scope_and_the_callers_duty():
    txt = " ".join(open(HDR).read().replace(" * ", " ").split())
    for phrase in ("THE CALLER VOUCHES FOR THESE ROOTS", "never evicts", "OFF by default", "grouped regime",
                   "_device entry points", "gbls_fast_aggregate_verify_indexed", "not 32 bytes", "bypassed",
                   "normal-class context", "ONCE per submission", "at least 64, at most 4096"):
        assert phrase in txt, phrase
    assert '#include "grandine_bls_gpu_msgcache.h"' in open(HDR).read()
    assert "prefetch" not in open(BASE_HDR).read() and "serve_checks" not in open(BASE_HDR).read()


def test_library_exports_every_symbol():
    L = G.load_library()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(c_prototypes()[name][1]), name


def test_lib_rs_declares_the_modules():
    lib = open(os.path.join(SRC, "lib.rs")).read()
    assert re.search(r"^pub mod msgcache_checks;$", lib, flags=re.M)
    assert re.search(r"^pub mod ffi_msgcache_checks;$", lib, flags=re.M)


def test_safe_wrappers():
    txt = open(os.path.join(SRC, "msgcache_checks.rs")).read()
    assert txt.count("unsafe {") == txt.count("// SAFETY:") == 3
    sigs = re.findall(r"\bpub fn (\w+)\s*\(([^{]*?)\{", txt, flags=re.S)
    assert sorted(n for n, _ in sigs) == ["msgcache_checks_stats", "msgcache_prefetch", "msgcache_serve_checks"]
    for name, sig in sigs:
        assert "*const" not in sig and "*mut" not in sig, name
    assert "msgs: &[[u8; 32]]" in dict(sigs)["msgcache_prefetch"]
    for name in NAMES:  # each entry is called once
        assert len(re.findall(r"ffi_msgcache_checks::%s\(" % name, txt)) == 1, name
    for name in ("msgcache_prefetch", "msgcache_checks_stats"):
        assert "status(rc)" in txt.split("pub fn %s(" % name, 1)[1].split("\npub fn ", 1)[0], name
    assert "vouches" in txt


@pytest.fixture(scope="module")
def c99_run(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgrandine_bls.so")), "library not built"
    exe = str(tmp_path_factory.mktemp("abi") / "abi_msgcache_checks_c99")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "abi_msgcache_checks_c99.c"),
                           "-L", LIBDIR, "-lgrandine_bls", "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def test_c99_consumer_calls_every_entry(c99_run):
    assert set(NAMES) <= set(c99_run)
    # these need no device: the same answers with and without one
    assert c99_run["serve_default"] == ["0", "0"]               # off by default
    assert c99_run["gbls_msgcache_serve_checks"] == ["1", "0"]  # the previous setting
    assert c99_run["serve_off"] == ["0", "0"]
    assert c99_run["prefetch_off"] == ["0", "0"] and c99_run["status_off"] == ["2", "2", "2"]
    assert c99_run["prefetch_none"] == ["0", "0"]
    assert c99_run["prefetch_null"] == ["5", "102"]  # GBLS_VERIFY_FAIL, GBLS_ERR_ARG
    assert c99_run["gbls_msgcache_checks_stats"] == ["0", "0"] and c99_run["stats_null"] == ["5", "102"]
    assert c99_run["constants"] == ["0", "1", "2"]


def test_c99_consumer_without_device(c99_run):
    if c99_run["gbls_init"][0] == "0":
        pytest.skip("a device is present: the fail-closed leg is for GPU-less hosts")
    assert c99_run["gbls_msgcache_prefetch"] == ["5", "100"]  # GBLS_VERIFY_FAIL, GBLS_ERR_NO_DEVICE
    assert c99_run["status_on"] == ["2", "2", "2"] and c99_run["stats"] == ["0"] * 4


def test_without_a_device_through_python():
    L = G.load_library()
    st = (ctypes.c_uint64 * 4)()
    assert L.gbls_msgcache_checks_stats(st) == 0
    prev = L.gbls_msgcache_serve_checks(1)
    assert L.gbls_msgcache_serve_checks(prev) == 1
    status = G.i32_array(2)
    assert L.gbls_msgcache_slots() == 0
    assert L.gbls_msgcache_prefetch(bytes(64), 2, status) == 0 and list(status) == [2, 2]


# ---------------------------------------------------------------- the Python mirror, engine stubbed
class Stub:
    def __init__(self):
        self.calls, self.fail, self.serving = [], None, 0

    def gbls_msgcache_prefetch(self, msgs, n, status):
        self.calls.append(("prefetch", bytes(msgs.raw[:32 * n]), n))
        if self.fail == "prefetch":
            return G.VERIFY_FAIL
        for i in range(n):
            status[i] = i % 3
        return 0

    def gbls_msgcache_serve_checks(self, on):
        self.calls.append(("serve_checks", on))
        prev, self.serving = self.serving, on
        return prev

    def gbls_msgcache_checks_stats(self, out):
        self.calls.append(("checks_stats",))
        if self.fail == "checks_stats":
            return G.VERIFY_FAIL
        for i in range(4):
            out[i] = 20 + i
        return 0

    def gbls_last_error(self):
        return 103


@pytest.fixture()
def stub(monkeypatch):
    s = Stub()
    monkeypatch.setattr(G, "load_library", lambda: s)

    def no_device(*a, **k):
        raise AssertionError("MessageCache must not initialise a device")

    monkeypatch.setattr(G, "lib", lambda *a, **k: s if s.fail else no_device())
    return s


def test_mirror_prefetch(stub):
    roots = [bytes([i]) * 32 for i in range(4)]
    assert bls.MessageCache.prefetch(roots) == [0, 1, 2, 0]
    assert stub.calls == [("prefetch", b"".join(roots), 4)]
    assert bls.MessageCache.prefetch([]) == []
    with pytest.raises(ValueError):
        bls.MessageCache.prefetch([b"short"])
    assert len(stub.calls) == 2
    stub.fail = "prefetch"
    with pytest.raises(G.EngineUnavailable):
        bls.MessageCache.prefetch(roots)


def test_mirror_serve_checks_and_stats(stub):
    assert bls.MessageCache.serve_checks(True) is False and bls.MessageCache.serve_checks(False) is True
    assert stub.calls == [("serve_checks", 1), ("serve_checks", 0)]
    st = bls.MessageCache.checks_stats()
    assert st == {"prefetched": 20, "check_lookups": 21, "check_hits": 22, "check_published": 23}
    assert tuple(st) == G.MSGCACHE_CHECKS_STATS
    stub.fail = "checks_stats"
    with pytest.raises(G.EngineUnavailable):
        bls.MessageCache.checks_stats()
