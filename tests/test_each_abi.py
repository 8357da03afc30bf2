"""CPU: the boundary of the per-set and per-item calls over span sets
(include/grandine_bls_gpu_each.h).

* the header's two prototypes agree in argument count and types with
  rust/bls_gpu_sys/src/ffi_each.rs, and in names with grandine_amd/_lib.EXPORTS_EACH; no other
  header and no other export list holds the names, and the header spells no entry of the spans or
  bits headers;
* the built library exports both;
* tests/native/abi_each_c99.c includes the header in a -std=c99 -Wall -Wextra -Werror -pedantic
  translation unit and calls both; without a GPU every call fails closed (GBLS_VERIFY_FAIL,
  GBLS_ERR_NO_DEVICE, verdicts at GBLS_VERIFY_FAIL, both status arrays at GBLS_BAD_ENCODING);
* every `unsafe` block of rust/bls_gpu_sys/src/each.rs carries a SAFETY note, no safe signature
  takes a raw pointer, and every wrapper validates its ranges.
"""
import os
import re
import subprocess

import pytest

from grandine_amd import _lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HDR = os.path.join(INC, "grandine_bls_gpu_each.h")
SRC = os.path.join(ROOT, "rust", "bls_gpu_sys", "src")
LIBDIR = os.path.join(ROOT, "grandine_amd", "lib")

NAMES = ["gbls_verify_each_spans", "gbls_verify_items_spans"]
SCALAR = {"size_t": "usize", "int": "c_int", "uint32_t": "u32", "int32_t": "i32", "uint64_t": "u64", "uint8_t": "u8"}
SETS = ["*const [u8; 32]", "*const [u8; 96]", "*const u32", "*const [u8; 8]", "*const u8", "*const u32", "*const u32",
        "*const u32"]
OUTS = ["*mut i32", "*mut i32", "*mut i32"]


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
    m = re.match(r"(const\s+)?(\w+)\s*\(\*\s*\w+\)\[(\d+)\]$", arg)  # const uint8_t (*cbits)[8]
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
    txt = open(os.path.join(SRC, "ffi_each.rs")).read()
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
    assert sorted(G.EXPORTS_EACH) == NAMES
    others = (set(G.EXPORTS) | set(G.EXPORTS_COMMITTEES) | set(G.EXPORTS_MSGCACHE) | set(G.EXPORTS_BITS) |
              set(G.EXPORTS_SPANS))
    assert not others & set(NAMES)
    assert c["gbls_verify_each_spans"] == ("c_int", SETS + ["usize"] + OUTS)
    assert c["gbls_verify_items_spans"] == ("c_int", SETS + ["*const u64", "usize", "*const u32", "usize"] + OUTS + ["u32"])


def test_other_headers_declare_none_of_them():
    for other in os.listdir(INC):
        if other != "grandine_bls_gpu_each.h":
            txt = open(os.path.join(INC, other)).read()
            assert not any(n in txt for n in NAMES), other
    hdr = open(HDR).read()
    assert '#include "grandine_bls_gpu_spans.h"' in hdr
    # the spans and the bits headers' entries are theirs alone: not spelled here, not even in a comment
    assert not any(n in hdr for n in G.EXPORTS_SPANS + G.EXPORTS_BITS)
    # what the header has to say: the fail-closed pre-fill, the merge, how an empty item and a zero
    # scalar are treated, and the soundness of the grouped regime
    for word in ("fail closed", "coalescer", "EMPTY item", "ZERO scalar", "2^-64", "GBLS_CALL_BLOCK",
                 "GBLS_AGGR_TYPE_MISMATCH"):
        assert word in hdr, word


def test_library_exports_every_symbol():
    L = G.load_library()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(c_prototypes()[name][1]), name


def test_lib_rs_declares_the_modules():
    lib = open(os.path.join(SRC, "lib.rs")).read()
    assert re.search(r"^pub mod each;$", lib, flags=re.M) and re.search(r"^pub mod ffi_each;$", lib, flags=re.M)


def test_safe_wrappers():
    txt = open(os.path.join(SRC, "each.rs")).read()
    assert txt.count("unsafe {") == txt.count("// SAFETY:") == 2
    sigs = re.findall(r"\bpub fn (\w+)\s*\(([^{]*?)\{", txt, flags=re.S)
    assert sorted(n for n, _ in sigs) == ["verify_each_spans", "verify_items_spans"]
    for name, sig in sigs:
        assert "*const" not in sig and "*mut" not in sig, name
    assert "*const" not in txt and "*mut" not in txt  # nor anywhere else in the file
    c = c_prototypes()
    for name in NAMES:  # each entry is called once, with the header's argument count
        assert txt.count("ffi_each::%s(" % name) == 1, name
        m = re.search(r"ffi_each::%s\((.*?)\)\s*\}?;?\n" % name, txt, flags=re.S)
        assert m, name
        args = [a for a in split_args(" ".join(m.group(1).split()).rstrip(",")) if a.strip()]
        assert len(args) == len(c[name][1]), (name, args)
    for name in ("verify_each_spans", "verify_items_spans"):  # slices are validated, engine errors read back
        body = txt.split("pub fn %s(" % name, 1)[1].split("\npub fn ", 1)[0]
        assert "ranges_ok(" in body and "sets_ok(" in body and "EngineError::Argument" in body, name
        assert "status(rc)" in body or "last_error()" in body, name
    # the items call checks its item offsets against the sets and refuses a zero scalar
    body = txt.split("pub fn verify_items_spans(", 1)[1]
    assert "ranges_ok(messages, item_offsets" in body and "scalars.contains(&0)" in body


@pytest.fixture(scope="module")
def c99_run(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgrandine_bls.so")), "library not built"
    exe = str(tmp_path_factory.mktemp("abi") / "abi_each_c99")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC,
                           os.path.join(ROOT, "tests", "native", "abi_each_c99.c"),
                           "-L", LIBDIR, "-lgrandine_bls", "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def test_c99_consumer_calls_every_entry(c99_run):
    assert set(NAMES) <= set(c99_run)


def test_c99_consumer_fails_closed(c99_run):
    """Without a device: GBLS_VERIFY_FAIL with GBLS_ERR_NO_DEVICE and the pre-fill.  With one: the
    registry and the table are empty, so both keys are rejected, the all-zero signatures do not
    decode, and every verdict is GBLS_VERIFY_FAIL in a call that succeeds."""
    device = c99_run["gbls_init"][0] == "0"
    for name in NAMES:
        assert c99_run[name] == (["0", "0"] if device else ["5", "100"]), (name, c99_run[name])
    for call in ("each", "items"):
        assert c99_run[call + "_verdicts"] == ["5", "5"]
        assert c99_run[call + "_key_status"] == ["1", "1"]
        if device:
            assert "0" not in c99_run[call + "_sig_status"]
        else:
            assert c99_run[call + "_sig_status"] == ["1", "1"]
