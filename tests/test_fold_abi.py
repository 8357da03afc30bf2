"""CPU: the boundary of the verified folds (include/grandine_bls_gpu_fold.h).

* the header's prototype agrees in argument count and types with rust/bls_gpu_sys/src/ffi_fold.rs,
  and in name with grandine_amd/_lib.EXPORTS_FOLD; no other header and no other export list holds
  the name, and the header spells no entry of the earlier extension headers;
* the header says what a consumer has to know: the pre-fill, the infinity encoding, that only the
  each-call has a fold and why;
* the built library exports the symbol, with the header's argument count (this fails on a library
  built without the feature);
* tests/native/abi_fold_c99.c includes the header in a -std=c99 -Wall -Wextra -Werror -pedantic
  translation unit and calls the entry; without a GPU the call fails closed (GBLS_VERIFY_FAIL,
  GBLS_ERR_NO_DEVICE, verdicts at GBLS_VERIFY_FAIL, both status arrays at GBLS_BAD_ENCODING, zero
  points, zero counts, infinity bytes);
* the `unsafe` block of rust/bls_gpu_sys/src/fold.rs carries a SAFETY note, no safe signature takes
  a raw pointer, the wrapper validates its ranges and its groups, and the patched bodies stay
  unwired.
"""
import os
import re
import subprocess

import pytest

from grandine_amd import _lib as G

import test_each_abi as A

ROOT = A.ROOT
INC, SRC, LIBDIR = A.INC, A.SRC, A.LIBDIR
HDR = os.path.join(INC, "grandine_bls_gpu_fold.h")

NAMES = ["gbls_verify_each_fold"]
SCALAR = dict(A.SCALAR, gbls_p2_affine="gbls_p2_affine")
GROUPS = ["*const u32", "*const u32", "usize"]
FOLDS = ["*mut gbls_p2_affine", "*mut [u8; 96]", "*mut u32"]


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
    txt = open(os.path.join(SRC, "ffi_fold.rs")).read()
    block = txt[txt.index('extern "C" {'):]
    out = {}
    for name, args, ret in re.findall(r"pub fn (gbls_\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", block, flags=re.S):
        args = " ".join(args.split()).rstrip(",")
        out[name] = (ret.strip() if ret else None, [a.split(":", 1)[1].strip() for a in A.split_args(args) if a])
    return out


def test_header_rust_and_python_agree():
    c, r = c_prototypes(), rust_prototypes()
    assert sorted(c) == NAMES and sorted(r) == NAMES
    assert c[NAMES[0]] == r[NAMES[0]], (c, r)
    assert sorted(G.EXPORTS_FOLD) == NAMES
    others = (set(G.EXPORTS) | set(G.EXPORTS_COMMITTEES) | set(G.EXPORTS_MSGCACHE) | set(G.EXPORTS_MSGCACHE_CHECKS) |
              set(G.EXPORTS_BITS) | set(G.EXPORTS_SPANS) | set(G.EXPORTS_EACH) | set(G.EXPORTS_LOCAL))
    assert not others & set(NAMES)
    # the each-call's arguments, the groups between the sets and the outputs, the folds last
    assert c[NAMES[0]] == ("c_int", A.SETS + ["usize"] + GROUPS + A.OUTS + FOLDS)


def test_other_headers_declare_none_of_them():
    for other in os.listdir(INC):
        if other != "grandine_bls_gpu_fold.h":
            assert NAMES[0] not in open(os.path.join(INC, other)).read(), other
    hdr = open(HDR).read()
    assert '#include "grandine_bls_gpu_each.h"' in hdr
    # the earlier extension headers' entries are theirs alone: not spelled here, not even in a comment
    assert not any(n in hdr for n in G.EXPORTS_SPANS + G.EXPORTS_BITS + G.EXPORTS_EACH + G.EXPORTS_LOCAL)
    for word in ("Fail closed", "pre-fill", "0xc0", "SignatureBytes::empty", "may be NULL", "GBLS_ERR_ARG", "fold_off[0] != 0",
                 "entry >= n", "does not fit 32 bits", "each\n * occurrence adds once", "An empty group is legal",
                 "sigs_groupcheck = false", "Only the each-call has a fold", "coalescer", "one engine device",
                 "nfold == 0", "blst_p2_affine"):
        assert word in hdr, word


def test_library_exports_the_symbol():
    L = G.load_library()
    fn = getattr(L, NAMES[0])
    assert fn.argtypes is not None and len(fn.argtypes) == len(c_prototypes()[NAMES[0]][1]) == 18
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libgrandine_bls.so")],
                         capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % NAMES[0], out, flags=re.M)


def test_the_kernels_are_in_the_library_without_scratch():
    """Both forms of the fold kernel are built, none keeps anything in scratch memory, and the
    workgroup form's LDS staging has an odd word stride (128 slots of 73 words)."""
    usage = open(os.path.join(LIBDIR, "resource-usage.txt")).read()
    blocks = re.split(r"remark: Function Name: ", usage)
    mine = [b for b in blocks if re.match(r"_ZN4gbls\d+k_g2_fold_", b)]
    assert len(mine) == 3 and sum("k_g2_fold_rows" in b for b in mine) == 2 and sum("k_g2_fold_wg" in b for b in mine) == 1
    for b in mine:
        assert re.search(r"ScratchSize \[bytes/lane\]: 0 ", b), b[:80]
        assert re.search(r"Dynamic Stack: False", b), b[:80]
    wg = next(b for b in mine if "k_g2_fold_wg" in b)
    assert re.search(r"LDS Size \[bytes/block\]: %d " % (128 * 73 * 4), wg)


def test_lib_rs_declares_the_modules():
    lib = open(os.path.join(SRC, "lib.rs")).read()
    assert re.search(r"^pub mod fold;$", lib, flags=re.M) and re.search(r"^pub mod ffi_fold;$", lib, flags=re.M)


def test_safe_wrapper():
    txt = open(os.path.join(SRC, "fold.rs")).read()
    assert txt.count("unsafe {") == txt.count("// SAFETY:") == 1
    sigs = re.findall(r"\bpub fn (\w+)\s*\(([^{]*?)\{", txt, flags=re.S)
    assert [n for n, _ in sigs] == ["verify_each_fold"]
    assert "*const" not in txt and "*mut" not in txt
    assert txt.count("ffi_fold::gbls_verify_each_fold(") == 1
    m = re.search(r"ffi_fold::gbls_verify_each_fold\((.*?)\)\s*\}?;?\n", txt, flags=re.S)
    args = [a for a in A.split_args(" ".join(m.group(1).split()).rstrip(",")) if a.strip()]
    assert len(args) == len(c_prototypes()[NAMES[0]][1])
    body = txt.split("pub fn verify_each_fold(", 1)[1]
    assert "sets_ok(" in body and "groups_ok(group_sets, group_offsets, n)" in body
    assert "EngineError::Argument" in body and "status(rc)" in body
    groups = txt.split("fn groups_ok(", 1)[1].split("\n}\n", 1)[0]
    assert "ranges_ok(group_sets, group_offsets" in groups and "s < n" in groups and "u32::try_from" in groups
    # the patched bodies stay unwired
    patch = os.path.join(ROOT, "rust", "bls_patch")
    for dirpath, _, files in os.walk(patch):
        for f in files:
            assert "fold::" not in open(os.path.join(dirpath, f), errors="replace").read(), f


@pytest.fixture(scope="module")
def c99_run(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgrandine_bls.so")), "library not built"
    exe = str(tmp_path_factory.mktemp("abi") / "abi_fold_c99")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC,
                           os.path.join(ROOT, "tests", "native", "abi_fold_c99.c"),
                           "-L", LIBDIR, "-lgrandine_bls", "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def test_c99_consumer_fails_closed(c99_run):
    """Without a device: GBLS_VERIFY_FAIL with GBLS_ERR_NO_DEVICE and the pre-fill.  With one: the
    registry and the committee table are empty, so every key is rejected, the all-zero signatures
    do not decode, every verdict is GBLS_VERIFY_FAIL in a call that succeeds -- and nothing enters
    any sum, so the fold outputs are the same either way."""
    device = c99_run["gbls_init"][0] == "0"
    for name in (NAMES[0], "no_bytes", "no_groups"):
        assert c99_run[name] == (["0", "0"] if device else ["5", "100"]), (name, c99_run[name])
    assert c99_run["fold_verdicts"] == ["5", "5", "5"] and c99_run["no_groups_verdicts"] == ["5", "5", "5"]
    assert c99_run["fold_key_status"] == ["1", "1", "1"]
    if device:
        assert "0" not in c99_run["fold_sig_status"]
    else:
        assert c99_run["fold_sig_status"] == ["1", "1", "1"]
    assert c99_run["fold_out_nonzero_bytes"] == ["0"] and c99_run["fold_count"] == ["0", "0", "0"]
    assert c99_run["fold_bytes_infinity"] == ["3"]
    assert c99_run["no_bytes_out_nonzero_bytes"] == ["0"] and c99_run["no_bytes_count"] == ["0", "0", "0"]
