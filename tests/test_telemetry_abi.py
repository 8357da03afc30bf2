"""CPU: the boundary of the engine telemetry (include/grandine_bls_gpu_telemetry.h).

* the header's prototypes and structs agree with rust/bls_gpu_sys/src/ffi_telemetry.rs (argument
  types, field names, order and types, the constants) and with grandine_amd/_lib.py
  (EXPORTS_TELEMETRY, the ctypes structs and their sizes); no other header and no other export list
  holds the names, and the header spells no entry of any other header, not even in a comment;
* the built library exports the symbols (this fails on a library built without the feature);
* tests/native/abi_telemetry_c99.c includes the header in a -std=c99 -Wall -Wextra -Werror -pedantic
  translation unit and, with no engine open, finds: enable returns the previous levels, a read is all
  zero (and a shorter struct is filled only as far as it reaches), the trace is empty, the memory
  gauges are zeros, the name functions end in NULL;
* the safe wrappers of rust/bls_gpu_sys/src/telemetry.rs: one SAFETY note per `unsafe` block, no raw
  pointer in a safe signature, `engine()` reads GBLS_TELEMETRY, and the patched bodies stay unwired.
"""
import ctypes
import os
import re
import subprocess

import pytest

from grandine_amd import _lib as G

import test_each_abi as A

ROOT = A.ROOT
INC, SRC, LIBDIR = A.INC, A.SRC, A.LIBDIR
HDR = os.path.join(INC, "grandine_bls_gpu_telemetry.h")
FFI = os.path.join(SRC, "ffi_telemetry.rs")

NAMES = sorted(["gbls_telemetry_enable", "gbls_telemetry_read", "gbls_telemetry_reset", "gbls_telemetry_trace",
                "gbls_telemetry_memory", "gbls_telemetry_phase_name", "gbls_telemetry_kind_name",
                "gbls_telemetry_class_name"])
STRUCTS = {"gbls_telemetry_hist": G.TelemetryHist, "gbls_telemetry_cell": G.TelemetryCell,
           "gbls_telemetry_snapshot": G.TelemetrySnapshot, "gbls_telemetry_record": G.TelemetryRecord,
           "gbls_telemetry_engine_memory": G.TelemetryEngineMemory, "gbls_telemetry_memory_info": G.TelemetryMemoryInfo}
SCALAR = dict(A.SCALAR, char="c_char", void="c_void", **{s: s for s in STRUCTS})
CTYPES = {"u32": ctypes.c_uint32, "u64": ctypes.c_uint64}


def header():
    return re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)


def c_defines():
    return {k: int(v) for k, v in re.findall(r"^#define (GBLS_TELEMETRY_\w+) (\d+)", header(), flags=re.M)}


def c_prototypes():
    out = {}
    for ret, name, args in re.findall(r"^((?:const )?\w+ \*?)(gbls_telemetry_\w+)\(([^;{]*?)\);", header(), flags=re.M | re.S):
        args = " ".join(args.split())
        types = []
        for a in ([] if args == "void" else A.split_args(args)):
            m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*\w+$", a.strip())
            assert m, a
            types.append(("*%s " % ("const" if m.group(1) else "mut") if m.group(3) else "") + SCALAR[m.group(2)])
        m = re.match(r"(const )?(\w+) (\*?)$", ret)
        r = ("*%s " % ("const" if m.group(1) else "mut") if m.group(3) else "") + SCALAR[m.group(2)]
        out[name] = (None if r == "c_void" else r, types)
    return out


def rust_prototypes():
    txt = open(FFI).read()
    block = txt[txt.index('extern "C" {'):]
    out = {}
    for name, args, ret in re.findall(r"pub fn (gbls_\w+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", block, flags=re.S):
        args = " ".join(args.split()).rstrip(",")
        out[name] = (ret.strip() if ret else None, [a.split(":", 1)[1].strip() for a in A.split_args(args) if a])
    return out


def c_structs():
    """{name: [(field, rust type)]} from the header's typedefs, array sizes by their macro names."""
    out = {}
    for body, name in re.findall(r"typedef struct \{(.*?)\} (\w+);", header(), flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            ctype, rest = decl.split(" ", 1)
            for item in rest.split(","):
                m = re.match(r"(\w+)((?:\[\w+\])*)$", item.strip())
                assert m, decl
                t = SCALAR[ctype]
                for dim in reversed(re.findall(r"\[(\w+)\]", m.group(2))):
                    t = "[%s; %s]" % (t, dim)
                fields.append((m.group(1), t))
        out[name] = fields
    return out


def rust_structs():
    txt = open(FFI).read()
    out = {}
    for name, body in re.findall(r"#\[repr\(C\)\]\n#\[derive\([^\]]*\)\]\npub struct (\w+) \{(.*?)\n\}", txt, flags=re.S):
        out[name] = [(f, t.strip()) for f, t in re.findall(r"pub (\w+): ([^,\n]+),", body)]
    return out


def test_header_rust_and_python_agree():
    c, r = c_prototypes(), rust_prototypes()
    assert sorted(c) == NAMES and sorted(r) == NAMES
    for n in NAMES:
        assert c[n] == r[n], (n, c[n], r[n])
    assert sorted(G.EXPORTS_TELEMETRY) == NAMES
    others = (set(G.EXPORTS) | set(G.EXPORTS_COMMITTEES) | set(G.EXPORTS_MSGCACHE) | set(G.EXPORTS_MSGCACHE_CHECKS) |
              set(G.EXPORTS_BITS) | set(G.EXPORTS_SPANS) | set(G.EXPORTS_EACH) | set(G.EXPORTS_LOCAL) | set(G.EXPORTS_FOLD))
    assert not others & set(NAMES)
    assert c["gbls_telemetry_enable"] == ("c_int", ["c_int"])
    assert c["gbls_telemetry_trace"] == ("usize", ["*mut gbls_telemetry_record", "usize", "*mut u64"])
    assert c["gbls_telemetry_phase_name"] == ("*const c_char", ["c_int"]) and c["gbls_telemetry_reset"] == (None, [])


def test_constants_and_structs_agree():
    defs = c_defines()
    assert defs["GBLS_TELEMETRY_TRACE_CAPACITY"] == 1024 and defs["GBLS_TELEMETRY_BUCKETS"] == 32
    rs = open(FFI).read()
    for k, v in defs.items():
        assert re.search(r"^pub const %s: usize = %d;$" % (k, v), rs, flags=re.M), k
        assert getattr(G, k[len("GBLS_"):]) == v, k
    c, r = c_structs(), rust_structs()
    assert sorted(c) == sorted(r) == sorted(STRUCTS)
    for name, cls in STRUCTS.items():
        assert c[name] == r[name], name
        assert [f for f, _ in c[name]] == [f for f, _ in cls._fields_], name
        # the ctypes struct, field by field: element type and total element count
        for (f, t), (_, ct) in zip(c[name], cls._fields_):
            dims = [defs[d] for d in re.findall(r"; (\w+)\]", t)]
            base = re.sub(r"[\[\]]|; \w+", "", t)
            want = CTYPES.get(base) or STRUCTS[base]
            total = 1
            for d in dims:
                total *= d
            assert ctypes.sizeof(ct) == total * ctypes.sizeof(want), (name, f)


def test_other_headers_declare_none_of_them():
    for other in os.listdir(INC):
        if other != "grandine_bls_gpu_telemetry.h":
            txt = open(os.path.join(INC, other)).read()
            assert "gbls_telemetry" not in txt, other
    hdr = open(HDR).read()
    assert '#include "grandine_bls_gpu.h"' in hdr
    # every other header's entries are theirs alone: not spelled here, not even in a comment
    theirs = (G.EXPORTS + G.EXPORTS_COMMITTEES + G.EXPORTS_MSGCACHE + G.EXPORTS_MSGCACHE_CHECKS + G.EXPORTS_BITS +
              G.EXPORTS_SPANS + G.EXPORTS_EACH + G.EXPORTS_LOCAL + G.EXPORTS_FOLD)
    assert not [n for n in theirs if re.search(r"\b%s\b" % n, hdr)]
    for word in ("GBLS_TELEMETRY_TRACE_CAPACITY (1024)", "one relaxed atomic load", "under 1024 ns", "2^40", "never negative",
                 "lock-free", "never synchronises", "total >= hold + window + queue + run", "run >= enqueue + sync",
                 "enqueue >= staging", "left on in a node", "sizeof of ITS struct", "NULL past the end", "rejected"):
        assert " ".join(word.split()) in " ".join(hdr.replace(" *", " ").split()), word


def test_library_exports_every_symbol():
    L = G.load_library()
    protos = c_prototypes()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libgrandine_bls.so")],
                         capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(protos[name][1]), name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
    # the earlier export lists are as they were
    assert len(G.EXPORTS) == 43 and "gbls_telemetry_enable" not in G.EXPORTS


def test_lib_rs_declares_the_modules_and_reads_the_variable():
    lib = open(os.path.join(SRC, "lib.rs")).read()
    assert re.search(r"^pub mod telemetry;$", lib, flags=re.M) and re.search(r"^pub mod ffi_telemetry;$", lib, flags=re.M)
    engine = lib.split("pub fn engine()", 1)[1].split("\n}\n", 1)[0]
    assert "telemetry::level_from_env()" in engine and engine.index("level_from_env") < engine.index("ffi::gbls_init(")
    txt = open(os.path.join(SRC, "telemetry.rs")).read()
    assert '"GBLS_TELEMETRY"' in txt and '"1" => Some(Level::Phases)' in txt and '"2" => Some(Level::DeviceTime)' in txt


def test_safe_wrappers():
    txt = open(os.path.join(SRC, "telemetry.rs")).read()
    assert txt.count("unsafe {") == txt.count("// SAFETY:") == 6
    sigs = re.findall(r"\bpub fn (\w+)\s*\(([^{]*?)\{", txt, flags=re.S)
    assert [n for n, _ in sigs] == ["enable", "level_from_env", "snapshot", "reset", "trace", "memory", "phase_names",
                                    "kind_names", "class_names"]
    for n, sig in sigs:
        assert "*const" not in sig and "*mut" not in sig, n
    for name in NAMES:
        assert len(re.findall(r"ffi_telemetry::%s\b" % name, txt)) == 1, name
    # the patched bodies stay unwired
    patch = os.path.join(ROOT, "rust", "bls_patch")
    for dirpath, _, files in os.walk(patch):
        for f in files:
            assert "telemetry::" not in open(os.path.join(dirpath, f), errors="replace").read(), f


@pytest.fixture(scope="module")
def c99_run(tmp_path_factory):
    assert os.path.exists(os.path.join(LIBDIR, "libgrandine_bls.so")), "library not built"
    exe = str(tmp_path_factory.mktemp("abi") / "abi_telemetry_c99")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INC,
                           os.path.join(ROOT, "tests", "native", "abi_telemetry_c99.c"),
                           "-L", LIBDIR, "-lgrandine_bls", "-Wl,-rpath," + LIBDIR, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return {line.split()[0]: line.split()[1:] for line in out.stdout.splitlines()}


def test_c99_consumer_without_an_engine(c99_run):
    r = c99_run
    assert r["gbls_telemetry_enable"] == ["0", "1", "2", "2", "0"]            # the previous levels, 7 clamped to 2
    size = str(ctypes.sizeof(G.TelemetrySnapshot))
    assert r["gbls_telemetry_read"] == ["0", size, "0", "0"]                   # level 0, every byte behind the head zero
    assert r["short_read"] == ["0", "16", "16"] and r["bad_read"] == ["5", "5"]
    assert r["gbls_telemetry_trace"] == ["0", "0", "0"]
    assert r["gbls_telemetry_memory"] == ["0", str(ctypes.sizeof(G.TelemetryMemoryInfo)), "0", "0"]
    assert r["gbls_telemetry_phase_name"] == ["13", "hold", "lag"]
    assert r["gbls_telemetry_kind_name"] == ["9", "batch", "device"]
    assert r["gbls_telemetry_class_name"] == ["2", "normal", "block"]
    assert r["sizes"] == [str(ctypes.sizeof(c)) for c in (G.TelemetryHist, G.TelemetryCell, G.TelemetrySnapshot,
                                                          G.TelemetryRecord, G.TelemetryEngineMemory, G.TelemetryMemoryInfo)]
    assert r["capacity"] == ["1024"]
