"""CPU: the host rules of local key sets (grandine_amd/csrc/gbls_local.h) in a stand-alone native
program (tests/native/local_harness.cpp): the tail layout of the piece array over interleaved
local, span and plain sets and over shard slices, a local set's piece, the argument rules, and what
a local set's piece gives over a small key table (sums, a repeated position, a key with its
negation, empty and out-of-range ranges, an invalid key) behind the plain-piece loop and the finish
the kernels compile.  The layouts the program prints are checked here against a computation of
their own.

The program is built and run twice: plainly, and with -fsanitize=address,undefined
-fno-sanitize-recover=all.  Nothing is preloaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "local_harness.cpp")


def pieces(kind):
    return 1 if kind in "LP" else 64 if kind == "0" else int(kind) + 1


def layout(kinds, b, e):
    """Non-local sets' pieces first, in set order, then the local sets', in set order."""
    part = kinds[b:e]
    np_span = sum(pieces(k) for k in part if k != "L")
    first, s, l = [], 0, np_span
    for k in part:
        if k == "L":
            first.append(l)
            l += 1
        else:
            first.append(s)
            s += pieces(k)
    return [np_span, l - np_span] + first


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_layout_pieces_and_arguments(tmp_path, san):
    exe = str(tmp_path / "local_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas"] + san +
                          ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    log = out.stdout[-3000:] + out.stderr[-3000:]
    assert out.returncode == 0, log
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, log
    assert "local_harness: OK" in out.stdout, log
    shown = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith("layout ")]
    assert len(shown) == 7 and {row[0] for row in shown} == {"L2PL0PLLP7L", "LLLL", "P3P"}
    for kinds, b, e, *got in shown:
        assert [int(x) for x in got] == layout(kinds, int(b), int(e)), (kinds, b, e)
    # the interleaved case: 3 + 1 + 64 + 1 + 1 + 8 head pieces, five local pieces behind them
    assert layout("L2PL0PLLP7L", 0, 11)[:2] == [78, 5]
