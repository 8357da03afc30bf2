"""CPU: the verified folds' shared code (grandine_amd/csrc/gbls_fold.h) in a stand-alone native
program (tests/native/fold_harness.cpp): the accumulation and the finish that the fold kernels
compile, built for the CPU and run in the row kernel's order (16 lanes, four row folds) and in the
workgroup kernel's order (256 lanes, the LDS tree), against the Python oracle's
aggregate_signatures and g2_compress over exactly the members whose verdict is GBLS_SUCCESS.

Groups of 0, 1, 2, 15, 16, 17, 255, 256 and 257 members (on both sides of a row and of a
workgroup), and the content cases: a member listed twice (doubles), a signature with its negation
(cancels to infinity with its true count), a group whose members all fail (count 0, infinity), a
failing member between passing ones, a signature listed with its negation twice over and with
infinity.  The argument rules are checked inside the program.

The program is built and run twice: plainly, and with -fsanitize=address,undefined
-fno-sanitize-recover=all.  Nothing is preloaded."""
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "fold_harness.cpp")
INF_BYTES = bytes([0xC0]) + bytes(95)
SIZES = [0, 1, 2, 15, 16, 17, 255, 256, 257]


def mont(a):
    return (a * (1 << 384) % O.P).to_bytes(48, "little")


def raw(pt):
    """blst_p2_affine: x.c0, x.c1, y.c0, y.c1 as little-endian Montgomery limbs; infinity all-zero."""
    if pt is None:
        return bytes(192)
    (x0, x1), (y0, y1) = pt
    return mont(x0) + mont(x1) + mont(y0) + mont(y1)


@pytest.fixture(scope="module")
def case():
    rnd = random.Random(20)
    pool = [O.g2_mul(O.G2_GEN, rnd.randrange(1, O.R)) for _ in range(20)]
    pts = pool + [O.g2_neg(pool[3]), None]             # 20: -pool[3], 21: infinity
    SUCCESS, FAIL = 0, 5
    verdicts = [SUCCESS] * len(pts)
    for bad in (5, 11, 12):
        verdicts[bad] = FAIL
    verdicts[17] = 1                                    # any other nonzero value is not a pass either
    passing = [i for i in range(len(pts)) if verdicts[i] == SUCCESS]
    groups = [[rnd.randrange(len(pts)) for _ in range(k)] for k in SIZES]
    groups += [
        [4, 4],                     # a member listed twice doubles
        [3, 20],                    # a signature with its negation
        [5, 11, 12, 17, 5],         # all members failing
        [1, 11, 2, 5, 6],           # failing members between passing ones
        [3, 7, 20, 3, 20, 21, 21],  # cancels down to pool[7], infinity absorbed
        [7] * 33,                   # one point 33 times: doublings in every lane and in the folds
        passing * 13,               # every lane of the workgroup form busy
    ]
    return pts, verdicts, groups


def expected(case):
    pts, verdicts, groups = case
    out = []
    for g in groups:
        members = [s for s in g if verdicts[s] == 0]
        total = O.aggregate_signatures([pts[s] for s in members])
        out.append((len(members), raw(total).hex(), (O.g2_compress(total) if total is not None else INF_BYTES).hex()))
    return out


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_rows_and_workgroup_orders_match_the_oracle(tmp_path, case, san):
    pts, verdicts, groups = case
    exe = str(tmp_path / "fold_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas"] + san +
                          ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", SRC, "-o", exe])
    inp = tmp_path / "input.txt"
    lines = [str(len(pts))] + ["%s %d" % (raw(p).hex(), v) for p, v in zip(pts, verdicts)]
    lines += [str(len(groups))] + [" ".join(str(x) for x in [len(g)] + g) for g in groups]
    inp.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, str(inp)], env=env, capture_output=True, text=True, timeout=600)
    log = out.stdout[-3000:] + out.stderr[-3000:]
    assert out.returncode == 0, log
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, log
    assert "fold_harness: OK" in out.stdout, log
    want = expected(case)
    # what the content cases must give, whatever the oracle says
    base = len(SIZES)
    assert want[0] == (0, bytes(192).hex(), INF_BYTES.hex())
    assert want[base + 0][0] == 2 and want[base + 0][1] == raw(O.g2_mul(pts[4], 2)).hex()
    assert want[base + 1] == (2, bytes(192).hex(), INF_BYTES.hex())
    assert want[base + 2] == (0, bytes(192).hex(), INF_BYTES.hex())
    assert want[base + 3][0] == 3
    assert want[base + 4] == (7, raw(pts[7]).hex(), O.g2_compress(pts[7]).hex())
    assert want[base + 5] == (33, raw(O.g2_mul(pts[7], 33)).hex(), O.g2_compress(O.g2_mul(pts[7], 33)).hex())
    for order in ("rows", "wg"):
        got = [line.split()[1:] for line in out.stdout.splitlines() if line.startswith(order + " ")]
        assert [int(r[0]) for r in got] == list(range(len(groups)))
        for g, (row, (count, point, comp)) in enumerate(zip(got, want)):
            assert int(row[1]) == count, (order, g)
            assert row[2] == point, (order, g)
            assert row[3] == comp, (order, g)
