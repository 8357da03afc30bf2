"""CPU: the coalescer's merge of fold requests (grandine_amd/csrc/gbls_sched.h), the code behind
gbls_verify_each_fold, with a recording fake verifier (tests/native/sched_fold_main.cpp): fold
requests are a kind of their own (never merged with span or local requests), the merged CSR is the
concatenation of the callers' groups with each caller's entries moved up by its first set, every
caller receives exactly its slices of the points, counts and bytes beside its verdicts and statuses
(a caller without groups among the others included), a failure reaches every merged caller with no
fold output written, and eight threads go through Coalescer::submit.

The merged CSR the program prints is checked here against a concatenation computed from the
callers' own groups.  The program is stand-alone (its own main) and is built and run twice:
plainly, and with -fsanitize=address,undefined -fno-sanitize-recover=all."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sched_fold_main.cpp")


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_merge_of_fold_requests(tmp_path, san):
    exe = str(tmp_path / "sched_fold")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "grandine_amd", "csrc"), SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    log = out.stdout[-3000:] + out.stderr[-3000:]
    assert out.returncode == 0, log
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, log
    assert "sched_fold: OK" in out.stdout, log
    rows = {}
    callers = []
    for line in out.stdout.splitlines():
        words = line.split()
        if words[0] in ("csr_off", "csr_set"):
            rows[words[0]] = [int(w) for w in words[1:]]
        elif words[0] == "caller":
            groups = [[int(w) for w in part.split()] for part in line.split("|")[1:]]
            callers.append((int(words[1]), groups))
    # five callers, the second without groups; the concatenation computed here
    assert [n for n, _ in callers] == [3, 2, 1, 5, 2] and callers[1][1] == [] and [] in callers[0][1]
    want_off, want_set, at = [0], [], 0
    for n, groups in callers:
        for g in groups:
            want_set += [at + s for s in g]
            want_off.append(len(want_set))
        at += n
    assert rows["csr_off"] == want_off and rows["csr_set"] == want_set
    assert len(want_off) == 10 and want_set[:3] == [0, 1, 2] and want_set[6] == 5 and max(want_set) == 12
