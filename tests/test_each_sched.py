"""CPU: the coalescer's merge of span-source requests (grandine_amd/csrc/gbls_sched.h), the code
behind gbls_verify_each_spans and gbls_verify_items_spans, with a recording fake verifier
(tests/native/sched_each_main.cpp): the merged request is the concatenation of the callers'
requests with rebased offsets, every caller receives exactly its slice of the verdicts and of both
status arrays, a failure reaches every merged caller, and single checks, block-class calls and
other key sources are never merged with span batches.

The program is stand-alone (its own main) and is built and run twice: plainly, and with
-fsanitize=address,undefined -fno-sanitize-recover=all."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sched_each_main.cpp")


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_merge_of_span_requests(tmp_path, san):
    exe = str(tmp_path / "sched_each")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "grandine_amd", "csrc"), SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    log = out.stdout[-3000:] + out.stderr[-3000:]
    assert out.returncode == 0, log
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, log
    assert "sched_each: OK" in out.stdout, log
