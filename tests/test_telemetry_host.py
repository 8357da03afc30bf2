"""CPU: the telemetry recording structures (grandine_amd/csrc/gbls_telemetry.h) and the scheduler's
telemetry stamps (grandine_amd/csrc/gbls_sched.h), in the stand-alone tests/native/telemetry_main.cpp
(its own main), built and run plainly, under ASan + UBSan and under ThreadSanitizer:

* bucket edges at 1023, 1024, 2^k - 1, 2^k, 2^40 and UINT64_MAX; sum and max; the power-of-two bins;
* a ring compiled at capacity 8: order, overwrite, the dropped count, a short drain;
* a reader draining while 8 threads record never sees a torn record (each record carries a checksum
  of its own fields) and every ticket is either read or counted as lost;
* counters conserved under 8 recorders, with a snapshot taken meanwhile;
* the scheduler with a stub verifier and an injected clock: the phases of a lone caller; a follower's
  queue equals its leader's window + queue less its later arrival; a held caller's hold; run
  identical across a batch; the callers of all submissions are the requests submitted (8 threads);
  and with the hooks absent (requests without phases, or no clock) the injected clock is never read;
* a context pool of stub contexts: a lease that waits for a context of an exhausted class, and a wait
  on a staging slot, through the hooks the engine uses (tel::timed_acquire, tel::timed_wait), arrive
  as nonzero `lease` and `staging` samples and in `staging_waits`; without a shard no clock is read;
* a caller with phases whose leader had no clock records nothing waited (no wrap-around).

Neither a lease wait nor a staging-slot wait can be provoked deterministically on the GPU; both are
measured by host-only hooks of gbls_telemetry.h, which this program drives with a stub pool and a
stub wait.
Every existing program under tests/native that includes gbls_sched.h builds unchanged: their own
tests build them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "telemetry_main.cpp")


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["-fsanitize=thread"]],
                         ids=["plain", "asan-ubsan", "tsan"])
def test_recording_structures_and_scheduler_stamps(tmp_path, san):
    exe = str(tmp_path / "telemetry_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra", "-Werror"] + san +
                          ["-I", os.path.join(ROOT, "grandine_amd", "csrc"), SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    log = out.stdout[-3000:] + out.stderr[-3000:]
    assert out.returncode == 0, log
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, log
    lines = out.stdout.split("\n")
    for part in ("buckets ok", "ring ok", "counters ok", "scheduler ok", "waits ok", "unstamped ok", "telemetry: OK"):
        assert part in lines, log
    assert any(line.startswith("ring threads ok read ") for line in lines), log


def test_the_header_is_host_only():
    txt = open(os.path.join(ROOT, "grandine_amd", "csrc", "gbls_telemetry.h")).read()
    assert "hip" not in txt.lower().replace("gbls_capi.hip", "").replace("(no hip)", "")
    assert "memory_order_relaxed" in txt and "compare_exchange_weak" in txt
