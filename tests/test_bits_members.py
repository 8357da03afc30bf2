"""CPU: the bookkeeping of the resident committee member lists (grandine_amd/csrc/gbls_members.h)
as a stand-alone ASan + UBSan program (tests/native/members_main.cpp) against a Python dict model.

A random sequence of gbls_committees_set_members (also with committees whose status comes back
nonzero), plain gbls_committees_set, gbls_committees_clear, the registry rewrite, failure
truncation and reader look-ups, over overlapping ranges with changing sizes; after every step the
slot -> (present, length, contents) map, the blocks freed by the step and the bytes held are
compared.  Readers hold no pin in this bookkeeping: in the engine they enqueue under the shared
registry lock and a dead block is freed on the device behind their events, so here a reader step
reads every slot's members through its view (a freed block would be a sanitizer report) and must
change nothing.

The deterministic leg is the steady epoch rollover: 20 alternating rewrites of the two halves of
the table with committee sizes that differ from call to call.  The bytes held stay within the bound
DESIGN.md section 15 states: two calls' blocks between calls, three inside a call."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "members_main.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("members") / "members_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", out])
    return out


class Model:
    """slot -> (call, [contents]); a call's block is held while a slot still shows its members."""

    def __init__(self):
        self.slots = {}
        self.size = 0
        self.calls = {}   # call -> bytes of its block, while held
        self.call = 0

    def _reap(self):
        live = {c for c, _ in self.slots.values()}
        freed = sorted(c for c in self.calls if c not in live)
        for c in freed:
            del self.calls[c]
        return freed

    def step(self, op):
        kind = op[0]
        before = sum(self.calls.values())
        peak = before
        freed = []
        if kind in "MJF":
            first, lens, extra = op[1], op[2], op[3]
            self.call += 1
            keep = kind != "F" or extra
            total = sum(lens)
            if keep and lens:
                self.calls[self.call] = 4 * total
                peak = before + 4 * total
            if kind == "F":
                self.slots = {s: v for s, v in self.slots.items() if s < first}
                self.size = min(self.size, first)
            else:
                self.size = max(self.size, first + len(lens))
                pos = 0
                for c, n in enumerate(lens):
                    self.slots[first + c] = (self.call, [self.call * 65536 + pos + k for k in range(n)])
                    pos += n
            freed = self._reap()
            if kind == "J":
                for c in range(len(lens)):
                    if extra >> (c % 32) & 1:
                        self.slots.pop(first + c, None)
                freed += self._reap()
        elif kind == "P":
            first, ncom = op[1], op[2]
            self.call += 1
            self.size = max(self.size, first + ncom)
            for c in range(ncom):
                self.slots.pop(first + c, None)
            freed = self._reap()
        elif kind in "CR":
            self.slots = {}
            self.size = 0
            freed = self._reap()
        return {"bytes": sum(self.calls.values()), "peak": peak, "blocks": len(self.calls), "freed": freed,
                "slots": {s: v[1] for s, v in self.slots.items()}}


def text(op):
    if op[0] in "MJF":
        tail = [] if op[0] == "M" else [op[3]]
        return " ".join(map(str, [op[0], op[1], len(op[2])] + list(op[2]) + tail))
    return " ".join(map(str, op))


def parse(line):
    head, _, tail = line.partition(" |")
    f = dict(kv.split("=") for kv in head.split())
    slots = {}
    for item in tail.split():
        s, n, vals = item.split(":")
        slots[int(s)] = [int(v) for v in vals.split(",")] if vals else []
        assert len(slots[int(s)]) == int(n)
    return {"bytes": int(f["bytes"]), "peak": int(f["peak"]), "blocks": int(f["blocks"]),
            "freed": sorted(int(c) for c in f["freed"].split(",") if c), "slots": slots}


def run(exe, ops):
    out = subprocess.run([exe], input="\n".join(text(o) for o in ops) + "\n", capture_output=True, text=True,
                         timeout=300)
    log = out.stdout[-2000:] + out.stderr[-3000:]
    assert out.returncode == 0, log
    lines = out.stdout.splitlines()
    assert lines[-1] == "members: OK" and len(lines) == len(ops) + 1, log
    return [parse(l) for l in lines[:-1]]


def random_ops(seed, n):
    rng = random.Random(seed)
    ops = []
    for _ in range(n):
        k = rng.random()
        first = rng.randrange(0, 40)
        lens = [rng.choice([0, 1, 2, 3, 7, 16, 33]) for _ in range(rng.randrange(0, 24))]
        if k < 0.40:
            ops.append(("M", first, lens, 0))
        elif k < 0.50:
            ops.append(("J", first, lens, rng.getrandbits(32) & rng.getrandbits(32)))
        elif k < 0.68:
            ops.append(("P", first, rng.randrange(0, 24)))
        elif k < 0.72:
            ops.append(("C",))
        elif k < 0.76:
            ops.append(("R",))
        elif k < 0.86:
            ops.append(("F", first, lens, rng.randrange(2)))
        else:
            ops.append(("V", rng.randrange(0, 64)))
    return ops


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sequence_against_the_model(exe, seed):
    ops = random_ops(seed, 400)
    assert {o[0] for o in ops} == set("MJPCRFV")
    got = run(exe, ops)
    model = Model()
    for i, (op, g) in enumerate(zip(ops, got)):
        want = model.step(op)
        assert g == want, (i, op)
    assert any(g["freed"] for g in got) and max(g["blocks"] for g in got) >= 3


def test_epoch_rollover_stays_within_the_bound(exe):
    """Halves A (slots 0..63) and B (64..127) rewritten alternately, 20 rewrites, the committee
    sizes changing with every call."""
    ops, half_bytes = [], []
    for i in range(20):
        lens = [90 + 13 * ((i * 7 + c) % 11) + 5 * i for c in range(64)]
        ops.append(("M", 64 * (i % 2), lens, 0))
        half_bytes.append(4 * sum(lens))
    got = run(exe, ops)
    model = Model()
    for i, (op, g) in enumerate(zip(ops, got)):
        assert g == model.step(op), i
        assert len(g["slots"]) == (64 if i == 0 else 128)
        # between calls: this call's block and the other half's last one; the block this call
        # replaced (two calls back) was freed by it
        assert g["blocks"] == min(i + 1, 2) and g["bytes"] == sum(half_bytes[max(0, i - 1):i + 1])
        assert g["freed"] == ([i - 1] if i >= 2 else [])
        # inside a call: three halves at the most
        assert g["peak"] == sum(half_bytes[max(0, i - 2):i + 1]) <= 3 * max(half_bytes)
