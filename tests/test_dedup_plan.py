"""CPU: the host-side message-grouping plan (grandine_amd/csrc/gbls_dedup.h, GBLS_INIT_DEDUP)
through a stand-alone program built with AddressSanitizer and UBSan
(tests/native/dedup_plan_main.cpp), against a Python dict grouping."""
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "dedup_plan_main.cpp")
EXE = os.path.join(ROOT, "tests", "native", "_build", "dedup_plan_main_san")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", EXE, SRC])
    return EXE


def run_plan(exe, tmp_path, msgs, seg_off):
    path = str(tmp_path / "shape.bin")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<II", len(msgs), len(seg_off) - 1))
        fh.write(struct.pack("<%dI" % len(seg_off), *seg_off))
        fh.write(b"".join(msgs))
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout


def parse(text):
    lines = text.splitlines()
    head = lines[0].split()
    plan = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    for line in lines[1:4]:
        name, *vals = line.split()
        plan[name] = [int(v) for v in vals]
    hexs = lines[4].split()
    plan["msgs"] = bytes.fromhex(hexs[1]) if len(hexs) > 1 else b""
    return plan


def expect(msgs, seg_off):
    """Groups per segment in order of first member (dicts keep insertion order)."""
    groups, grp_seg_off = [], [0]
    for s in range(len(seg_off) - 1):
        by_msg = {}
        for i in range(seg_off[s], seg_off[s + 1]):
            by_msg.setdefault(msgs[i], []).append(i)
        groups += list(by_msg.items())
        grp_seg_off.append(len(groups))
    return groups, grp_seg_off


def check(exe, tmp_path, msgs, seg_off):
    n = len(msgs)
    text = run_plan(exe, tmp_path, msgs, seg_off)
    assert run_plan(exe, tmp_path, msgs, seg_off) == text  # two runs (two process keys): identical output
    p = parse(text)
    groups, grp_seg_off = expect(msgs, seg_off)
    assert p["n"] == n and p["nseg"] == len(seg_off) - 1
    assert p["groups"] == len(groups)
    assert p["duplicates"] == (1 if len(groups) < n else 0)
    assert p["max_group"] == max([len(m) for _, m in groups], default=0)
    assert p["grp_seg_off"] == grp_seg_off  # group order: by segment ...
    assert len(p["grp_off"]) == len(groups) + 1 and p["grp_off"][0] == 0 and p["grp_off"][-1] == n
    got = [p["grp_set"][p["grp_off"][g]:p["grp_off"][g + 1]] for g in range(len(groups))]
    assert got == [m for _, m in groups]  # ... then by first member; members ascending
    assert sorted(p["grp_set"]) == list(range(n))  # every set in exactly one group
    for s in range(len(seg_off) - 1):  # ... of its own segment
        for g in range(grp_seg_off[s], grp_seg_off[s + 1]):
            assert all(seg_off[s] <= i < seg_off[s + 1] for i in got[g])
    for g, members in enumerate(got):  # members byte-equal
        assert len({msgs[i] for i in members}) == 1
    if len(groups) < n:
        assert p["msgs"] == b"".join(m for m, _ in groups)
    else:
        assert p["msgs"] == b""  # no duplicates: nothing to upload
    return p


def rnd_msgs(rng, k):
    return [rng.randbytes(32) for _ in range(k)]


def test_empty_and_single(exe, tmp_path):
    assert check(exe, tmp_path, [], [0])["groups"] == 0
    assert check(exe, tmp_path, [], [0, 0, 0])["groups"] == 0
    p = check(exe, tmp_path, rnd_msgs(random.Random(1), 1), [0, 1])
    assert p["groups"] == 1 and p["duplicates"] == 0


def test_all_equal_and_all_distinct(exe, tmp_path):
    rng = random.Random(2)
    m = rng.randbytes(32)
    p = check(exe, tmp_path, [m] * 64, [0, 64])
    assert p["groups"] == 1 and p["max_group"] == 64
    p = check(exe, tmp_path, rnd_msgs(rng, 131), [0, 131])
    assert p["groups"] == 131 and p["duplicates"] == 0  # U == n is reported


def test_messages_differing_in_one_byte(exe, tmp_path):
    base = random.Random(3).randbytes(32)
    last = [base[:31] + bytes([b]) for b in (0, 1, 2, 0, 1, 255)]
    assert check(exe, tmp_path, last, [0, 6])["groups"] == 4
    first = [bytes([b]) + base[1:] for b in (7, 8, 7, 9, 8, 7)]
    assert check(exe, tmp_path, first, [0, 6])["groups"] == 3
    zeros = [bytes(32), bytes(31) + b"\x01", b"\x01" + bytes(31), bytes(32)]
    assert check(exe, tmp_path, zeros, [0, 4])["groups"] == 3


def test_one_message_in_two_segments_and_empty_segments(exe, tmp_path):
    rng = random.Random(4)
    a, b = rnd_msgs(rng, 2)
    msgs = [a, b, a, a, b, b]
    p = check(exe, tmp_path, msgs, [0, 0, 3, 3, 6, 6])
    assert p["groups"] == 4  # a and b in each of the two non-empty segments
    assert p["grp_seg_off"] == [0, 0, 2, 2, 4, 4]
    p = check(exe, tmp_path, [a, a], [0, 1, 2])  # the same message, one set per segment
    assert p["groups"] == 2 and p["duplicates"] == 0


def test_group_sizes(exe, tmp_path):
    rng = random.Random(5)
    sizes = [1, 2, 63, 64, 65, 513]
    keys = rnd_msgs(rng, len(sizes))
    msgs = [k for k, s in zip(keys, sizes) for _ in range(s)]
    rng.shuffle(msgs)
    p = check(exe, tmp_path, msgs, [0, len(msgs)])
    assert sorted(p["grp_off"][g + 1] - p["grp_off"][g] for g in range(p["groups"])) == sizes
    # the same multiset cut into segments at odd places
    check(exe, tmp_path, msgs, [0, 1, 64, 65, 300, len(msgs)])


def test_65536_sets_1000_messages(exe, tmp_path):
    rng = random.Random(6)
    keys = rnd_msgs(rng, 1000)
    msgs = keys + [keys[rng.randrange(1000)] for _ in range(65536 - 1000)]
    rng.shuffle(msgs)
    p = check(exe, tmp_path, msgs, [0, 65536])
    assert p["groups"] == 1000
    check(exe, tmp_path, msgs, [0, 4096, 4096, 40000, 65536])
