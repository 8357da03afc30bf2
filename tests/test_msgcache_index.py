"""CPU: the host index and shard plan of the message line cache (grandine_amd/csrc/gbls_msgcache.h)
through a stand-alone program built with AddressSanitizer and UBSan
(tests/native/msgcache_index_main.cpp), against a Python dict-plus-LRU model: random sequences of
plan (hits pinned), end-with-verdicts (publish on success, drop on failure, unpin) and clear over
2-16 slots and 1-40 messages, several calls in flight."""
import collections
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "msgcache_index_main.cpp")
EXE = os.path.join(ROOT, "tests", "native", "_build", "msgcache_index_main_san")
FREE, TAKEN, ENTRY, ZOMBIE = range(4)
STATS = ("lookups", "hits", "misses", "published", "evictions", "bypassed")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", EXE, SRC])
    return EXE


def run_script(exe, tmp_path, lines):
    path = str(tmp_path / "script.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout


def parse(line):
    head, state = line.split(" | ")
    r = {"op": head.split()[0]}
    if r["op"] == "plan":
        parts = [p.strip() for p in head.split(";") if p.strip()]
        tok = parts[0].split()
        r.update(t=int(tok[1]), U=int(tok[3]), M=int(tok[5]), D=int(tok[7]))
        parts[0] = " ".join(tok[8:])
        for part in parts:
            name, *vals = part.split()
            r[name] = [None if v == "-1" else int(v) for v in vals]
    tok = state.split()
    r["entries"] = int(tok[1])
    r["stats"] = dict(zip(STATS, (int(x) for x in tok[3:9])))
    at = tok.index("slots")
    lru = tok.index("lru")
    r["slots"] = []
    for s in tok[at + 1:lru]:
        st, pins, mid = s.split(":")
        r["slots"].append((int(st), int(pins), None if mid == "-" else int(mid)))
    r["lru"] = [int(x) for x in tok[lru + 1:]]
    return r


class Model:
    """dict + LRU: entries (message -> slot) in use order, a free stack, pins per slot."""

    def __init__(self, slots, spare):
        self.slots, self.total = slots, slots + spare
        self.entries = collections.OrderedDict()  # last = most recently used
        self.pins = [0] * self.total
        self.zombie = set()
        self.taken = set()
        self.free = list(range(self.total - 1, -1, -1))  # pop() hands out slot 0 first
        self.epoch = 0
        self.st = dict.fromkeys(STATS, 0)
        self.calls = {}

    def plan(self, t, seg_off, ids):
        groups = []  # (segment, message) in order of first member
        for s in range(len(seg_off) - 1):
            seen = []
            for i in range(seg_off[s], seg_off[s + 1]):
                if ids[i] not in seen:
                    seen.append(ids[i])
            groups += [(s, m) for m in seen]
        distinct = list(dict.fromkeys(m for _, m in groups))
        hit, slot = {}, {}
        for m in distinct:
            self.st["lookups"] += 1
            if m in self.entries:
                self.st["hits"] += 1
                hit[m], slot[m] = True, self.entries[m]
                self.pins[slot[m]] += 1
                self.entries.move_to_end(m)
            else:
                self.st["misses"] += 1
                hit[m] = False
                if self.free:
                    slot[m] = self.free.pop()
                    self.taken.add(slot[m])
                else:
                    slot[m] = None
                    self.st["bypassed"] += 1
        self.calls[t] = dict(groups=groups, distinct=distinct, hit=hit, slot=slot, epoch=self.epoch)
        return self.calls[t]

    def fin(self, t, seg_ok):
        c = self.calls.pop(t)
        for m in c["distinct"]:
            if c["hit"][m]:
                s = c["slot"][m]
                self.pins[s] -= 1
                if self.pins[s] == 0 and s in self.zombie:
                    self.zombie.discard(s)
                    self.free.append(s)
        for m in c["distinct"]:
            s = c["slot"][m]
            if c["hit"][m] or s is None:
                continue
            self.taken.discard(s)
            ok = any(seg_ok[seg] for seg, gm in c["groups"] if gm == m) and c["epoch"] == self.epoch
            if not ok or m in self.entries:
                self.free.append(s)
                continue
            if len(self.entries) == self.slots:
                victim = next((v for v, vs in self.entries.items() if self.pins[vs] == 0), None)
                if victim is None:
                    self.st["bypassed"] += 1
                    self.free.append(s)
                    continue
                self.free.append(self.entries.pop(victim))
                self.st["evictions"] += 1
            self.entries[m] = s
            self.st["published"] += 1

    def clear(self):
        self.epoch += 1
        for m, s in self.entries.items():
            if self.pins[s]:
                self.zombie.add(s)
        self.entries.clear()
        busy = self.zombie | self.taken
        self.free = [s for s in range(self.total - 1, -1, -1) if s not in busy]


def check_plan(r, c, seg_off, ids):
    """The program's plan line against the model's call and the plan's own invariants."""
    n = len(ids)
    groups, distinct = c["groups"], c["distinct"]
    assert (r["U"], r["D"]) == (len(groups), len(distinct))
    assert r["ids"] == distinct
    assert r["hit"] == [int(c["hit"][m]) for m in distinct]
    assert r["slot"] == [c["slot"][m] for m in distinct]
    miss_groups = [g for g, (_, m) in enumerate(groups) if not c["hit"][m]]
    hit_groups = [g for g, (_, m) in enumerate(groups) if c["hit"][m]]
    assert r["M"] == len(miss_groups)
    # pairs: the misses [0, M) and the hits [M, U), each in group order
    pair_of = r["pair_of"]
    assert [pair_of[g] for g in miss_groups] == list(range(r["M"]))
    assert [pair_of[g] for g in hit_groups] == list(range(r["M"], r["U"]))
    assert r["miss_ids"] == [groups[g][1] for g in miss_groups]
    assert r["hit_slot"] == [c["slot"][groups[g][1]] for g in hit_groups]
    # one store per missed message that has a slot, from the pair of its first group
    stores = {}
    for g in miss_groups:
        m = groups[g][1]
        if c["slot"][m] is not None and m not in stores:
            stores[m] = (pair_of[g], c["slot"][m])
    assert list(zip(r["store_pair"], r["store_slot"])) == list(stores.values())
    # the CSR in pair order holds every set once, under its own (segment, message)
    off, sets = r["csr"][:r["U"] + 1], r["csr"][r["U"] + 1:]
    assert off[0] == 0 and off[-1] == n and sorted(sets) == list(range(n))
    for g, (seg, m) in enumerate(groups):
        members = sets[off[pair_of[g]]:off[pair_of[g] + 1]]
        assert members == [i for i in range(seg_off[seg], seg_off[seg + 1]) if ids[i] == m]


def check_state(r, model):
    assert r["stats"] == model.st
    assert r["stats"]["lookups"] == r["stats"]["hits"] + r["stats"]["misses"]
    assert r["entries"] == len(model.entries) <= model.slots
    got = {mid: k for k, (st, _, mid) in enumerate(r["slots"]) if st == ENTRY}
    assert got == dict(model.entries)  # a message has at most one entry, at the model's slot
    assert len(got) == sum(1 for st, _, _ in r["slots"] if st == ENTRY)
    assert r["lru"] == [model.entries[m] for m in reversed(model.entries)]
    for k, (st, pins, _) in enumerate(r["slots"]):
        assert pins == model.pins[k]
        assert (st == ZOMBIE) == (k in model.zombie) and (st == TAKEN) == (k in model.taken)
        if pins:
            assert st in (ENTRY, ZOMBIE)  # a pinned slot is never free and never handed out


@pytest.mark.parametrize("seed", range(12))
def test_random_operations_against_the_model(exe, tmp_path, seed):
    rng = random.Random(seed)
    slots, spare, nmsg = rng.randint(2, 16), rng.randint(1, 6), rng.randint(1, 40)
    lines, ops = ["cfg %d %d" % (slots, spare)], [("cfg",)]
    open_calls, next_t = {}, 0
    for _ in range(120):
        x = rng.random()
        if x < 0.45 and len(open_calls) < 4:
            nseg = rng.randint(1, 3)
            sizes = [rng.randint(0 if nseg > 1 else 1, 6) for _ in range(nseg)]
            if sum(sizes) == 0:
                sizes[0] = 1
            seg_off = [0]
            for s in sizes:
                seg_off.append(seg_off[-1] + s)
            hot = rng.sample(range(nmsg), min(nmsg, rng.randint(1, 8)))
            ids = [rng.choice(hot) for _ in range(seg_off[-1])]
            lines.append("plan %d %d %s %s" % (next_t, nseg, " ".join(map(str, seg_off)), " ".join(map(str, ids))))
            ops.append(("plan", next_t, seg_off, ids))
            open_calls[next_t] = nseg
            next_t += 1
        elif x < 0.93 and open_calls:
            t = rng.choice(list(open_calls))
            ok = [int(rng.random() < 0.7) for _ in range(open_calls.pop(t))]
            lines.append("fin %d %s" % (t, " ".join(map(str, ok))))
            ops.append(("fin", t, ok))
        elif x >= 0.93:
            lines.append("clear")
            ops.append(("clear",))
    for t, nseg in open_calls.items():  # every call ends
        lines.append("fin %d %s" % (t, " ".join(["1"] * nseg)))
        ops.append(("fin", t, [1] * nseg))
    text = run_script(exe, tmp_path, lines)
    assert run_script(exe, tmp_path, lines) == text  # two runs (two process keys): identical output
    out = text.splitlines()
    assert len(out) == len(ops)
    model = Model(slots, spare)
    for line, op in zip(out, ops):
        r = parse(line)
        assert r["op"] == op[0]
        if op[0] == "plan":
            before = set(model.entries.values())
            pinned = {k for k in range(model.total) if model.pins[k]}
            c = model.plan(op[1], op[2], op[3])
            check_plan(r, c, op[2], op[3])
            handed = {c["slot"][m] for m in c["distinct"] if not c["hit"][m]} - {None}
            assert not handed & before and not handed & pinned  # an entry's slot is never handed out
        elif op[0] == "fin":
            n_before = len(model.entries)
            model.fin(op[1], op[2])
            if not any(op[2]):
                assert r["entries"] == n_before  # a failed call leaves the entry count unchanged
        elif op[0] == "clear":
            model.clear()
            assert r["entries"] == 0
        check_state(r, model)
    final = parse(out[-1])
    assert all(pins == 0 and st in (FREE, ENTRY) for st, pins, _ in final["slots"])  # nothing leaks


def test_published_entry_is_found_and_failed_call_is_not(exe, tmp_path):
    lines = ["cfg 2 1", "plan 0 1 0 2 7 7", "fin 0 1", "plan 1 1 0 1 7", "fin 1 1", "plan 2 1 0 1 9", "fin 2 0",
             "plan 3 1 0 1 9", "fin 3 1"]
    out = [parse(x) for x in run_script(exe, tmp_path, lines).splitlines()]
    assert out[1]["hit"] == [0] and out[1]["U"] == 1 and out[1]["csr"] == [0, 2, 0, 1]
    assert out[2]["stats"]["published"] == 1
    assert out[3]["hit"] == [1] and out[3]["slot"] == out[1]["slot"]  # found by its next lookup
    assert out[6]["stats"]["published"] == 1 and out[6]["entries"] == 1  # the failed call published nothing
    assert out[7]["hit"] == [0]
    assert out[8]["entries"] == 2


def test_in_flight_duplicates_pins_and_no_spare(exe, tmp_path):
    lines = ["cfg 2 1",
             "plan 0 1 0 1 5",        # takes the first free slot
             "plan 1 1 0 1 5",        # the same message in flight: a plain miss, its own slot
             "fin 0 1", "fin 1 1",    # the second publication is a no-op that returns its slot
             "plan 2 1 0 1 6", "fin 2 1",          # the table is full: 5 and 6
             "plan 3 1 0 1 5",                     # pins 5
             "plan 5 1 0 1 6", "fin 5 1",          # 6 is now the most recently used
             "plan 4 2 0 1 2 7 8",                 # two misses, one free slot: the second is bypassed
             "fin 4 1 1",                          # 7 evicts 6: 5 is older, but pinned
             "fin 3 1"]
    out = [parse(x) for x in run_script(exe, tmp_path, lines).splitlines()]
    assert out[1]["slot"] != out[2]["slot"] and out[2]["hit"] == [0]
    assert out[4]["entries"] == 1 and out[4]["stats"]["published"] == 1
    assert out[9]["lru"] == [out[8]["slot"][0], out[7]["slot"][0]]
    assert out[10]["slot"][1] is None and out[10]["stats"]["bypassed"] == 1
    assert out[10]["store_slot"] == out[10]["slot"][:1]
    ids = {mid for st, _, mid in out[11]["slots"] if st == ENTRY}
    assert ids == {5, 7} and out[11]["stats"]["evictions"] == 1
    assert all(p == 0 for _, p, _ in out[12]["slots"])
