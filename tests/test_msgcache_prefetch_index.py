"""CPU: the host side of gbls_msgcache_prefetch and of the per-check plan
(grandine_amd/csrc/gbls_msgcache_checks.h) through a stand-alone program
(tests/native/msgcache_prefetch_main.cpp), built plain and with AddressSanitizer and UBSan, against
a Python dict-plus-LRU model of two engines: the status rules, duplicates within a call, the spare
limit, eviction order, the two-engine merge rule, a failed call, and per-check plans with repeated
messages over hits and misses."""
import collections
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "msgcache_prefetch_main.cpp")
BUILD = os.path.join(ROOT, "tests", "native", "_build")
STATS = ("lookups", "hits", "misses", "published", "evictions", "bypassed")
ENTERED, PRESENT, SKIPPED = 0, 1, 2


@pytest.fixture(scope="module", params=["plain", "san"])
def exe(request):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "msgcache_prefetch_main_" + request.param)
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fno-omit-frame-pointer",
                                                      "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", out, SRC])
    return out


def run_script(exe, tmp_path, lines):
    path = str(tmp_path / "script.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.splitlines()


def parse_state(text):
    tok = text.split()
    lru, busy = tok.index("lru"), tok.index("busy")
    return dict(entries=int(tok[1]), stats=dict(zip(STATS, (int(x) for x in tok[3:9]))),
                lru=[int(x) for x in tok[lru + 1:busy]], busy=int(tok[busy + 1]), pins=int(tok[busy + 3]))


def parse(line):
    head, s0, s1 = line.split(" | ")
    r = {"op": head.split()[0], "state": [parse_state(s0), parse_state(s1)]}
    parts = [p.strip() for p in head.split(";") if p.strip()]
    tok = parts[0].split()
    if r["op"] == "prefetch":
        r["D"] = int(tok[2])
        parts[0] = " ".join(tok[3:])
    elif r["op"] == "checks":
        r.update(U=int(tok[4]), M=int(tok[6]), C=int(tok[8]), D=int(tok[10]))
        parts[0] = " ".join(tok[11:])
    else:
        parts = []
    for part in parts:
        name, *vals = part.split()
        r[name] = [None if v == "-1" else int(v) for v in vals]
    return r


class Model:
    """One engine: dict + LRU (last = most recently used), pins per entry, slots taken by calls."""

    def __init__(self, slots, spare):
        self.slots, self.total = slots, slots + spare
        self.entries = collections.OrderedDict()
        self.pins = collections.Counter()
        self.taken = 0
        self.st = dict.fromkeys(STATS, 0)
        self.calls = {}

    def lookup(self, distinct, limit=None):
        hit, has_slot = {}, {}
        for m in distinct:
            self.st["lookups"] += 1
            if m in self.entries:
                self.st["hits"] += 1
                hit[m] = True
                self.pins[m] += 1
                self.entries.move_to_end(m)
            else:
                self.st["misses"] += 1
                hit[m] = False
                free = self.total - len(self.entries) - self.taken
                if free > 0 and (limit is None or limit > 0):
                    has_slot[m] = True
                    self.taken += 1
                    if limit is not None:
                        limit -= 1
                else:
                    has_slot[m] = False
                    self.st["bypassed"] += 1
        return hit, has_slot

    def finish(self, distinct, hit, has_slot, ok):
        """ok: message -> publish it.  Returns the messages that were entries right after their turn."""
        for m in distinct:
            if hit[m]:
                self.pins[m] -= 1
        entered = set()
        for m in distinct:
            if hit[m] or not has_slot[m]:
                continue
            self.taken -= 1
            if not ok.get(m):
                continue
            if m not in self.entries:
                if len(self.entries) == self.slots:
                    victim = next((v for v in self.entries if self.pins[v] == 0), None)
                    if victim is None:
                        self.st["bypassed"] += 1
                        continue
                    del self.entries[victim]
                    self.st["evictions"] += 1
                self.entries[m] = True
                self.st["published"] += 1
            entered.add(m)
        return entered

    def clear(self):
        assert not self.calls
        self.entries.clear()


def check_state(r, models):
    for st, m in zip(r["state"], models):
        assert st["stats"] == m.st
        assert st["stats"]["lookups"] == st["stats"]["hits"] + st["stats"]["misses"]
        assert st["entries"] == len(m.entries) <= m.slots
        assert st["lru"] == list(reversed(m.entries))
        assert st["busy"] == len(m.entries) + m.taken and st["pins"] == sum(m.pins.values())


def model_prefetch(models, limit, engines, done, ids):
    distinct = list(dict.fromkeys(ids))
    looked = [models[k].lookup(distinct, limit) for k in range(engines)]
    merged = {}
    fills = []
    for k in range(engines):
        hit, has_slot = looked[k]
        fills.append(sum(1 for m in distinct if not hit[m] and has_slot[m]))
        entered = models[k].finish(distinct, hit, has_slot, {m: bool(done) for m in distinct})
        for m in distinct:
            s = PRESENT if hit[m] else ENTERED if m in entered else SKIPPED
            if m not in merged:
                merged[m] = s
            elif SKIPPED in (merged[m], s):
                merged[m] = SKIPPED
            elif ENTERED in (merged[m], s):
                merged[m] = ENTERED
    if not done:
        merged = dict.fromkeys(distinct, SKIPPED)
    return [merged[m] for m in ids], fills, len(distinct)


def check_checks(r, model, t, ids):
    n = len(ids)
    distinct = list(dict.fromkeys(ids))
    hit, has_slot = model.lookup(distinct)
    model.calls[t] = (ids, distinct, hit, has_slot)
    assert (r["U"], r["D"]) == (n, len(distinct)) and r["ids"] == distinct
    assert r["hit"] == [int(hit[m]) for m in distinct]
    assert [s is not None for s in r["slot"]] == [hit[m] or has_slot[m] for m in distinct]
    slot = dict(zip(distinct, r["slot"]))
    taken = [slot[m] for m in distinct if not hit[m] and has_slot[m]]
    assert len(set(taken)) == len(taken)
    first = {m: ids.index(m) for m in distinct}
    gen = [q for q in range(n) if not hit[ids[q]] and (not has_slot[ids[q]] or first[ids[q]] == q)]
    hits = [q for q in range(n) if hit[ids[q]]]
    copies = [q for q in range(n) if not hit[ids[q]] and has_slot[ids[q]] and first[ids[q]] != q]
    assert (r["M"], r["C"]) == (len(gen), len(copies))
    # pairs: generated lines, then the entries' lines, then copies of this call's own stores
    assert [r["pair_of"][q] for q in gen + hits + copies] == list(range(n))
    assert r["miss_ids"] == [ids[q] for q in gen]  # a missed message with a slot is hashed once
    assert r["hit_slot"] == [slot[ids[q]] for q in hits + copies]
    stores = [(r["pair_of"][q], slot[ids[q]]) for q in gen if has_slot[ids[q]]]
    assert list(zip(r["store_pair"], r["store_slot"])) == stores
    assert {s for _, s in stores} >= {slot[ids[q]] for q in copies}  # every copy's slot is stored by this call
    inv = sorted(range(n), key=lambda q: r["pair_of"][q])
    assert r["csr"] == list(range(n + 1)) + inv


@pytest.mark.parametrize("seed", range(10))
def test_random_operations_against_the_model(exe, tmp_path, seed):
    rng = random.Random(seed)
    slots, spare, nmsg = rng.randint(2, 8), rng.randint(1, 5), rng.randint(2, 24)
    lines, ops = ["cfg %d %d" % (slots, spare)], [("cfg",)]
    open_calls = [{}, {}]
    next_t = 0
    for _ in range(100):
        x = rng.random()
        if x < 0.4:
            ids = [rng.randrange(nmsg) for _ in range(rng.randint(1, 10))]
            op = ("prefetch", rng.randint(0, spare + 1), rng.randint(1, 2), int(rng.random() < 0.85), ids)
            lines.append("prefetch %d %d %d %s" % (op[1], op[2], op[3], " ".join(map(str, ids))))
            ops.append(op)
        elif x < 0.65 and sum(map(len, open_calls)) < 3:
            e = rng.randint(0, 1)
            hot = rng.sample(range(nmsg), min(nmsg, rng.randint(1, 4)))
            ids = [rng.choice(hot) for _ in range(rng.randint(1, 9))]
            lines.append("checks %d %d %s" % (e, next_t, " ".join(map(str, ids))))
            ops.append(("checks", e, next_t, ids))
            open_calls[e][next_t] = len(ids)
            next_t += 1
        elif x < 0.95 and (open_calls[0] or open_calls[1]):
            e = 0 if open_calls[0] and (not open_calls[1] or rng.random() < 0.5) else 1
            t = rng.choice(list(open_calls[e]))
            ok = [int(rng.random() < 0.6) for _ in range(open_calls[e].pop(t))]
            lines.append("fin %d %d %s" % (e, t, " ".join(map(str, ok))))
            ops.append(("fin", e, t, ok))
        elif x >= 0.95:
            e = rng.randint(0, 1)
            if not open_calls[e]:
                lines.append("clear %d" % e)
                ops.append(("clear", e))
    for e in range(2):
        for t, n in open_calls[e].items():
            lines.append("fin %d %d %s" % (e, t, " ".join(["1"] * n)))
            ops.append(("fin", e, t, [1] * n))
    out = run_script(exe, tmp_path, lines)
    assert len(out) == len(ops)
    models = [Model(slots, spare), Model(slots, spare)]
    for line, op in zip(out, ops):
        r = parse(line)
        assert r["op"] == op[0]
        if op[0] == "prefetch":
            status, fills, D = model_prefetch(models, op[1], op[2], op[3], op[4])
            assert (r["status"], r["fills"], r["D"]) == (status, fills, D)
            ids = op[4]
            assert all(status[i] == status[ids.index(m)] for i, m in enumerate(ids))  # duplicates agree
            assert all(f <= op[1] for f in fills)
        elif op[0] == "checks":
            check_checks(r, models[op[1]], op[2], op[3])
        elif op[0] == "fin":
            ids, distinct, hit, has_slot = models[op[1]].calls.pop(op[2])
            ok = {m: any(op[3][q] for q in range(len(ids)) if ids[q] == m) for m in distinct}
            models[op[1]].finish(distinct, hit, has_slot, ok)
        elif op[0] == "clear":
            models[op[1]].clear()
        check_state(r, models)
    final = parse(out[-1])
    assert all(st["pins"] == 0 and st["busy"] == st["entries"] for st in final["state"])  # nothing leaks


def test_status_rules_duplicates_and_limit(exe, tmp_path):
    out = [parse(x) for x in run_script(exe, tmp_path, [
        "cfg 4 2",
        "prefetch 2 1 1 7 8 7",       # a duplicate: handled once, both occurrences ENTERED
        "prefetch 2 1 1 8 9 10 11",   # 8 present; 9 10 taken (the limit); 11 beyond it
        "prefetch 2 1 0 12 13",       # the device work failed: nothing entered, the slots returned
        "prefetch 2 1 1 12 13",       # the table is full (7 8 9 10): the least recently used go
    ])]
    assert out[1]["status"] == [ENTERED, ENTERED, ENTERED] and out[1]["D"] == 2 and out[1]["fills"] == [2]
    assert out[2]["status"] == [PRESENT, ENTERED, ENTERED, SKIPPED]
    assert out[2]["state"][0]["stats"]["bypassed"] == 1 and out[2]["state"][0]["entries"] == 4
    assert out[3]["status"] == [SKIPPED, SKIPPED] and out[3]["state"][0]["entries"] == 4
    assert out[3]["state"][0]["busy"] == 4 and out[3]["state"][0]["stats"]["published"] == 4
    assert out[4]["status"] == [ENTERED, ENTERED] and out[4]["state"][0]["lru"] == [13, 12, 10, 9]
    assert out[4]["state"][0]["stats"]["evictions"] == 2


def test_more_roots_than_capacity_in_one_call(exe, tmp_path):
    out = [parse(x) for x in run_script(exe, tmp_path, ["cfg 4 8", "prefetch 8 1 1 0 1 2 3 4 5",
                                                        "prefetch 8 1 1 2 3 4 5", "prefetch 8 1 1 0 1"])]
    assert out[1]["status"] == [ENTERED] * 6 and out[1]["state"][0]["entries"] == 4
    assert out[1]["state"][0]["stats"]["evictions"] == 2
    assert out[2]["status"] == [PRESENT] * 4 and out[3]["status"] == [ENTERED] * 2


def test_two_engine_merge_rule(exe, tmp_path):
    out = [parse(x) for x in run_script(exe, tmp_path, [
        "cfg 2 1",
        "prefetch 1 1 1 5",      # engine 0 only
        "prefetch 1 2 1 5",      # present on 0, missing on 1: ENTERED
        "prefetch 1 2 1 5",      # present on both
        "checks 1 0 6 7",        # engine 1: 6 and 7 take its last two slots and keep them in flight
        "prefetch 1 2 1 8",      # engine 0 enters 8, engine 1 has no slot to spare: SKIPPED
        "fin 1 0 0 0",
        "prefetch 1 2 1 8",      # present on 0, entered on 1
    ])]
    assert out[1]["status"] == [ENTERED] and out[2]["status"] == [ENTERED] and out[3]["status"] == [PRESENT]
    assert out[2]["fills"] == [0, 1]
    assert None not in out[4]["slot"] and out[4]["state"][1]["busy"] == 3
    assert out[5]["status"] == [SKIPPED] and [s["entries"] for s in out[5]["state"]] == [2, 1]
    assert out[7]["status"] == [ENTERED] and [s["entries"] for s in out[7]["state"]] == [2, 2]


def test_per_check_plan_hashes_a_missed_message_once(exe, tmp_path):
    out = [parse(x) for x in run_script(exe, tmp_path, [
        "cfg 8 4",
        "prefetch 4 1 1 1",
        "checks 0 0 2 1 2 3 1 2",     # 1 hits; 2 (three checks) and 3 miss
        "fin 0 0 0 1 0 0 0 1",        # a check of 2 passed, 3's did not
        "checks 0 1 3 2",
        "fin 0 1 1 1",
    ])]
    p = out[2]
    assert (p["U"], p["M"], p["C"], p["D"]) == (6, 2, 2, 3) and p["miss_ids"] == [2, 3]
    assert p["pair_of"] == [0, 2, 4, 1, 3, 5] and len(p["store_pair"]) == 2
    assert out[3]["state"][0]["lru"] == [2, 1] and out[3]["state"][0]["stats"]["published"] == 2
    assert out[4]["hit"] == [0, 1]
