"""CPU: bls.MessageCache, the Python mirror of include/grandine_bls_gpu_msgcache.h, with the engine
stubbed: every method makes the one engine call it stands for, without initialising a device,
checks its argument first, turns a failure into an exception and names the counters."""
import ctypes

import pytest

from grandine_amd import _lib as G
from grandine_amd import bls


class Stub:
    """Stands for the loaded library: records the four calls and answers like the engine."""

    def __init__(self):
        self.calls = []
        self.n = 0
        self.fail = None

    def _rc(self, name):
        return 5 if self.fail == name else 0

    def gbls_msgcache_configure(self, slots):
        self.calls.append(("configure", slots))
        if self._rc("configure") == 0:
            self.n = slots
        return self._rc("configure")

    def gbls_msgcache_slots(self):
        self.calls.append(("slots",))
        return self.n

    def gbls_msgcache_clear(self):
        self.calls.append(("clear",))
        return self._rc("clear")

    def gbls_msgcache_stats(self, out):
        self.calls.append(("stats",))
        for i in range(8):
            out[i] = 10 + i
        out[7] = 0
        return self._rc("stats")

    def gbls_last_error(self):
        return 101


@pytest.fixture
def stub(monkeypatch):
    s = Stub()
    monkeypatch.setattr(G, "load_library", lambda: s)

    def no_device(*a, **k):
        raise AssertionError("MessageCache must not initialise a device")

    monkeypatch.setattr(G, "lib", lambda *a, **k: s if s.fail else no_device())
    return s


def test_configure_slots_clear(stub):
    bls.MessageCache.configure(4096)
    assert bls.MessageCache.slots() == 4096
    bls.MessageCache.clear()
    bls.MessageCache.configure(0)
    assert bls.MessageCache.slots() == 0
    assert stub.calls == [("configure", 4096), ("slots",), ("clear",), ("configure", 0), ("slots",)]


def test_configure_checks_its_argument_first(stub):
    for bad in (-1, (1 << 20) + 1):
        with pytest.raises(ValueError):
            bls.MessageCache.configure(bad)
    assert stub.calls == []
    bls.MessageCache.configure(1 << 20)
    assert stub.calls == [("configure", 1 << 20)] and bls.MessageCache.MAX_SLOTS == 1 << 20


def test_stats_names_the_counters(stub):
    st = bls.MessageCache.stats()
    assert st == {"lookups": 10, "hits": 11, "misses": 12, "published": 13, "evictions": 14, "bypassed": 15,
                  "entries": 16}
    assert tuple(st) == G.MSGCACHE_STATS[:7]


@pytest.mark.parametrize("name", ["configure", "clear", "stats"])
def test_engine_failures_raise(stub, name):
    stub.fail = name
    with pytest.raises(G.EngineUnavailable):
        {"configure": lambda: bls.MessageCache.configure(8), "clear": bls.MessageCache.clear,
         "stats": bls.MessageCache.stats}[name]()


def test_memory_cost():
    assert bls.MessageCache.BYTES_PER_SLOT == 19584 == 68 * 72 * ctypes.sizeof(ctypes.c_uint32)
    assert bls.MessageCache.memory_bytes(0) == 0
    assert bls.MessageCache.memory_bytes(16) == (16 + 64) * 19584  # at least 64 spare slots
    assert bls.MessageCache.memory_bytes(4096) == (4096 + 1024) * 19584  # a quarter
    assert bls.MessageCache.memory_bytes(1 << 20) == ((1 << 20) + 4096) * 19584  # at most 4096
