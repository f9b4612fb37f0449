"""The host arithmetic that keeps a tally and an append of ``ResidentChain`` away from the sticky
PZ_ERANGE under ``"grow"`` / ``"retire"`` (prysm_amd/blockchain.py: ``_CacheRoom``, ``_PoolRoom``),
driven directly with fake handles that record every call and keep the true occupancy.  The
invariant: a bound never falls below the truth, so that what fits the bound fits the handle.  The
expected calls come from a model restated here from ``ResidentChain``'s text.  No GPU needed: the
steps that queue device work are not run."""
import random

import numpy as np
import pytest

from prysm_amd.blockchain import _CacheRoom, _PoolRoom

SEEDS = range(6)


class Log:
    """A run's hash log: ``ids[j]`` stands for the 32 bytes of entry j."""

    def __init__(self, ids):
        self.ids = list(ids)

    def __getitem__(self, s):
        assert s.start is None and s.step is None and s.stop % 32 == 0
        return Log(self.ids[:s.stop // 32])


class FakeCache:
    """A vote cache as the policy sees it.  Its entries: ``keys`` (log hashes, by id) and ``other``
    (a count of entries under hashes no log holds: what was there before, and oblique hashes)."""

    def __init__(self, slot_cap, other=0):
        self.slot_cap, self.keys, self.other, self.calls = slot_cap, set(), other, []
        self.reserves = []  # (capacity before, argument) of every reserve

    def entries(self):
        return len(self.keys) + self.other

    def read(self, strict=True):
        self.calls.append(("read", strict))
        return None, range(self.entries())

    def retain(self, log):
        self.calls.append(("retain", len(log.ids)))
        self.keys &= set(log.ids)
        self.other = 0

    def reserve(self, min_slots, device_form=False):
        self.calls.append(("reserve", min_slots, device_form))
        self.reserves.append((self.slot_cap, min_slots))
        self.slot_cap = max(self.slot_cap, min_slots)

    def tally(self, log, oblique):
        """The worst a tally can do: every log hash and every oblique element a new entry.  A real
        one that met more entries than slots would land nothing and set PZ_ERANGE."""
        self.keys |= set(log.ids)
        self.other += oblique
        assert self.entries() <= self.slot_cap, "PZ_ERANGE"


class FakePool:
    """A pending pool as the policy sees it: seven capacities and the seven true counts ``n``."""

    def __init__(self, caps, counts=None):
        self.caps, self.n, self.calls = list(caps), list(counts or [0] * 7), []

    def counts(self, strict=True):
        self.calls.append(("counts", strict))
        return np.array(self.n, dtype=np.uint64)

    def reserve(self, min_caps, device_form=False):
        self.calls.append(("reserve", list(min_caps), device_form))
        self.caps = [max(c, m) for c, m in zip(self.caps, min_caps)]

    def append(self, need):
        """A real append that met a count above its capacity would land nothing and set PZ_ERANGE."""
        self.n = [a + b for a, b in zip(self.n, need)]
        assert all(a <= c for a, c in zip(self.n, self.caps)), "PZ_ERANGE"


class Untouchable:
    """A handle under ``"fixed"``: any use of it is recorded and refused."""

    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        self.seen.append(name)
        raise AssertionError("the handle was asked for %s" % name)


def cache_script(rng, nruns):
    """Seeded runs, ``(ncand, [oblique per landing], panic)``: ncand 0 rolls nothing and 70 is a
    full cycle and more; a run lands before stateRecalc and, with a transition block, behind it;
    a run without rows lands nothing; a panicked run lands nothing either."""
    for _ in range(nruns):
        ncand = rng.choice([0, 0, 1, 2, 7, 70, rng.randrange(71)])
        landings = rng.choice([0, 1, 1, 2, 2])
        yield ncand, [rng.choice([0, 0, 1, 5, 300]) for _ in range(landings)], rng.random() < 0.15


def drive_cache(policy, slot_cap, other, script):
    """Drives a ``_CacheRoom`` as ``ResidentChain`` does and checks it at every landing against the
    class text: the bound starts at the entries the cache holds; a landing can add the run's hash
    log -- without the ring's 129 where an earlier landing counted them, and once a run -- plus its
    oblique elements; where that does not fit, "retire" first retains the log, which leaves the
    log's entries at most, and a reserve follows only if it still does not fit, of at least the
    need, doubling, the doubling clipped at 2^30.  Returns the fake."""
    cache = FakeCache(slot_cap, other)
    room = _CacheRoom(cache, policy)
    assert room.extra_bytes == 16 and cache.calls == [("read", False)]
    ub, ring_counted = cache.entries(), False  # the model's bound
    ring, fresh, retains, grows = list(range(129)), 129, 0, 0
    for ncand, obliques, panic in script:
        log = Log(ring + list(range(fresh, fresh + ncand)))
        nlog = 129 + ncand
        read = np.array((obliques + [0, 0])[:2], dtype=np.uint64).view(np.uint8)
        assert room.parse(read) == (obliques + [0, 0])[:2]
        if panic:  # nothing lands and nothing rolls: the driver reads, parses and leaves
            continue
        fresh += ncand
        room.begin()
        run_counted = False
        for oblique in obliques:
            need = oblique + (0 if run_counted else nlog - (129 if ring_counted else 0))
            cap, want = cache.slot_cap, []
            if ub + need > cap:
                if policy == "retire":
                    want.append(("retain", nlog))
                    ub, need = nlog, oblique
                if ub + need > cap:
                    want.append(("reserve", max(ub + need, min(2 * cap, 1 << 30)), True))
            ub += need
            run_counted = True
            del cache.calls[:]
            room.fit(oblique, nlog, log)
            assert cache.calls == want
            retains += sum(c[0] == "retain" for c in want)
            grows += sum(c[0] == "reserve" for c in want)
            assert cache.slot_cap > cap or want[-1:] in ([], [("retain", nlog)])  # every reserve raised the capacity
            cache.tally(log, oblique)  # asserts that it fits
            assert room.slots_ub >= cache.entries()
        room.end(ncand)
        ring_counted = run_counted or (ring_counted and ncand == 0)
        ring = log.ids[ncand:ncand + 129]
    assert (room.retains, room.grows) == (retains, grows)
    return cache


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("policy", ["grow", "retire"])
def test_cache_bound_from_one_slot(policy, seed):
    cache = drive_cache(policy, 1, 0, cache_script(random.Random(seed), 60))
    assert cache.reserves and cache.reserves[0][0] == 1


@pytest.mark.parametrize("policy", ["grow", "retire"])
def test_cache_reserve_clips_the_doubling(policy):
    """From 2^29 slots the doubling stops at 2^30, and from there a reserve asks for the need alone."""
    script = [(3, [7, (1 << 29) + 9], False), (0, [1 << 30], False)]
    cache = drive_cache(policy, 1 << 29, (1 << 29) - 5, script)
    assert cache.reserves[0] == (1 << 29, 1 << 30) and len(cache.reserves) > 1
    assert all(cap >= 1 << 30 and cap < arg < 2 * cap for cap, arg in cache.reserves[1:])


def pool_script(rng, nruns):
    """Seeded runs, ``([need per landing], panic, prune)``; ``prune``: stateRecalc's prune lowers
    the pool's counts behind the run."""
    for _ in range(nruns):
        landings = rng.choice([0, 1, 1, 2, 2])
        yield [[rng.choice([0, 0, 1, 3, 40]) for _ in range(7)] for _ in range(landings)], rng.random() < 0.15, rng.random() < 0.3


def drive_pool(caps, counts, script, rng):
    """Drives a ``_PoolRoom`` as ``ResidentChain`` does and checks it against the class text: the
    bounds start at the pool's counts; where bound + need exceeds a capacity they are first read
    again (a prune leaves them stale upward), and if they still do not fit each short column is
    reserved to ``max(bound + need, 2 * capacity)``, clipped at 2^40 - 1.  Returns the fake."""
    pool = FakePool(caps, counts)
    room = _PoolRoom(pool, "grow")
    assert room.extra_bytes == 112 and pool.calls == [("counts", False)]
    ub, grows = list(pool.n), 0  # the model's bounds
    for needs, panic, prune in script:
        read = np.array((needs + [[0] * 7] * 2)[:2], dtype=np.uint64).view(np.uint8).reshape(-1)
        assert room.parse(read) == (needs + [[0] * 7] * 2)[:2]
        if panic:  # nothing lands: the driver reads, parses and leaves
            continue
        for need in needs:
            cap, want = list(pool.caps), []
            if any(u + a > c for u, a, c in zip(ub, need, cap)):
                want.append(("counts", False))
                ub = list(pool.n)
                to = [u + a for u, a in zip(ub, need)]
                if any(t > c for t, c in zip(to, cap)):
                    want.append(("reserve", [min(max(t, 2 * c), (1 << 40) - 1) if t > c else c for t, c in zip(to, cap)], True))
                    grows += 1
            ub = [u + a for u, a in zip(ub, need)]
            del pool.calls[:]
            room.fit(need)
            assert pool.calls == want
            assert len(want) < 2 or any(a > b for a, b in zip(pool.caps, cap))  # every reserve raised a capacity
            pool.append(need)  # asserts that it fits
            assert all(u >= n for u, n in zip(room.counts_ub, pool.n))
        if prune:
            pool.n = [rng.randrange(n + 1) for n in pool.n]
    assert room.grows == grows
    return pool


@pytest.mark.parametrize("seed", SEEDS)
def test_pool_bound_from_one_entry(seed):
    rng = random.Random(seed)
    pool = drive_pool([1] * 7, None, pool_script(rng, 60), rng)
    assert max(pool.caps) > 1


def test_pool_reserve_clips_at_2_40():
    """From 2^39 entries the doubling stops at 2^40 - 1; a column that is not short keeps its capacity."""
    at = (1 << 39) - 3
    pool = drive_pool([1 << 39] * 7, [at] * 7, [([[10, 3, 10, 0, 10, 10, 10]], False, False)], None)
    assert pool.caps == [(1 << 40) - 1, 1 << 39, (1 << 40) - 1, 1 << 39] + [(1 << 40) - 1] * 3


def test_a_panicked_run_moves_nothing():
    """With the gate's panic bit the driver parses the read and leaves: no bound, flag or counter moves."""
    cache, pool = FakeCache(4), FakePool([1] * 7)
    rooms = [_CacheRoom(cache, "retire"), _PoolRoom(pool, "grow")]
    before = [dict(vars(r)) for r in rooms]
    del cache.calls[:], pool.calls[:]
    rooms[0].parse(np.ones(16, np.uint8))
    rooms[1].parse(np.ones(112, np.uint8))
    assert [dict(vars(r)) for r in rooms] == before and cache.calls == [] and pool.calls == []


def test_fixed_asks_for_nothing():
    handle = Untouchable()
    cache, pool = _CacheRoom(handle, "fixed"), _PoolRoom(handle, "fixed")
    assert cache.extra_bytes == 0 and pool.extra_bytes == 0
    empty = np.zeros(0, np.uint8)
    cache.queue(empty, None, None)
    pool.queue(empty, None, 3, None, None)
    oblique, need = cache.parse(empty), pool.parse(empty)
    cache.begin()
    for phase in (0, 1):
        cache.fit(oblique[phase], 129 + 70, handle)
        pool.fit(need[phase])
    cache.end(70)
    assert handle.seen == []
    assert (cache.retains, cache.grows, pool.grows) == (0, 0, 0)
