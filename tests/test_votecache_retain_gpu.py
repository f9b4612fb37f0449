"""Growth and retirement of the device vote cache (prysm_amd/csrc/votecache.hip:
pz_[dev_]vote_cache_reserve, pz_[dev_]vote_cache_retain; votes.DeviceVoteCache.reserve / .retain;
blockchain.ResidentChain's cache_policy).

1. Caches filled by hand-made tallies (status, committee and parents_start set by hand; no oblique
   element) against a Python dict model -- hash -> (voter bits, total), in slot order -- filtered by
   the keep list: keys, slot ids, totals and voters bit-exact.  After every retain and reserve new
   rows are tallied and the whole map compared again, so a fresh slot that did not read zero shows.
2. The edges: reserve at or below the capacity, retain of no hash, the sticky error carried over,
   every PZ_EINVAL.
3. ResidentChain over synth.chain_blocks(1024, 330, seed=4) against oracle.replay.Chain: the default
   policy at 256 slots still ends in the capacity error, "retire" at 256 and "grow" at 64 do not."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ref
from oracle import replay as oreplay
from prysm_amd import _lib, synth, wire
from prysm_amd import blockchain as bc
from prysm_amd.pending import DevicePendingAttestations, DeviceRecentHashes, DeviceSavedBlocks
from prysm_amd.votes import DeviceVoteCache
from test_attpool_gpu import as_pb, table
from test_blockcycle_gpu import check_chain, check_outs
from test_blockwalk_gpu import CAPS
from test_votecache_gpu import put, snapshot, want

pytestmark = pytest.mark.gpu

U64 = np.uint64
PROCESSED = 0
NONE32 = 0xFFFFFFFF
E = _lib.PZ_EINVAL


# ---- the model and the hand-made tallies ------------------------------------------------------------------------
class Model:
    """calculateBlockVoteCache (core.go:300-345) for rows without oblique elements: hash -> [voter bits,
    total], a dict in insertion order, which is the cache's slot order."""

    def __init__(self, nval, rng):
        self.nval, self.rng = nval, rng
        ncomm = min(4, nval)
        perm = rng.permutation(nval).astype(np.uint32)
        cuts = np.sort(rng.choice(np.arange(1, nval), ncomm - 1, replace=False)) if ncomm > 1 else np.zeros(0, int)
        self.coffs = np.concatenate([[0], cuts, [nval]]).astype(U64)
        self.members = perm
        self.balance = rng.integers(1, 1 << 40, size=nval).astype(U64)
        self.map = {}

    def rows(self, recent, starts, p=0.5):
        """One row per entry of ``starts`` over ``recent`` ((k, 32) uint8, k >= 64): the tally's host columns.
        New hashes get their slots in ascending order of their first position in ``recent``, as the commit
        launch numbers them."""
        n = len(starts)
        used = sorted({q for s in starts for q in range(int(s), int(s) + 64)})
        for q in used:
            self.map.setdefault(recent[q].tobytes(), [np.zeros(self.nval, bool), 0])
        comm = self.rng.integers(0, len(self.coffs) - 1, size=n).astype(np.uint32)
        bits, boffs = [], [0]
        for i in range(n):
            lo, hi = int(self.coffs[comm[i]]), int(self.coffs[comm[i] + 1])
            on = self.rng.random(hi - lo) < p
            bits.append(np.packbits(on.astype(np.uint8)))  # MSB first
            boffs.append(boffs[-1] + len(bits[-1]))
            voters = self.members[lo:hi][on]
            for h in recent[int(starts[i]):int(starts[i]) + 64]:
                e = self.map[h.tobytes()]
                new = voters[~e[0][voters]]
                e[0][new] = True
                e[1] = (e[1] + int(self.balance[new].sum(dtype=U64))) & ((1 << 64) - 1)
        cols = {"attester_bitfield": np.concatenate(bits), "attester_bitfield_offs": np.array(boffs, U64)}
        return cols, n, np.full(n, PROCESSED, np.int32), comm, np.asarray(starts, U64)

    def tally(self, cache, recent, starts=None, device_form=False):
        """One tally over ``recent``; ``starts`` None: rows whose windows cover every entry."""
        k = len(recent)
        if starts is None:
            starts = list(range(0, k - 63, 64)) + [k - 64, int(self.rng.integers(0, k - 63))]
        cols, n, status, comm, pstart = self.rows(recent, starts)
        if device_form:
            cache.tally_columns({k: put(v) for k, v in cols.items()}, n, put(status), put(comm), put(pstart), put(recent),
                                put(self.members), put(self.coffs), put(self.balance))
        else:
            cache.tally_host(cols, n, status, comm, pstart, recent, self.members, self.coffs, self.balance)

    def keys(self):
        return np.frombuffer(b"".join(self.map), dtype=np.uint8).reshape(-1, 32)

    def retain(self, keep):
        keep = set(keep)
        self.map = {h: e for h, e in self.map.items() if h in keep}

    def check(self, cache):
        """Keys in slot order, slot ids, totals and voters, bit for bit."""
        hashes, totals = cache.read()
        keys = list(self.map)
        assert [h.tobytes() for h in hashes] == keys
        assert [int(t) for t in totals] == [e[1] for e in self.map.values()]
        for h, e in self.map.items():
            np.testing.assert_array_equal(cache.voters(h), np.nonzero(e[0])[0].astype(np.uint32))
        if keys:
            t, s = cache.lookup(keys)
            assert s.tolist() == list(range(len(keys))) and [int(x) for x in t] == [e[1] for e in self.map.values()]


def hashes_of(rng, n, edge=False):
    """n distinct random hashes as (n, 32) uint8; with ``edge`` the all-zero one and two whose first word is
    0xFFFFFFFF among them: their home cell is the table's last, so their probes wrap."""
    h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    if edge and n >= 3:
        h[0, :4] = h[1, :4] = 255
        h[n // 2 + 1 if n // 2 + 1 < n else 2] = 0
    assert len({r.tobytes() for r in h}) == n
    return h


def recent_over(rng, pool, k=96):
    """RecentBlockHashes of max(k, len(pool), 64) entries: the pool's hashes in a random order, then more of them."""
    k = max(k, len(pool), 64)
    return pool[np.concatenate([rng.permutation(len(pool)), rng.integers(0, len(pool), size=k - len(pool))])]


def keep_list(rng, keys, frac, absent=3):
    """A keep list over ``keys``: about ``frac`` of them, some twice, ``absent`` hashes the map lacks
    (one sharing a key's first word, so its probe walks the key's cells), shuffled."""
    kept = [k for k in keys if rng.random() < frac]
    extra = [kept[i] for i in rng.integers(0, len(kept), size=min(2, len(kept)))] if kept else []
    strangers = [rng.bytes(32) for _ in range(absent)]
    if keys and absent:
        strangers[0] = keys[0][:4] + strangers[0][4:]
    out = kept + extra + [s for s in strangers if s not in keys]
    rng.shuffle(out)
    return kept, out


def as_device(hashes):
    return put(np.frombuffer(b"".join(hashes), dtype=np.uint8).reshape(-1, 32))


def cycle_of_moves(nval, slot_cap, seed, device_form):
    """fill -> retain -> tally -> retain (back into the first buffer set, stale now) -> tally -> reserve ->
    tally -> retain after the reserve -> tally, the model compared after every step."""
    rng = np.random.default_rng(seed)
    m = Model(nval, rng)
    cache = DeviceVoteCache(nval, slot_cap)

    def retain(frac):
        kept, hashes = keep_list(rng, list(m.map), frac)
        cache.retain(as_device(hashes) if device_form else hashes)
        m.retain(kept)
        m.check(cache)

    def refill():  # new hashes take every free slot: one that does not read zero shows in the model's comparison
        room = cache.slot_cap - len(m.map)
        if room:
            m.tally(cache, recent_over(rng, np.concatenate([hashes_of(rng, room), m.keys()])), device_form=device_form)
            assert len(m.map) == cache.slot_cap
            m.check(cache)
        return room

    m.tally(cache, recent_over(rng, hashes_of(rng, slot_cap, edge=True)), device_form=device_form)
    assert len(m.map) == slot_cap  # every slot taken, every row with voters
    m.check(cache)
    retain(0.5)
    fresh = refill()
    retain(0.6)
    fresh += refill()
    assert fresh > 0 and cache.slot_cap == slot_cap
    before = list(m.map)
    grown = slot_cap + 1 + int(rng.integers(0, slot_cap + 2))
    assert cache.reserve(grown, device_form=device_form) == grown == cache.slot_cap
    assert list(m.map) == before
    m.check(cache)  # (slot ids included: every entry where it was)
    assert refill() == grown - slot_cap
    retain(0.4)
    assert refill() > 0
    return cache


# ---- 1: shapes that can break the move --------------------------------------------------------------------------
@pytest.mark.parametrize("nval,slot_cap", [(8, 4), (33, 7), (65, 9), (100, 16), (161, 33), (1024, 64), (65537, 5)])
def test_retain_and_reserve_over_row_shapes(nval, slot_cap):
    """words = 1, 2, 3, 4, 6, 32 and 2,049: rows that start at every dword phase, with and without a
    16-byte body, a head and a tail."""
    cycle_of_moves(nval, slot_cap, 100 + nval, device_form=nval % 2 == 1)


def test_renumber_past_its_tile():
    """2,500 slots at 33 validators: ten tiles of the renumber launch, the last one partial."""
    rng = np.random.default_rng(7)
    nval, slot_cap = 33, 2500
    m = Model(nval, rng)
    cache = DeviceVoteCache(nval, slot_cap)
    pool = hashes_of(rng, slot_cap)
    m.tally(cache, pool, device_form=True)
    assert len(m.map) == slot_cap
    keys = list(m.map)
    kept = [k for j, k in enumerate(keys) if rng.random() < 0.5 or j in (0, 255, 256, 257, 2499)]
    cache.retain(as_device(list(reversed(kept))))
    m.retain(kept)
    hashes, totals = cache.read()
    assert [h.tobytes() for h in hashes] == kept and [int(t) for t in totals] == [m.map[k][1] for k in kept]
    t, s = cache.lookup(keys)
    ids = {k: j for j, k in enumerate(kept)}
    assert s.tolist() == [ids.get(k, NONE32) for k in keys]
    for k in kept[:3] + kept[254:259] + kept[-3:]:
        np.testing.assert_array_equal(cache.voters(k), np.nonzero(m.map[k][0])[0].astype(np.uint32))
    new = hashes_of(rng, 128)
    m.tally(cache, new, device_form=True)
    for k in [h.tobytes() for h in new[::9]]:
        np.testing.assert_array_equal(cache.voters(k), np.nonzero(m.map[k][0])[0].astype(np.uint32))
    assert cache.items() == {k: e[1] for k, e in m.map.items()}


# ---- 2: the edges -------------------------------------------------------------------------------------------------
def small_cache(seed=3, nval=100, slot_cap=16, fill=10):
    rng = np.random.default_rng(seed)
    m = Model(nval, rng)
    cache = DeviceVoteCache(nval, slot_cap)
    m.tally(cache, recent_over(rng, hashes_of(rng, fill)))
    return rng, m, cache


@pytest.mark.parametrize("device_form", [False, True])
def test_reserve_at_or_below_the_capacity_changes_nothing(device_form):
    rng, m, cache = small_cache()
    for want_cap in (0, 1, 15, 16):
        assert cache.reserve(want_cap, device_form=device_form) == 16
    m.check(cache)
    assert cache.reserve(17, device_form=device_form) == 17
    m.check(cache)


@pytest.mark.parametrize("device_form", [False, True])
def test_retain_of_no_hash_empties_the_cache(device_form):
    import torch

    rng, m, cache = small_cache()
    cache.retain(torch.zeros((0, 32), dtype=torch.uint8, device="cuda:0") if device_form else [])
    assert cache.items() == {} and cache.slot_cap == 16
    m.retain([])
    m.tally(cache, recent_over(rng, hashes_of(rng, 16)))
    m.check(cache)


def test_the_sticky_capacity_error_is_carried_over():
    rng, m, cache = small_cache()
    kept_map = dict(m.map)
    m2 = Model(100, rng)
    m2.tally(cache, hashes_of(rng, 64))  # 64 new hashes into 6 free slots: dropped whole, sticky
    with pytest.raises(_lib.PzError) as e:
        cache.read()
    assert e.value.code == _lib.PZ_ERANGE
    keys = list(kept_map)
    cache.retain(keys[::2])
    with pytest.raises(_lib.PzError) as e:
        cache.read()
    assert e.value.code == _lib.PZ_ERANGE
    assert cache.reserve(40) == 40
    with pytest.raises(_lib.PzError) as e:
        cache.voters(keys[0])
    assert e.value.code == _lib.PZ_ERANGE
    assert cache.items(strict=False) == {k: kept_map[k][1] for k in keys[::2]}


def test_every_einval_edge():
    import torch

    rng, m, cache = small_cache()
    dll = _lib.lib.dll
    h = cache._h
    hashes = torch.zeros(32 * 4 + 16, dtype=torch.uint8, device="cuda:0")
    scratch = torch.zeros(int(dll.pz_vote_cache_retain_scratch_bytes(16, 4)) + 16, dtype=torch.uint8, device="cuda:0")
    hp, sp = hashes.data_ptr(), scratch.data_ptr()
    assert hp % 16 == 0 and sp % 16 == 0
    host = np.zeros((4, 32), np.uint8)
    cap = ctypes.c_uint32(0)
    assert dll.pz_vote_cache_capacity(None, ctypes.byref(cap)) == E and dll.pz_vote_cache_capacity(h, None) == E
    assert dll.pz_dev_vote_cache_reserve(None, 32, None) == E and dll.pz_vote_cache_reserve(None, 32) == E
    assert dll.pz_dev_vote_cache_reserve(h, (1 << 30) + 1, None) == E and dll.pz_vote_cache_reserve(h, (1 << 30) + 1) == E
    assert dll.pz_dev_vote_cache_retain(None, hp, 4, sp, None) == E and dll.pz_vote_cache_retain(None, host.ctypes.data, 4) == E
    assert dll.pz_dev_vote_cache_retain(h, None, 4, sp, None) == E and dll.pz_vote_cache_retain(h, None, 4) == E
    assert dll.pz_dev_vote_cache_retain(h, hp + 8, 4, sp, None) == E
    assert dll.pz_dev_vote_cache_retain(h, hp, 1 << 31, sp, None) == E and dll.pz_vote_cache_retain(h, host.ctypes.data, 1 << 31) == E
    assert dll.pz_dev_vote_cache_retain(h, hp, 4, None, None) == E
    assert dll.pz_dev_vote_cache_retain(h, hp, 4, sp + 4, None) == E
    assert dll.pz_dev_vote_cache_retain(h, None, 0, None, None) == E  # (no hash still needs its scratch)
    torch.cuda.synchronize()
    assert dll.pz_vote_cache_capacity(h, ctypes.byref(cap)) == 0 and cap.value == 16
    m.check(cache)  # nothing was launched: the cache is as it was


# ---- 3: ResidentChain over the 330-block chain ----------------------------------------------------------------------
@functools.lru_cache(None)
def chain330():
    """synth.chain_blocks(1024, 330, seed=4), its bytes, and the oracle stepped over it once (shared, never changed)."""
    blocks = synth.chain_blocks(1024, 330, seed=4)
    data, offs = bc.serialize_blocks(blocks)
    chain = oreplay.Chain(1024)
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks]
    assert [r["status"] for r in recs] == ["processed"] * 330
    return blocks, data, offs, chain, recs


def resident(slot_cap, **kw):
    from test_state_wire_gpu import genesis_resident

    state, tab = genesis_resident(oreplay.Chain(1024).C)
    return bc.ResidentChain(DeviceVoteCache(1024, slot_cap), DevicePendingAttestations(CAPS), DeviceRecentHashes(),
                            DeviceSavedBlocks(None), state, tab, **kw)


def watch(rc):
    """(entries, capacity) after every call of ``rc.process_serialized``."""
    seen, inner = [], rc.process_serialized

    def spy(*a, **k):
        out = inner(*a, **k)
        seen.append((len(rc.cache.read()[1]), rc.cache.slot_cap))
        return out

    rc.process_serialized = spy
    return seen


def test_the_default_policy_still_ends_in_the_capacity_error():
    blocks, data, offs, chain, recs = chain330()
    rc = resident(256)
    assert rc.cache_policy == "fixed"
    with pytest.raises(_lib.PzError) as e:
        rc.process_all(data, offs)
        rc.cache.read()
    assert e.value.code == _lib.PZ_ERANGE
    assert rc.cache.slot_cap == 256 and rc.cache_retains == 0 and rc.cache_grows == 0


def test_retire_runs_the_chain_in_256_slots():
    blocks, data, offs, chain, recs = chain330()
    assert len(chain.candidate[1].cache) > 256  # (CPU: the reference's map has outgrown the capacity)
    rc = resident(256, cache_policy="retire")
    seen = watch(rc)
    outs = rc.process_all(data, offs, want_digests=True)
    check_outs(outs, recs, blocks)
    assert rc.cache_retains >= 1 and all(n <= cap for n, cap in seen)
    # check_chain without its whole-map comparison: the entries a later stateRecalc can read
    _, A, C = chain.candidate
    state = rc.state
    ring = [bytes(h) for h in A.data.recent_block_hashes]
    got, oracle = snapshot(rc.cache), want(A.cache)
    assert {h: got[h] for h in set(ring) if h in got} == {h: oracle[h] for h in set(ring) if h in oracle}
    assert set(got) <= set(oracle) and all(got[h] == oracle[h] for h in got if h in ring)
    assert rc.pool.records() == [as_pb(a) for a in A.data.pending_attestations]
    assert rc.ring.hashes() == ring
    assert set(rc.saved.hashes()) == chain.saved and rc.saved.count() == len(chain.saved)
    assert tuple(getattr(state, k) for k in state._SCALARS) == tuple(getattr(C, k) for k in state._SCALARS)
    assert [(r.dynasty, r.slot, bytes(r.blockhash)) for r in state.crosslink_records] == \
        [(r.dynasty, r.slot, bytes(r.blockhash)) for r in C.crosslink_records]
    np.testing.assert_array_equal(state.balances(), np.array([v.balance for v in C.validators], U64))
    rest = (C.crosslinking_start_shard, bytes(C.dynasty_seed), C.dynasty_seed_last_reset)
    assert bc.resident_state_roots(rc.pool, state, rc.ring, wire.committees_device(table(C)), None, *rest) == \
        (ref.active_state_hash(A.data), ref.crystallized_state_hash(C))
    assert rc.has_candidate and rc.candidate_slot == chain.candidate[0].slot_number and rc.lag == int(C is not chain.C)


def test_grow_runs_the_chain_from_64_slots():
    blocks, data, offs, chain, recs = chain330()
    rc = resident(64, cache_policy="grow")
    seen = watch(rc)
    outs = rc.process_all(data, offs, want_digests=True)
    check_outs(outs, recs, blocks)
    check_chain(chain, rc)  # the whole map included
    assert rc.cache_grows >= 1 and rc.cache_retains == 0 and all(n <= cap for n, cap in seen)


def test_an_unknown_policy_is_refused():
    with pytest.raises(_lib.PzError) as e:
        resident(64, cache_policy="evict")
    assert e.value.code == E
