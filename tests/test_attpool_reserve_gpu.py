"""Growth of the device-resident pending-attestation pool (prysm_amd/csrc/attpool.hip:
pz_att_pool_capacity, pz_[dev_]att_pool_reserve, pz_[dev_]att_pool_need;
pending.DevicePendingAttestations.reserve / .capacity / .need_columns / .need_host;
blockchain.ResidentChain's pool_policy).

1. Pools built with append_host from small record lists, compared through records(), columns(),
   shard32(), active_state() and counts() before and after a reserve, in both forms.
2. Which capacity grows: each of the seven alone from a pool full in exactly that one, all seven at
   once, min_caps at and below the capacities, growth to exactly max(cap, min).
3. Order with the other calls, and stateRecalc over a grown pool against a twin created large.
4. The sticky word, the need sums against a real append on a twin, every PZ_EINVAL with a handle.
5. ResidentChain over synth.chain_blocks(1024, 330, seed=4) from a pool the oracle shows to be too small.
The model is a Python list of pb.AttestationRecord; every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ref
from oracle import replay as oreplay
from prysm_amd import _lib, pb, wire
from prysm_amd import blockchain as bc
from prysm_amd.pending import DevicePendingAttestations, DeviceRecentHashes, DeviceSavedBlocks
from prysm_amd.votes import DeviceVoteCache
from test_attpool_gpu import append, as_pb, check, kept, pool_for, put, rec, sizes, table
from test_blockcycle_gpu import check_chain, check_outs
from test_blockwalk_gpu import CAPS
from test_votecache_retain_gpu import chain330

pytestmark = pytest.mark.gpu

U64 = np.uint64
PROCESSED = 0
E = _lib.PZ_EINVAL
STATUSES = [0, 1, 2, 3, 4, 5, 6, 7, _lib.PZ_EINVAL]
RECENT = np.random.default_rng(99).integers(0, 256, size=(8, 32), dtype=np.uint8)


# ---- helpers ----------------------------------------------------------------------------------------------------
def ok(n):
    return np.zeros(n, np.int32)


def fill(pool, recs, form="host", comm=None):
    comm = np.arange(len(recs), dtype=np.uint32) if comm is None else comm
    append(pool, form, wire.attestation_columns(recs), len(recs), ok(len(recs)), comm)


def everything(pool, strict=True):
    """What the pool shows through every read: records, columns, shard32, the stored ActiveState, counts."""
    cols = pool.columns(strict)
    return (pool.records(strict), {k: v.tobytes() for k, v in cols.items()}, pool.shard32().tobytes(),
            pool.active_state(RECENT, strict=strict), pool.counts(strict).tolist())


def rich(rng, k):
    """Record k of a list with every shape: 3 oblique hashes and none, aggregate_sig of 0 and 2 values."""
    return rec(rng, jb=int(rng.integers(0, 40)), sb=int(rng.integers(0, 40)), bf=int(rng.integers(0, 9)),
               elems=(32, 0, 5) if k % 3 == 0 else (), nsig=2 if k % 2 == 0 else 0, shard=(1 << 40) if k % 7 == 3 else None)


def grow_by(pool, extra, device_form):
    want = pool.capacity() + np.asarray(extra, dtype=U64)
    pool.reserve(want, device_form=device_form)
    np.testing.assert_array_equal(pool.capacity(), want)
    np.testing.assert_array_equal(pool.caps, want)
    return want


# ---- 1: row shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_form", [True, False])
@pytest.mark.parametrize("rows", [0, 1, 4, 257, 513])
def test_a_reserve_changes_nothing_a_read_shows(rows, device_form):
    """Live rows 0, 1, 4 (the row capacity: full), 257 (past one tile) and 513, from pools full in every
    capacity; the grown pool then takes one more row."""
    rng = np.random.default_rng(rows)
    recs = [rich(rng, k) for k in range(rows)]
    pool = pool_for(recs)  # exactly full (an empty pool: one row of room, nothing else)
    fill(pool, recs)
    before = everything(pool)
    assert before[0] == recs
    grow_by(pool, [1, 40, 40, 9, 3, 37, 2], device_form)
    assert everything(pool) == before
    more = rich(rng, 0)
    fill(pool, [more], "device", comm=np.array([77], np.uint32))
    check(pool, recs + [more], list(range(rows)) + [77])


@pytest.mark.parametrize("device_form", [True, False])
@pytest.mark.parametrize("length", [1, 15, 17, 33])
def test_bytes_columns_of_odd_live_lengths(length, device_form):
    """Every bytes column's live length 1, 15, 17 and 33: under, across and past the 16-byte pieces, with a
    tail of 1, 3 x 4 + 3, 1 and 1 bytes; the rows' u32 columns end on a 4-byte tail."""
    rng = np.random.default_rng(length)
    recs = [rec(rng, jb=length, sb=length, bf=length, elems=(length,), nsig=length % 3)] + [rec(rng, jb=0, sb=0, bf=0) for _ in range(2)]
    pool = pool_for(recs)
    fill(pool, recs)
    np.testing.assert_array_equal(pool.counts()[[1, 2, 3, 5]], [length] * 4)
    before = everything(pool)
    grow_by(pool, [1, 1, 1, 1, 1, 1, 1], device_form)
    assert everything(pool) == before and before[0] == recs


# ---- 2: which capacity grows -------------------------------------------------------------------------------------------
def two_batches(rng):
    first = [rich(rng, k) for k in range(1 + int(rng.integers(0, 5)))]
    second = [rich(rng, k) for k in range(int(rng.integers(0, 4)))] + [rec(rng, jb=32, sb=32, bf=5, elems=(3, 0), nsig=2)]
    return first, second


@pytest.mark.parametrize("device_form", [True, False])
@pytest.mark.parametrize("c", range(7))
def test_each_capacity_alone(c, device_form):
    """A pool with room for the second batch everywhere but in capacity c, where it is one short: a twin
    refuses the batch (sticky PZ_ERANGE); after a reserve of that one capacity by one it lands."""
    rng = np.random.default_rng(10 + c)
    first, second = two_batches(rng)
    caps = sizes(first + second) + U64(7)
    caps[c] = sizes(first + second)[c] - U64(1)
    twin, pool = DevicePendingAttestations(caps), DevicePendingAttestations(caps)
    fill(twin, first), fill(twin, second)
    with pytest.raises(_lib.PzError) as e:
        twin.counts()
    assert e.value.code == _lib.PZ_ERANGE and twin.records(strict=False) == first
    fill(pool, first)
    min_caps = np.zeros(7, U64)
    min_caps[c] = caps[c] + U64(1)
    pool.reserve(min_caps, device_form=device_form)
    want = caps.copy()
    want[c] += U64(1)
    np.testing.assert_array_equal(pool.capacity(), want)  # exactly max(cap, min): nothing is rounded up
    fill(pool, second, "device" if device_form else "host", comm=np.arange(100, 100 + len(second), dtype=np.uint32))
    check(pool, first + second, list(range(len(first))) + list(range(100, 100 + len(second))))
    assert int(pool.counts()[c]) == int(want[c])  # full to the element in the grown capacity


@pytest.mark.parametrize("device_form", [True, False])
def test_all_seven_at_once(device_form):
    rng = np.random.default_rng(3)
    first, second = two_batches(rng)
    caps = sizes(first)
    twin, pool = DevicePendingAttestations(caps), DevicePendingAttestations(caps)
    fill(twin, first), fill(twin, second)
    with pytest.raises(_lib.PzError) as e:
        twin.counts()
    assert e.value.code == _lib.PZ_ERANGE
    fill(pool, first)
    pool.reserve(sizes(first + second), device_form=device_form)
    np.testing.assert_array_equal(pool.capacity(), sizes(first + second))
    fill(pool, second, "device")
    check(pool, first + second)
    np.testing.assert_array_equal(pool.counts(), pool.capacity())


@pytest.mark.parametrize("device_form", [True, False])
def test_min_caps_at_or_below_the_capacities_change_nothing(device_form):
    import torch

    rng = np.random.default_rng(4)
    recs = [rich(rng, k) for k in range(6)]
    pool = pool_for(recs, slack=40)
    fill(pool, recs)
    caps, n = pool.capacity().copy(), pool.counts()
    used = {"justified_block_hash": int(n[1]), "shard_block_hash": int(n[2]), "attester_bitfield": int(n[3]),
            "oblique_parent_hashes": int(n[5]), "aggregate_sig": 8 * int(n[6])}
    for k, t in pool.raw_columns().items():  # a canary behind the live bytes of the live set
        t[used[k]:].fill_(0xA5)
    addresses = [getattr(pool.view()[0], k) for k in wire.ATT_COLS] + list(pool.view()[1:])
    below = caps.copy()
    below[::2] -= U64(1)
    for min_caps in (caps, below, np.zeros(7, U64)):
        pool.reserve(min_caps, device_form=device_form)
        np.testing.assert_array_equal(pool.capacity(), caps)
    torch.cuda.synchronize()
    assert [getattr(pool.view()[0], k) for k in wire.ATT_COLS] + list(pool.view()[1:]) == addresses  # the same buffers
    for k, t in pool.raw_columns().items():
        assert (t[used[k]:].cpu().numpy() == 0xA5).all(), k
    check(pool, recs)


# ---- 3: order with the other calls ---------------------------------------------------------------------------------
def slots(recs, lsr):
    return [r for r in recs if r.slot > lsr]


@pytest.mark.parametrize("case", ["reserve-prune-append", "prune-reserve", "two reserves", "behind an append"])
def test_order_with_the_other_calls(case):
    """Device forms on one stream with no synchronize between them; every result equals the list model."""
    rng = np.random.default_rng(len(case))
    first = [rich(rng, k) for k in range(40)]
    second = [rich(rng, k) for k in range(300)]  # more than a tile, and more than the pool had room for
    pool = pool_for(first, slack=2)
    big = sizes(first + second) + U64(5)
    if case == "reserve-prune-append":
        fill(pool, first, "device")
        pool.reserve(big, device_form=True)
        pool.prune(100)  # into the set the reserve left behind: it grows first
        fill(pool, second, "device")
        model = slots(first, 100) + second
    elif case == "prune-reserve":
        fill(pool, first, "device")
        pool.prune(100)
        pool.reserve(big, device_form=True)
        fill(pool, second, "device")
        pool.prune(50)
        model = slots(slots(first, 100) + second, 50)
    elif case == "two reserves":
        fill(pool, first, "device")
        half = pool.capacity() + U64(3)
        pool.reserve(half, device_form=True)
        np.testing.assert_array_equal(pool.capacity(), half)
        pool.reserve(big, device_form=True)
        fill(pool, second, "device")
        model = first + second
    else:
        fill(pool, first, "device")
        pool.reserve(big, device_form=True)  # right behind the append's four launches
        fill(pool, second, "device")
        pool.reserve(big + U64(1), device_form=True)
        model = first + second
    check(pool, model)
    assert (pool.counts() <= pool.capacity()).all()


def test_state_recalc_over_a_grown_pool_equals_a_twin_created_large():
    """pz_dev_state_recalc sizes its scratch by the pool's row capacity: a pool grown from half the rows
    against a twin created with the final capacities -- winners, scalars, records, balances and the
    pruned pools."""
    from test_recalc_gpu import records_of, scalars_of, states_for, synthetic
    from test_votecache_gpu import rand_hashes

    inst, recs = synthetic(4096, False, (32, 0, 7))
    comm = inst["att_comm"][:len(recs)]
    half = len(recs) // 2
    twin = pool_for(recs, slack=64)
    fill(twin, recs, comm=comm)
    pool = pool_for(recs[:half])
    fill(pool, recs[:half], comm=comm[:half])
    pool.reserve(twin.capacity(), device_form=True)
    fill(pool, recs[half:], "device", comm=comm[half:])
    np.testing.assert_array_equal(pool.capacity(), twin.capacity())
    _, s_twin = states_for(inst, last_state_recalc=31)
    _, s_pool = states_for(inst, last_state_recalc=31)
    recent = rand_hashes(np.random.default_rng(3), 64)
    w_twin = bc.state_recalc_resident(twin, None, s_twin, recent, 1234)
    w_pool = bc.state_recalc_resident(pool, None, s_pool, recent, 1234)
    np.testing.assert_array_equal(w_pool, w_twin)
    assert (w_pool != 0xFFFFFFFF).any()
    assert scalars_of(s_pool) == scalars_of(s_twin) and records_of(s_pool) == records_of(s_twin)
    np.testing.assert_array_equal(s_pool.balances(), s_twin.balances())
    assert everything(pool) == everything(twin) and 0 < len(pool) < len(recs)


# ---- 4: the sticky word, need, the refusals ---------------------------------------------------------------------------
def inverted_columns(recs, rows):
    """The records' host columns with the bitfield ranges of ``rows`` inverted (each needs a longer row before it)."""
    cols = wire.attestation_columns(recs)
    offs = cols["attester_bitfield_offs"]
    for i in rows:
        offs[i], offs[i + 1] = offs[i + 1], offs[i]
        assert offs[i + 1] < offs[i]
    return cols


@pytest.mark.parametrize("device_form", [True, False])
@pytest.mark.parametrize("bits", ["capacity", "inverted", "both"])
def test_the_sticky_word_is_carried_over(bits, device_form):
    rng = np.random.default_rng(5)
    recs = [rec(rng, bf=3 + k) for k in range(4)]
    pool = pool_for(recs, slack=2)
    model = []
    if bits != "capacity":
        pool.append_host(inverted_columns(recs, [1]), 4, ok(4), np.arange(4, dtype=np.uint32), np.array([0, 1, 0, 0], np.uint8))
        model = [pb.AttestationRecord()]  # the row landed empty
    if bits != "inverted":
        fill(pool, recs + recs)  # more than the pool holds: dropped whole
    code = _lib.PZ_EINVAL if bits != "capacity" else _lib.PZ_ERANGE
    for _ in range(2):
        with pytest.raises(_lib.PzError) as e:
            pool.counts()
        assert e.value.code == code
        assert pool.records(strict=False) == model
        grow_by(pool, [8, 300, 300, 100, 8, 100, 8], device_form)
    fill(pool, recs + recs)  # now it lands, and the word stays
    with pytest.raises(_lib.PzError) as e:
        pool.counts()
    assert e.value.code == code and pool.records(strict=False) == model + recs + recs


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_need_is_what_an_append_adds(n):
    """need_columns and need_host against counts() after minus counts() before of the real append on a twin:
    take0 alone, take1 alone, both, neither, and rows with an inverted range among them; canaries behind the
    fourteen output words."""
    import torch

    rng = np.random.default_rng(n)
    recs = [rec(rng, bf=2 + int(rng.integers(0, 6)), elems=(3,) * int(rng.integers(0, 3)), nsig=int(rng.integers(0, 3))) for _ in range(n)]
    status = rng.choice(STATUSES, size=n, p=[0.6] + [0.05] * 8).astype(np.int32)
    takes = [(rng.random(n) < 0.5).astype(np.uint8), (rng.random(n) < 0.3).astype(np.uint8)]
    for inverted in ([], list(range(1, n - 1, 7))):
        cols = inverted_columns(recs, inverted) if n else {}
        base = [rec(rng), rec(rng, elems=(4,), nsig=1)]

        @functools.lru_cache(None)
        def added(which):  # the real append, on a twin with room for everything (an inversion lengthens its neighbours)
            twin = pool_for(base + recs, slack=8 + 8 * n)
            fill(twin, base)
            before = twin.counts()
            twin.append_host(cols, n, status, np.zeros(n, np.uint32), None if which is None else takes[which])
            return (twin.counts(strict=False) - before).tolist()

        for w0, w1 in ((0, None), (None, 1), (0, 1), (None, None)):
            t0, t1 = (None if w is None else takes[w] for w in (w0, w1))
            want = [added(w0), added(w1)]
            if t0 is None and t1 is None:
                assert want[0] == want[1]
            assert DevicePendingAttestations.need_host(cols, n, status, t0, t1).tolist() == want
            d = {k: put(v) for k, v in cols.items()}
            d_status = put(status)
            d0, d1 = (None if t is None else put(t) for t in (t0, t1))
            got = DevicePendingAttestations.need_columns(d, n, d_status, d0, d1)
            assert got.cpu().numpy().view(U64).tolist() == want
            # the ABI over a buffer of its own: nothing behind the fourteen words is written
            out = torch.full((14 + 16,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
            scratch = torch.empty(int(_lib.lib.dll.pz_att_pool_need_scratch_bytes(n)) + 16, dtype=torch.uint8, device="cuda:0")
            c = _lib.att_cols(d)
            _lib.lib.call("pz_dev_att_pool_need", ctypes.byref(c), n, _lib.dptr(d_status), _lib.dptr(d0), _lib.dptr(d1),
                          out.data_ptr(), scratch.data_ptr(), _lib.stream_ptr(0))
            host = out.cpu().numpy()
            assert host[:14].view(U64).reshape(2, 7).tolist() == want and (host[14:] == 0x5A5A5A5A5A5A5A5A).all()
        if n < 3:
            break


def test_argument_errors_are_einval_and_launch_nothing():
    import torch

    rng = np.random.default_rng(6)
    recs = [rich(rng, k) for k in range(5)]
    pool = pool_for(recs, slack=1)
    fill(pool, recs)
    before, caps = everything(pool), pool.capacity().copy()
    addresses = [getattr(pool.view()[0], k) for k in wire.ATT_COLS]
    dll, h = _lib.lib.dll, pool._h
    out = np.zeros(7, U64)
    assert dll.pz_att_pool_capacity(h, None) == E and dll.pz_att_pool_capacity(None, out.ctypes.data) == E
    assert dll.pz_dev_att_pool_reserve(h, None, None) == E and dll.pz_att_pool_reserve(h, None) == E
    assert dll.pz_dev_att_pool_reserve(None, out.ctypes.data, None) == E and dll.pz_att_pool_reserve(None, out.ctypes.data) == E
    for c in range(7):  # what pz_att_pool_new refuses as a capacity
        bad = caps.copy()
        bad[c] = U64(1) << U64(40)
        assert dll.pz_dev_att_pool_reserve(h, bad.ctypes.data, None) == E and dll.pz_att_pool_reserve(h, bad.ctypes.data) == E
        with pytest.raises(_lib.PzError) as e:
            DevicePendingAttestations(bad)
        assert e.value.code == E
    # need: the device form's pointers
    d = {k: put(v) for k, v in wire.attestation_columns(recs).items()}
    c, st = _lib.att_cols(d), put(ok(5))
    need = torch.full((14,), -1, dtype=torch.int64, device="cuda:0")
    scr = torch.zeros(int(dll.pz_att_pool_need_scratch_bytes(5)) + 16, dtype=torch.uint8, device="cuda:0")
    call = dll.pz_dev_att_pool_need
    good = dict(a=ctypes.byref(c), n=5, status=st.data_ptr(), t0=None, t1=None, need=need.data_ptr(), scr=scr.data_ptr(), sh=None)
    args = lambda **o: [o.get(k, v) for k, v in good.items()]  # noqa: E731
    lone = _lib.att_cols({"attester_bitfield_offs": d["attester_bitfield_offs"]})
    lone.attester_bitfield = None
    for bad in (dict(a=None), dict(status=None), dict(need=None), dict(need=need.data_ptr() + 4), dict(scr=None),
                dict(scr=scr.data_ptr() + 8), dict(a=ctypes.byref(lone)), dict(n=1 << 38)):
        assert call(*args(**bad)) == E, list(bad)
    torch.cuda.synchronize()
    assert (need.cpu().numpy() == -1).all()  # nothing was launched
    np.testing.assert_array_equal(pool.capacity(), caps)
    assert [getattr(pool.view()[0], k) for k in wire.ATT_COLS] == addresses and everything(pool) == before


# ---- 5: ResidentChain over the 330-block chain ------------------------------------------------------------------------
SMALL = [8, 256, 256, 16, 8, 256, 16]  # an eighth of what the chain's busiest list holds (below)
SLOTS = 2048  # a vote cache that holds the whole chain: only the pool is short


def resident(caps, slot_cap=SLOTS, **kw):
    from test_state_wire_gpu import genesis_resident

    state, tab = genesis_resident(oreplay.Chain(1024).C)
    return bc.ResidentChain(DeviceVoteCache(1024, slot_cap), DevicePendingAttestations(caps), DeviceRecentHashes(),
                            DeviceSavedBlocks(None), state, tab, **kw)


@functools.lru_cache(None)
def pending_peaks():
    """The seven sizes of the oracle's PendingAttestations at their largest over the 330 blocks (CPU only)."""
    blocks = chain330()[0]
    chain = oreplay.Chain(1024)
    peak = np.zeros(7, U64)
    for b in blocks:
        chain.process_block(oreplay.to_pb_block(b))
        peak = np.maximum(peak, sizes([as_pb(a) for a in chain.candidate[1].data.pending_attestations]))
    return peak


@functools.lru_cache(None)
def ample_twin():
    """(calls, resubmits) of the chain under the default policy with a pool that holds everything."""
    _, data, offs, _, _ = chain330()
    rc = resident(CAPS)
    rc.process_all(data, offs)
    assert rc.pool_policy == "fixed" and rc.pool_grows == 0
    return rc.calls, rc.resubmits


def watch(rc):
    seen, inner = [], rc.process_serialized

    def spy(*a, **k):
        out = inner(*a, **k)
        seen.append((rc.pool.counts(), rc.pool.capacity()))
        return out

    rc.process_serialized = spy
    return seen


def test_the_oracle_alone_shows_the_small_pool_is_too_small():
    peak = pending_peaks()
    assert (peak > np.array(SMALL, U64)).all(), peak  # rows, bitfield bytes and every other column
    assert int(peak[0]) > SMALL[0] and int(peak[3]) > SMALL[3]
    assert (peak <= np.array(CAPS, U64)).all()  # and the twin's pool is ample


def test_the_default_policy_ends_in_the_capacity_error():
    """The default queues nothing and reads nothing more than it did, so -- as with the vote cache's
    default (test_votecache_retain_gpu) -- the dropped appends show where the pool is next read: the sticky
    PZ_ERANGE, with a list shorter than the oracle's.  (On the MI355X process_all itself returns: nothing in
    the default path reads the pool's word, so the object is not marked spent by it.)"""
    _, data, offs, _, _ = chain330()
    rc = resident(SMALL)
    assert rc.pool_policy == "fixed"
    with pytest.raises(_lib.PzError) as e:
        rc.process_all(data, offs)
        rc.pool.counts()
    assert e.value.code == _lib.PZ_ERANGE
    assert rc.pool_grows == 0
    np.testing.assert_array_equal(rc.pool.capacity(), SMALL)
    assert (rc.pool.counts(strict=False) <= np.array(SMALL, U64)).all()


def test_grow_runs_the_chain_from_the_small_pool():
    blocks, data, offs, chain, recs = chain330()
    rc = resident(SMALL, pool_policy="grow")
    seen = watch(rc)
    outs = rc.process_all(data, offs, want_digests=True)
    check_outs(outs, recs, blocks)
    check_chain(chain, rc)  # cache with voters, pool, ring, saved set, scalars, records, balances, both roots
    assert rc.pool_grows >= 1
    assert (rc.calls, rc.resubmits) == ample_twin()
    assert all((n <= cap).all() for n, cap in seen)
    assert (rc.pool.capacity() >= pending_peaks()).all()


def test_grow_together_with_a_retiring_cache():
    from test_votecache_gpu import snapshot, want

    blocks, data, offs, chain, recs = chain330()
    rc = resident(SMALL, slot_cap=256, pool_policy="grow", cache_policy="retire")
    seen = watch(rc)
    outs = rc.process_all(data, offs, want_digests=True)
    check_outs(outs, recs, blocks)
    assert rc.pool_grows >= 1 and rc.cache_retains >= 1 and all((n <= cap).all() for n, cap in seen)
    _, A, C = chain.candidate
    state = rc.state
    ring = [bytes(h) for h in A.data.recent_block_hashes]
    got, oracle = snapshot(rc.cache), want(A.cache)
    assert {h: got[h] for h in set(ring) if h in got} == {h: oracle[h] for h in set(ring) if h in oracle}
    assert rc.pool.records() == [as_pb(a) for a in A.data.pending_attestations]
    assert rc.ring.hashes() == ring
    assert set(rc.saved.hashes()) == chain.saved
    assert tuple(getattr(state, k) for k in state._SCALARS) == tuple(getattr(C, k) for k in state._SCALARS)
    np.testing.assert_array_equal(state.balances(), np.array([v.balance for v in C.validators], U64))
    rest = (C.crosslinking_start_shard, bytes(C.dynasty_seed), C.dynasty_seed_last_reset)
    assert bc.resident_state_roots(rc.pool, state, rc.ring, wire.committees_device(table(C)), None, *rest) == \
        (ref.active_state_hash(A.data), ref.crystallized_state_hash(C))


def test_from_state_grows_through_the_first_two_cycles():
    blocks = chain330()[0][:130]
    chain = oreplay.Chain(1024)
    raw = ref.marshal(chain.C)  # the stored bytes of the genesis CrystallizedState
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks]
    assert sum(r["transition"] for r in recs) == 2
    rc = bc.ResidentChain.from_state(raw, caps=SMALL, pool_policy="grow")
    assert rc.pool_policy == "grow" and rc.cache_policy == "fixed"
    np.testing.assert_array_equal(rc.pool.capacity(), SMALL)
    data, offs = bc.serialize_blocks(blocks)
    outs = rc.process_all(data, offs, want_digests=True)
    check_outs(outs, recs, blocks)
    check_chain(chain, rc)
    assert rc.pool_grows >= 1


def test_an_unknown_policy_is_refused():
    with pytest.raises(_lib.PzError) as e:
        resident(SMALL, pool_policy="shrink")
    assert e.value.code == E
    with pytest.raises(_lib.PzError) as e:
        bc.ResidentChain.from_state(b"", pool_policy="evict")
    assert e.value.code == E
