"""stateRecalc as one ABI call over the resident pool and vote cache (pz_dev_state_recalc,
prysm_amd/csrc/recalc.hip) and the vote cache's device lookup (pz_dev_vote_cache_lookup): the
lookup against pz_vote_cache_read as a dict; the justification loop through the whole call against
ref.state_recalc; the whole transition on twin states, pools and caches against
blockchain.state_recalc_device and the oracle; the refusals and the reference's panics."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ref
from oracle import replay as oreplay
from prysm_amd import _lib, casper, pb, synth, wire
from prysm_amd import blockchain as bc
from prysm_amd.pending import DevicePendingAttestations, RecalcState, ResidentRecalcState
from prysm_amd.votes import DeviceVoteCache
from test_attpool_gpu import as_pb, late_chain, pool_for, table
from test_votecache_gpu import State, att, put, rand_hashes

pytestmark = pytest.mark.gpu

U64 = np.uint64
M64 = (1 << 64) - 1
NONE32 = 0xFFFFFFFF
PROCESSED = 0
SCALARS = ("last_state_recalc", "justified_streak", "last_justified_slot", "last_finalized_slot", "current_dynasty",
           "total_deposits")


class NoDownload(DeviceVoteCache):
    """A vote cache whose map cannot be downloaded as a dict: the resident call must not need it."""

    def items(self, strict=True):
        raise AssertionError("the resident transition downloaded the vote cache")


def scalars_of(state):
    if isinstance(state, ResidentRecalcState):
        return tuple(int(x) for x in state.read(strict=False)["scalars"][:6])
    return tuple(getattr(state, k) for k in SCALARS)


def records_of(state):
    return [(r.dynasty, r.slot, bytes(r.blockhash)) for r in state.crosslink_records]


# ---- 1: the lookup ---------------------------------------------------------------------------------------
def occupied_cells(keys, cells):
    """The cells linear probing fills for these keys: the set does not depend on the insertion order."""
    occ = set()
    for k in keys:
        c = int.from_bytes(k[:4], "little") & (cells - 1)
        while c in occ:
            c = (c + 1) & (cells - 1)
        occ.add(c)
    return occ


@functools.lru_cache(None)
def filled(slot_cap):
    """A cache filled through the host tally, its keys and, per query kind, a pool of hashes."""
    rng = np.random.default_rng(100 + slot_cap)
    if slot_cap == 4:  # 8 cells; three keys whose home cell is the last one: cells 7, 0, 1
        keys = [b"\xff" * 4 + rng.bytes(28) for _ in range(3)]
        recent = [keys[int(i)] for i in np.concatenate([np.arange(3), rng.integers(0, 3, 125)])]
    else:
        recent = rand_hashes(rng, 128)
    st = State(1024, recent, balances=rng.integers(1, 1000, size=1024))
    atts, bslots = [att(st, 0, rng, j=0), att(st, 1, rng, j=1)], [3, 64]
    status, comm, pstart = st.check(atts, bslots)
    assert (status == PROCESSED).all()
    cache = DeviceVoteCache(st.nval, slot_cap)
    cache.tally_host(wire.attestation_columns(atts), len(atts), status, comm, pstart, st.recent, st.members, st.coffs, st.balance)
    hashes, totals = cache.read()
    present = [h.tobytes() for h in hashes]
    assert (len(present) == 3 if slot_cap == 4 else len(present) > 64) and (totals > 0).all()
    cells = 2
    while cells < 2 * slot_cap:
        cells *= 2
    occ = occupied_cells(present, cells)
    free = [c for c in range(cells) if c not in occ]
    assert free and len(occ) == len(present)
    absent_occupied = [p[:4] + rng.bytes(28) for p in present]                                # home cell holds a key
    absent_empty = [int(free[k % len(free)] + cells * (k + 1)).to_bytes(4, "little") + rng.bytes(28) for k in range(16)]
    model = {h: (int(t), s) for s, (h, t) in enumerate(zip(present, totals))}
    return cache, model, present, absent_occupied, absent_empty


def queries(slot_cap, n):
    _, _, present, occupied, empty = filled(slot_cap)
    kinds = [present, occupied, empty, present[:1]]  # (the last kind: the same key again and again)
    return [kinds[q % 4][(q // 4) % len(kinds[q % 4])] for q in range(n)]


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("slot_cap", [4, 512])
def test_lookup_against_the_read_as_a_dict(slot_cap, n, form):
    import torch

    cache, model, _, _, _ = filled(slot_cap)
    qs = queries(slot_cap, n)
    if form == "host":
        totals, slots = cache.lookup(qs)
    else:
        d = put(np.frombuffer(b"".join(qs), np.uint8).reshape(-1, 32)) if n else torch.zeros((0, 32), dtype=torch.uint8, device="cuda:0")
        t, s = cache.lookup_device(d)
        totals, slots = t.cpu().numpy().view(U64), s.cpu().numpy().view(np.uint32)
        t2, s2 = cache.lookup_device(d, want_slots=False)  # d_slots is optional
        assert s2 is None and np.array_equal(t2.cpu().numpy().view(U64), totals)
    assert len(totals) == n and len(slots) == n
    want = [model.get(h, (0, NONE32)) for h in qs]
    assert totals.tolist() == [w[0] for w in want] and slots.tolist() == [w[1] for w in want]
    if n >= 63:
        assert {w[1] == NONE32 for w in want} == {True, False}


def test_lookup_argument_errors_are_einval():
    import torch

    cache, _, present, _, _ = filled(4)
    dll = _lib.lib.dll
    q = put(np.frombuffer(present[0] + present[1], np.uint8).reshape(-1, 32))
    out = torch.full((4,), -7, dtype=torch.int64, device="cuda:0")
    sh = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert q.data_ptr() % 16 == 0
    assert dll.pz_dev_vote_cache_lookup(None, q.data_ptr(), 2, out.data_ptr(), None, sh) == _lib.PZ_EINVAL
    assert dll.pz_dev_vote_cache_lookup(cache._h, None, 2, out.data_ptr(), None, sh) == _lib.PZ_EINVAL
    assert dll.pz_dev_vote_cache_lookup(cache._h, q.data_ptr(), 2, None, None, sh) == _lib.PZ_EINVAL
    raw = put(np.zeros(80, np.uint8))
    assert dll.pz_dev_vote_cache_lookup(cache._h, raw.data_ptr() + 8, 2, out.data_ptr(), None, sh) == _lib.PZ_EINVAL
    assert dll.pz_dev_vote_cache_lookup(cache._h, None, 0, None, None, sh) == _lib.PZ_OK  # n == 0: nothing to do
    host = np.frombuffer(present[0], np.uint8)
    tot = np.zeros(1, U64)
    assert dll.pz_vote_cache_lookup(None, host.ctypes.data, 1, tot.ctypes.data, None) == _lib.PZ_EINVAL
    assert dll.pz_vote_cache_lookup(cache._h, None, 1, tot.ctypes.data, None) == _lib.PZ_EINVAL
    assert dll.pz_vote_cache_lookup(cache._h, host.ctypes.data, 1, None, None) == _lib.PZ_EINVAL
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()  # no refused call launched anything


def test_lookup_after_a_call_rolled_back_for_capacity():
    """test_a_call_that_does_not_fit_changes_nothing's three calls: the second is dropped whole, and
    the table it probed answers as the twin's that never saw it."""
    rng = np.random.default_rng(7)
    st = State(1024, rand_hashes(rng, 128), balances=rng.integers(1, 1000, size=1024))
    calls = []
    for atts, bslots in (([att(st, 0, rng, j=0), att(st, 0, rng, j=1)], [0, 0]),
                         ([att(st, 0, rng, j=0), att(st, 1, rng, j=1)], [63, 65]), ([att(st, 0, rng, j=1)], [1])):
        status, comm, pstart = st.check(atts, bslots)
        assert (status == PROCESSED).all()
        calls.append((wire.attestation_columns(atts), len(atts), status, comm, pstart, st.recent, st.members, st.coffs, st.balance))
    full, twin = DeviceVoteCache(st.nval, 127), DeviceVoteCache(st.nval, 127)
    full.tally_host(*calls[0])
    twin.tally_host(*calls[0])
    full.tally_host(*calls[1])  # one slot more than remains
    with pytest.raises(_lib.PzError) as e:
        full.read()
    assert e.value.code == _lib.PZ_ERANGE
    for step in (0, 1):
        got, want = full.lookup(st.recent), twin.lookup(st.recent)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        assert (got[1][:64 + step] != NONE32).all() and (got[1][64 + step:] == NONE32).all()
        full.tally_host(*calls[2])
        twin.tally_host(*calls[2])


# ---- 2: the justification loop through the whole call -----------------------------------------------
def mask_state(mask, seed=0, balances=None):
    """128 recent hashes whose first 64 realise ``mask``: position i holds its own hash when bit i is
    set and the hash F when it is clear; the two attestations tallied below name F as a raw 32-byte
    oblique element, so every parent equal to F is skipped (core.go:318-320) and F gets no entry."""
    rng = np.random.default_rng(1000 + seed)
    f = rng.bytes(32)
    recent = [rng.bytes(32) if i >= 64 or (mask >> i) & 1 else f for i in range(128)]
    return State(1024, recent, balances=balances), f, rng


def tally_mask(st, f, rng, cache, p=0.5):
    """Tallies committee 0 into recent[0 .. 63) and committee 1 into recent[1 .. 64), F skipped; the
    same in the oracle's map.  Returns that map."""
    cache_o = {}
    for ps, j in ((0, 0), (1, 1)):
        a = att(st, 0, rng, [f], j=j, p=p)
        status, comm, _ = st.check([a], [0])
        assert status[0] == PROCESSED
        cache.tally_host(wire.attestation_columns([a]), 1, status, comm, np.array([ps], U64), st.recent, st.members, st.coffs,
                         st.balance)
        members = st.committee(0, j)[1]
        voters = [v for k, v in enumerate(members) if ref.check_bit(a.attester_bitfield, k)]
        for h in [st.recent[q].tobytes() for q in range(ps, ps + 63)]:
            if h == f:
                continue
            entry = cache_o.setdefault(h, [{}, 0])
            for v in voters:
                if v not in entry[0]:
                    entry[0][v] = None
                    entry[1] = (entry[1] + int(st.balance[v])) & M64
    return cache_o


def resident_for(st, **scalars):
    cs = st.cs
    scalars.setdefault("current_dynasty", cs.current_dynasty)
    return ResidentRecalcState(st.balance, [v.start_dynasty for v in cs.validators], [v.end_dynasty for v in cs.validators],
                               st.members, st.coffs, cs.crosslink_records, **scalars)


def oracle_three(st, cache_o, lsr, streak, justified, finalized, deposits, block_slot):
    cs = st.cs
    cs.last_state_recalc, cs.justified_streak, cs.last_justified_slot = lsr, streak, justified
    cs.last_finalized_slot, cs.total_deposits = finalized, deposits
    del st.active.pending_attestations[:]
    nc, _ = ref.state_recalc(cs, st.active, cache_o, block_slot)
    return nc.justified_streak, nc.last_justified_slot, nc.last_finalized_slot, nc.last_state_recalc, nc.total_deposits


SINGLE = [M64 ^ (1 << i) for i in (0, 1, 31, 62, 63)]
MASKS = [M64, 0, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA] + SINGLE + [0x0123456789ABCDEF, 0xFFFFFFFF00000001]
STARTS = [(0, 0), (64, 1), (128, 64), (M64 - 63, M64), (128, 1), (0, 64)]  # (lastStateRecalc, streak)


@pytest.mark.parametrize("k", range(len(MASKS)))
def test_justification_through_the_call(k):
    """An empty pool, so the epoch applies nothing and only the loop moves the state.  TotalDeposits
    is 1 or 2^63 + 1 (2 * TotalDeposits == 2 mod 2^64): a slot passes iff its hash has an entry."""
    mask = MASKS[k]
    lsr, streak = STARTS[k % len(STARTS)]
    deposits = 1 if k % 2 else (1 << 63) + 1
    st, f, rng = mask_state(mask, seed=k)
    cache = NoDownload(st.nval, 256)
    cache_o = tally_mask(st, f, rng, cache)
    got_mask = sum(1 << i for i in range(64) if cache_o.get(st.recent[i].tobytes(), [0, 0])[1] > 0)
    assert got_mask == mask and f not in cache_o
    justified, finalized = lsr // 2, lsr // 4
    state = resident_for(st, last_state_recalc=lsr, justified_streak=streak, last_justified_slot=justified,
                         last_finalized_slot=finalized, current_dynasty=1, total_deposits=deposits)
    pool = DevicePendingAttestations([4, 64, 64, 64, 4, 64, 4])
    win = bc.state_recalc_resident(pool, cache, state, st.recent, 77)
    assert (win == NONE32).all() and len(win) == len(st.cs.crosslink_records)
    want = oracle_three(st, cache_o, lsr, streak, justified, finalized, deposits, 77)
    assert (state.justified_streak, state.last_justified_slot, state.last_finalized_slot, state.last_state_recalc,
            state.total_deposits) == want
    assert state.current_dynasty == 0 and len(pool) == 0
    np.testing.assert_array_equal(state.balances(), st.balance)


def test_justification_with_totals_whose_triple_wraps():
    """Balances near 2^63, so the slots' totals and their triples wrap: the mask is whatever the
    arithmetic gives, and the device's equals the oracle's."""
    rng = np.random.default_rng(5)
    bal = rng.integers(1 << 62, (1 << 64) - 1, size=1024, dtype=U64)
    st, f, rng2 = mask_state(0xF0F0F0F0FFFF0000, seed=99, balances=bal)
    cache = DeviceVoteCache(st.nval, 256)
    cache_o = tally_mask(st, f, rng2, cache)
    deposits = (1 << 63) + (1 << 61)
    state = resident_for(st, last_state_recalc=128, justified_streak=3, last_justified_slot=70, last_finalized_slot=2,
                         total_deposits=deposits)
    model = RecalcState(st.balance, [v.start_dynasty for v in st.cs.validators], [v.end_dynasty for v in st.cs.validators],
                        st.members, st.coffs, st.cs.crosslink_records, last_state_recalc=128, justified_streak=3,
                        last_justified_slot=70, last_finalized_slot=2, total_deposits=deposits)
    pool, pool_m = (DevicePendingAttestations([4, 64, 64, 64, 4, 64, 4]) for _ in range(2))
    bc.state_recalc_resident(pool, cache, state, st.recent, 200)
    bc.state_recalc_device(pool_m, cache, model, st.recent, 200)
    assert scalars_of(state) == scalars_of(model)
    want = oracle_three(st, cache_o, 128, 3, 70, 2, deposits, 200)
    assert (state.justified_streak, state.last_justified_slot, state.last_finalized_slot, state.last_state_recalc,
            state.total_deposits) == want
    passes = [(3 * cache_o.get(st.recent[i].tobytes(), [0, 0])[1]) & M64 >= (2 * deposits) & M64 for i in range(64)]
    assert True in passes and False in passes


def test_an_empty_pool_and_no_cache():
    rng = np.random.default_rng(2)
    st = State(1024, rand_hashes(rng, 64))
    deposits = int(st.balance.sum())
    state = resident_for(st, last_state_recalc=64, justified_streak=9, last_justified_slot=5, last_finalized_slot=1,
                         total_deposits=deposits)
    pool = DevicePendingAttestations([4, 64, 64, 64, 4, 64, 4])
    before = records_of(state)
    win = bc.state_recalc_resident(pool, None, state, st.recent, 130)
    assert (win == NONE32).all()
    assert scalars_of(state) == (128, 0, 5, 1, 0, deposits) and records_of(state) == before
    assert oracle_three(st, {}, 64, 9, 5, 1, deposits, 130) == (0, 5, 1, 128, deposits)
    np.testing.assert_array_equal(state.balances(), st.balance)


# ---- 3: the whole transition ------------------------------------------------------------------------------
def test_the_chain_through_the_resident_call():
    """test_the_chain_through_the_pool's 130 blocks at 1,024 validators on twin pools, caches and
    states: state_recalc_resident beside state_recalc_device at the two transition blocks, both beside
    oracle.replay.Chain.  The block of slot 64 sets a crosslink record and drops all 63 pending rows;
    the block of slot 128 prunes, keeping 32 rows and dropping 32."""
    nval, nblocks = 1024, 130
    blocks = late_chain(nval, nblocks, seed=4)
    data, offs = bc.serialize_blocks(blocks)
    chain = oreplay.Chain(nval)
    cs0 = chain.C
    tab0 = table(cs0)
    args = ([v.balance for v in cs0.validators], [v.start_dynasty for v in cs0.validators],
            [v.end_dynasty for v in cs0.validators], [v for arr in tab0 for e in arr for v in e[1]],
            bc._committee_table(tab0)[3], cs0.crosslink_records)
    kw = dict(last_state_recalc=cs0.last_state_recalc, justified_streak=cs0.justified_streak,
              last_justified_slot=cs0.last_justified_slot, last_finalized_slot=cs0.last_finalized_slot,
              current_dynasty=cs0.current_dynasty, total_deposits=cs0.total_deposits)
    model, state = RecalcState(*args, **kw), ResidentRecalcState(*args, **kw)
    caps = [256, 256 * 32, 256 * 32, 256 * 8, 256, 256 * 32, 512]
    twins = [(DevicePendingAttestations(caps), DeviceVoteCache(nval, 512)), (DevicePendingAttestations(caps), NoDownload(nval, 512))]
    tables = {}
    seen = {"crosslink": 0, "kept": [], "dropped": [], "transitions": 0}
    lsr = cs0.last_state_recalc
    for i, blk in enumerate(blocks):
        C, A = chain.C, chain.A.data
        if C.last_state_recalc not in tables:
            tables[C.last_state_recalc] = table(C)
        transition = blk.slot_number >= lsr + 64
        if transition:
            recent = [bytes(h) for h in chain.candidate[1].data.recent_block_hashes]
            before = len(twins[1][0])
            xl = records_of(state)
            w0 = bc.state_recalc_device(twins[0][0], twins[0][1], model, recent, blk.slot_number)
            w1 = bc.state_recalc_resident(twins[1][0], twins[1][1], state, recent, blk.slot_number)
            np.testing.assert_array_equal(w1, w0)
            after = len(twins[1][0])
            lsr += 64
            seen["transitions"] += 1
            seen["crosslink"] += xl != records_of(state)
            seen["kept"].append(after)
            seen["dropped"].append(before - after)
        lo, hi = int(offs[i]), int(offs[i + 1])
        for pool, cache in twins:
            report, _, status = bc.tally_serialized_blocks(
                cache, data[lo:hi], np.array([0, hi - lo], dtype=U64), C.last_justified_slot, C.last_state_recalc,
                len(A.recent_block_hashes), tables[C.last_state_recalc], [bytes(h) for h in A.recent_block_hashes],
                np.array([v.balance for v in C.validators], U64), pending=pool, candidate=[1])
            assert list(report) == [bc.BLOCK_TALLIED] and (status == PROCESSED).all(), i
        r = chain.process_block(oreplay.to_pb_block(blk))
        assert r["status"] == "processed" and r["transition"] == transition, i
        if transition:
            _, A1, C1 = chain.candidate
            np.testing.assert_array_equal(state.balances(), np.array([v.balance for v in C1.validators], U64))
            np.testing.assert_array_equal(state.balances(), model.balances())
            assert records_of(state) == records_of(model) == [(r.dynasty, r.slot, bytes(r.blockhash)) for r in C1.crosslink_records]
            assert scalars_of(state) == scalars_of(model) == tuple(getattr(C1, k) for k in SCALARS), i
            assert twins[1][0].records() == twins[0][0].records() == [as_pb(a) for a in A1.data.pending_attestations], i
            np.testing.assert_array_equal(twins[1][1].read()[1], twins[0][1].read()[1])
    assert seen == {"crosslink": 1, "kept": [0, 32], "dropped": [63, 32], "transitions": 2}


def synthetic(n, inactive, sbh_lens, seed=5):
    """test_epoch_from_the_pool's instance, every attestation with a ShardBlockHash of one of sbh_lens."""
    shuffled = casper.shuffle_indices(ref.bytes_to_hash(b"A"), np.arange(n, dtype=np.uint32))
    inst = synth.epoch_batch(n, 1, seed=seed, shuffled=shuffled)
    rng = np.random.default_rng(seed + 1)
    if inactive:
        inst["start"][:, rng.random(n) < 0.1] = 7
        inst["end"][:, rng.random(n) < 0.1] = 1
    natt = int(inst["natt"])
    bo = inst["boffs"].astype(np.int64)
    recs = [pb.AttestationRecord(slot=int(inst["att_slot"][a]), shard_id=int(inst["att_shard"][a]),
                                 shard_block_hash=rng.bytes(sbh_lens[a % len(sbh_lens)]),
                                 attester_bitfield=inst["bits"][bo[a]:bo[a + 1]].tobytes()) for a in range(natt)]
    return inst, recs


def states_for(inst, nrec=1024, hash_stride=32, **over):
    records = [pb.CrosslinkRecord(int(inst["rec_dynasty"][0][s]), bytes([s & 255]) * (s % 33), 3 * s) for s in range(nrec)]
    args = (inst["balance"][0], inst["start"][0], inst["end"][0], inst["committee"], inst["coffs"], records)
    kw = dict(last_state_recalc=64, justified_streak=2, last_justified_slot=40, last_finalized_slot=7,
              current_dynasty=int(inst["dynasty"][0]), total_deposits=int(inst["total_deposit"][0]))
    kw.update(over)
    return RecalcState(*args, **kw), ResidentRecalcState(*args, hash_stride=hash_stride, **kw)


def pools_for(inst, recs, extra=()):
    pools = []
    for _ in range(2):
        pool = pool_for(list(recs) + [r for r, _ in extra], slack=64)
        for r, comm in extra:  # (first: CalculateRewards reads the LAST attestation's bitfield)
            pool.append_host(wire.attestation_columns([r]), 1, np.zeros(1, np.int32), np.array([comm], np.uint32))
        pool.append_host(wire.attestation_columns(recs), len(recs), np.zeros(len(recs), np.int32), inst["att_comm"][:len(recs)])
        pools.append(pool)
    return pools


@pytest.mark.parametrize("n,inactive,stride,lens", [(4096, False, 32, (32, 0, 7)), (5000, True, 48, (32, 48, 33, 1))])
def test_the_rewards_apply(n, inactive, stride, lens):
    """test_epoch_from_the_pool's shapes: the threshold holds, the rewards apply, records are set
    from ShardBlockHashes of several lengths; the attestations' slots straddle lastStateRecalc."""
    from epoch_ref_helpers import oracle_epoch

    inst, recs = synthetic(n, inactive, lens)
    model, state = states_for(inst, hash_stride=stride, last_state_recalc=31)
    pool_m, pool = pools_for(inst, recs)
    rng = np.random.default_rng(3)
    recent = rand_hashes(rng, 64)
    w0 = bc.state_recalc_device(pool_m, None, model, recent, 1234)
    w1 = bc.state_recalc_resident(pool, None, state, recent, 1234)
    nb, applied, nxt, _, _, w = oracle_epoch(inst, 0)
    assert applied and (w != NONE32).any()
    np.testing.assert_array_equal(w1, w0)
    np.testing.assert_array_equal(w1, w)
    np.testing.assert_array_equal(state.balances(), model.balances())
    np.testing.assert_array_equal(state.balances(), nb)
    assert scalars_of(state) == scalars_of(model) and state.total_deposits == nxt and state.last_state_recalc == 95
    got = records_of(state)
    assert got == records_of(model)
    won = [s for s in range(1024) if w[s] != NONE32]
    assert all(got[s] == (int(inst["dynasty"][0]), 1234, bytes(recs[int(w[s])].shard_block_hash)) for s in won)
    assert len({len(got[s][2]) for s in won}) > 1  # hashes of several lengths were copied
    assert pool.records() == pool_m.records() == [r for r in recs if r.slot > 31]
    assert 0 < len(pool) < len(recs)
    raw = state.read()
    assert all(not raw["rec_hash"][s, int(raw["rec_hash_len"][s]):].any() for s in range(1024))  # zeros behind each hash


def test_no_crosslink_records():
    inst, recs = synthetic(4096, False, (32,))
    inst["bits"][:] = 0  # nobody attests: no attestation qualifies, so no record is indexed
    recs = [pb.AttestationRecord(slot=r.slot, shard_id=r.shard_id, shard_block_hash=r.shard_block_hash,
                                 attester_bitfield=bytes(len(r.attester_bitfield))) for r in recs]
    model, state = states_for(inst, nrec=0)
    pool_m, pool = pools_for(inst, recs)
    recent = rand_hashes(np.random.default_rng(4), 64)
    w0 = bc.state_recalc_device(pool_m, None, model, recent, 99)
    w1 = bc.state_recalc_resident(pool, None, state, recent, 99)
    assert len(w0) == 0 and len(w1) == 0 and state.crosslink_records == []
    assert scalars_of(state) == scalars_of(model)
    np.testing.assert_array_equal(state.balances(), inst["balance"][0])
    assert pool.records() == pool_m.records()


# ---- 4: refusals and panics ----------------------------------------------------------------------------
def snapshot(state, pool):
    r = state.read(strict=False)
    return ({k: v.copy() for k, v in r.items()}, state.balances().copy(), pool.counts(strict=False).copy(), pool.records(strict=False))


def same(a, b):
    return all(np.array_equal(a[0][k], b[0][k]) for k in a[0]) and np.array_equal(a[1], b[1]) and \
        np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_a_hash_longer_than_the_stride_is_refused_whole():
    """A ShardBlockHash of stride + 1 bytes on a row that could not win (nobody attests in it)."""
    inst, recs = synthetic(4096, False, (32,))
    shard = int(inst["att_shard"][0])
    nbytes = len(recs[0].attester_bitfield)
    long_row = pb.AttestationRecord(slot=70, shard_id=shard, shard_block_hash=b"\x07" * 33, attester_bitfield=bytes(nbytes))
    _, state = states_for(inst)
    _, twin = states_for(inst)
    pool, pool_t = pools_for(inst, recs, extra=[(long_row, int(inst["att_comm"][0]))])
    recent = rand_hashes(np.random.default_rng(4), 64)
    before = snapshot(state, pool)
    with pytest.raises(_lib.PzError) as e:
        bc.state_recalc_resident(pool, None, state, recent, 99)
    assert e.value.code == _lib.PZ_ERANGE
    assert same(snapshot(state, pool), before) and same(before, snapshot(twin, pool_t))
    state.read()  # nothing sticky: the call never began
    # the same pool under a stride that holds the row: the call lands
    _, wide = states_for(inst, hash_stride=48)
    bc.state_recalc_resident(pool, None, wide, recent, 99)
    assert wide.last_state_recalc == 128


def test_too_few_recent_hashes_is_the_panic_of_the_loop():
    inst, recs = synthetic(4096, False, (32,))
    model, state = states_for(inst)
    pool_m, pool = pools_for(inst, recs)
    recent = rand_hashes(np.random.default_rng(4), 63)
    before = snapshot(state, pool)
    with pytest.raises(bc.ChainPanic):
        bc.state_recalc_resident(pool, None, state, recent, 99)
    with pytest.raises(bc.ChainPanic):
        bc.state_recalc_device(pool_m, None, model, recent, 99)
    assert same(snapshot(state, pool), before)
    state.read()


def test_argument_errors_are_einval():
    import torch

    inst, recs = synthetic(4096, False, (32,))
    _, state = states_for(inst)
    _, pool = pools_for(inst, recs[:8])
    dll = _lib.lib.dll
    recent = put(np.frombuffer(b"".join(rand_hashes(np.random.default_rng(4), 64)), np.uint8))
    scratch = torch.zeros(int(dll.pz_state_recalc_scratch_bytes(state.nval, int(pool.caps[0]), state.nrec)) + 16, dtype=torch.uint8,
                          device="cuda:0")
    sh = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def batch(**over):
        kw = dict(nval=state.nval, balance=state.balance.data_ptr(), start=state.start.data_ptr(), end=state.end.data_ptr(),
                  members=state.members.data_ptr(), coffs=state.coffs.data_ptr(), recent=recent.data_ptr(), n_recent=64,
                  block_slot=99)
        kw.update(over)
        return ctypes.byref(_lib.RecalcBatch(**kw))

    before = snapshot(state, pool)
    call = dll.pz_dev_state_recalc
    assert call(None, pool._h, None, batch(), scratch.data_ptr(), sh) == _lib.PZ_EINVAL
    assert call(state._h, None, None, batch(), scratch.data_ptr(), sh) == _lib.PZ_EINVAL
    assert call(state._h, pool._h, None, None, scratch.data_ptr(), sh) == _lib.PZ_EINVAL
    assert call(state._h, pool._h, None, batch(), None, sh) == _lib.PZ_EINVAL
    assert call(state._h, pool._h, None, batch(), scratch.data_ptr() + 8, sh) == _lib.PZ_EINVAL
    assert call(state._h, pool._h, None, batch(recent=recent.data_ptr() + 8), scratch.data_ptr(), sh) == _lib.PZ_EINVAL
    for k in ("balance", "start", "end", "members", "coffs", "recent"):
        assert call(state._h, pool._h, None, batch(**{k: None}), scratch.data_ptr(), sh) == _lib.PZ_EINVAL, k
    assert call(state._h, pool._h, None, batch(n_recent=63), scratch.data_ptr(), sh) == _lib.PZ_EINDEX
    other = DeviceVoteCache(state.nval + 1, 8)  # nval different from the cache's
    assert call(state._h, pool._h, other._h, batch(), scratch.data_ptr(), sh) == _lib.PZ_EINVAL
    assert same(snapshot(state, pool), before)
    # pz_recalc_state_new: the stride's limits, and a record longer than the stride
    h = ctypes.c_void_p()
    sc = np.zeros(_lib.RS_COUNT, U64)
    one, offs = np.zeros(1, U64), np.array([0, 33], U64)
    hashes = np.zeros(33, np.uint8)
    for stride in (0, 16, 40, 272):
        assert dll.pz_recalc_state_new(0, stride, sc.ctypes.data, None, None, None, None, 0, ctypes.byref(h)) == _lib.PZ_EINVAL
    assert dll.pz_recalc_state_new(0, 32, None, None, None, None, None, 0, ctypes.byref(h)) == _lib.PZ_EINVAL
    assert dll.pz_recalc_state_new(1, 32, sc.ctypes.data, one.ctypes.data, one.ctypes.data, hashes.ctypes.data, offs.ctypes.data,
                                   0, ctypes.byref(h)) == _lib.PZ_ERANGE
    assert dll.pz_recalc_state_new(1, 48, sc.ctypes.data, one.ctypes.data, one.ctypes.data, hashes.ctypes.data, offs.ctypes.data,
                                   0, ctypes.byref(h)) == _lib.PZ_OK
    dll.pz_recalc_state_free(h)


def check_panic(state, model, pool, pool_m, cache, recent, block_slot):
    before = snapshot(state, pool)
    with pytest.raises(bc.ChainPanic):
        bc.state_recalc_device(pool_m, cache, model, recent, block_slot)
    with pytest.raises(bc.ChainPanic):
        bc.state_recalc_resident(pool, cache, state, recent, block_slot)
    after = state.read(strict=False)
    assert all(np.array_equal(after[k], before[0][k]) for k in after)  # scalars, records and winners as before
    np.testing.assert_array_equal(state.balances(), before[1])
    np.testing.assert_array_equal(state.balances(), model.balances())
    with pytest.raises(_lib.PzError) as e:  # sticky: the reference is dead
        state.read()
    assert e.value.code == _lib.PZ_EINDEX


def test_a_qualifying_attestation_of_a_shard_without_a_record_panics():
    """processCrosslinks indexes crosslinkRecords[ShardId] once the 2/3 test holds (core.go:549)."""
    inst, recs = synthetic(4096, False, (32,))
    model, state = states_for(inst, nrec=8)
    assert (inst["att_shard"] >= 8).any()
    pool_m, pool = pools_for(inst, recs)
    check_panic(state, model, pool, pool_m, None, rand_hashes(np.random.default_rng(4), 64), 99)


def test_the_rewards_panic_of_the_small_chain_at_full_participation():
    """1,024 validators, every committee member attesting: the attesters' deposit reaches two thirds
    and CalculateRewards reads CheckBit(last bitfield, validator index) past a 2-byte committee
    bitfield (incentives.go:23).  The oracle panics at the block of slot 64 of this chain."""
    nval = 1024
    blocks = synth.chain_blocks(nval, 64, seed=2, participation=(1.0, 0.5))
    assert blocks[63].slot_number == 64
    chain = oreplay.Chain(nval)
    cs0 = chain.C
    tab0 = table(cs0)
    args = ([v.balance for v in cs0.validators], [v.start_dynasty for v in cs0.validators],
            [v.end_dynasty for v in cs0.validators], [v for arr in tab0 for e in arr for v in e[1]],
            bc._committee_table(tab0)[3], cs0.crosslink_records)
    kw = dict(last_state_recalc=cs0.last_state_recalc, justified_streak=cs0.justified_streak,
              last_justified_slot=cs0.last_justified_slot, last_finalized_slot=cs0.last_finalized_slot,
              current_dynasty=cs0.current_dynasty, total_deposits=cs0.total_deposits)
    model, state = RecalcState(*args, **kw), ResidentRecalcState(*args, **kw)
    data, offs = bc.serialize_blocks(blocks[:63])
    caps = [256, 256 * 32, 256 * 32, 256 * 8, 256, 256 * 32, 512]
    pool_m, pool = DevicePendingAttestations(caps), DevicePendingAttestations(caps)
    n_recent = len(chain.A.data.recent_block_hashes)
    for p in (pool_m, pool):
        bc.pend_serialized_blocks(p, data, offs, cs0.last_justified_slot, cs0.last_state_recalc, n_recent, tab0)
    assert len(pool) > 0 and pool.records() == pool_m.records()
    for blk in blocks[:63]:
        assert chain.process_block(oreplay.to_pb_block(blk))["status"] == "processed"
    recent = [bytes(h) for h in chain.candidate[1].data.recent_block_hashes]
    assert pool.records() == [as_pb(a) for a in chain.candidate[1].data.pending_attestations]
    with pytest.raises(ref.GoPanic):
        chain.process_block(oreplay.to_pb_block(blocks[63]))
    check_panic(state, model, pool, pool_m, None, recent, blocks[63].slot_number)
