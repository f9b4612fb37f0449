"""The block gate (prysm_amd/csrc/blockgate.hip: pz_dev_block_gate / pz_block_gate,
blockchain.gate_blocks, blockchain.tally_serialized_blocks(tally_mixed=True)).

Two references.  Which blocks are open, which rows reach the pool and which rows of a clean block
are tallied: the torch composition the gate replaces (blockchain._open_blocks over
wire.folded_block_status), on random batches at the wave's edges.  What a mixed block adds to the
vote cache: oracle.ref, run as blockchain/service.go:281-318 runs it -- processAttestation over
every attestation, the last error's verdict, then calculate_block_vote_cache over every attestation
of the block, a GoError logged and passed over, a GoPanic ending everything -- compared voter- and
total-exact.  The state is 1,024 validators with the genesis committees and 128 recent hashes; a
genesis committee of 1,024 validators has 16 members, so no bitfield has padding bits, and the one
TRAILING_BITS case runs at 1,000 validators (15- and 16-member committees)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ref
from oracle import replay as oreplay
from prysm_amd import _lib, pb
from prysm_amd import blockchain as bc
from prysm_amd.pending import DevicePendingAttestations
from prysm_amd.votes import DeviceVoteCache
from test_attpool_gpu import as_pb
from test_votecache_gpu import State, att, put, snapshot, want

pytestmark = pytest.mark.gpu

U64 = np.uint64
PROCESSED = 0
CODES = [0, 2, 3, 4, 5, 6, 7, _lib.PZ_ERANGE, _lib.PZ_EINDEX]
POOL_CAPS = [512, 512 * 8, 512 * 8, 512 * 8, 512, 512 * 40, 512]


@functools.lru_cache(None)
def state(nval=1024):
    rng = np.random.default_rng(100 + nval)
    return State(nval, [rng.bytes(32) for _ in range(128)], balances=rng.integers(1, 1000, size=nval))


# ---- 1: the gate's outputs against the torch composition ----------------------------------------------
def synthetic(rng, st, rows_per_block):
    """Columns for blocks of the given sizes: check statuses of every code, bad top levels, bad
    records, candidates -- and scalars that keep every re-derivation inside the state's table."""
    n = len(rows_per_block)
    first = np.zeros(n + 1, U64)
    first[1:] = np.cumsum(rows_per_block, dtype=U64)
    natt = int(first[-1])
    status = np.where(rng.random(natt) < 0.7, 0, rng.choice(CODES, natt)).astype(np.int32)
    rec = np.where(rng.random(natt) < 0.97, 0, _lib.PZ_EINVAL).astype(np.int32)
    top = np.where(rng.random(n) < 0.85, 0, _lib.PZ_EINVAL).astype(np.int32)
    cand = (rng.random(n) < 0.7).astype(np.uint8)
    att_block = np.repeat(np.arange(n, dtype=np.int32), np.asarray(rows_per_block, dtype=np.int64))
    bslot = rng.integers(60, 70, natt).astype(U64)
    cols = {"slot": (bslot - rng.integers(0, 70, natt).astype(U64)).astype(U64), "block_slot": bslot,
            "n_oblique": rng.integers(0, 3, natt).astype(U64), "shard_id": rng.integers(0, 4, natt).astype(U64),
            "committee": rng.integers(0, 64, natt).astype(np.uint32), "parents_start": rng.integers(0, 64, natt).astype(U64)}
    return {"n": n, "natt": natt, "first": first, "status": status, "rec": rec, "top": top, "cand": cand,
            "att_block": att_block, "cols": cols, "table": bc._committee_table(st.tab)[:3], "narr": len(st.tab)}


def torch_reference(s, with_rec, with_cand):
    """report, pend_take and the tallied rows of blocks that are not mixed, by the composition of
    tally_serialized_blocks / _pend (blockchain._open_blocks, wire.folded_block_status)."""
    import torch

    from prysm_amd import wire

    n, natt = s["n"], s["natt"]
    if not natt:
        return np.zeros(n, np.uint8), np.zeros(0, np.uint8), np.zeros(0, bool), None
    dev = torch.device("cuda", 0)
    rec = put(s["rec"] if with_rec else np.zeros(natt, np.int32))
    status = torch.where(rec != 0, rec, put(s["status"]))
    att_block = put(s["att_block"])
    d = {"dev": dev, "n": n, "natt": natt, "blk": {"att_first": put(s["first"]), "att_block": att_block}, "status": status,
         "block_status": wire.folded_block_status(put(s["top"]), att_block, rec)}
    open_, ab, count, nproc = bc._open_blocks(d)
    report = open_.long() * (bc.BLOCK_TALLIED + (bc.BLOCK_MIXED - bc.BLOCK_TALLIED) * (nproc != count).long())
    open_c = bc._open_blocks(d, s["cand"] if with_cand else None)[0]
    take = open_c[ab] & (status == PROCESSED)
    tallied = (report == bc.BLOCK_TALLIED)[ab]
    return (report.cpu().numpy().astype(np.uint8), take.cpu().numpy().astype(np.uint8), tallied.cpu().numpy(),
            status.cpu().numpy())


def run_gate(s, st, form, with_rec, with_cand):
    """pz_dev_block_gate (on the current stream) or pz_block_gate over the synthetic batch; the
    check status it gets has the record status folded in, as _split_decode_check folds it."""
    import torch

    n, natt = s["n"], s["natt"]
    status = np.where((s["rec"] != 0) & with_rec, s["rec"], s["status"]).astype(np.int32)
    arrays = {"att_first": s["first"], "block_status": s["top"], "rec_status": s["rec"] if with_rec else None,
              "candidate": s["cand"] if with_cand else None, "status": status, **s["cols"],
              "arr_offs": s["table"][0], "arr_shard": s["table"][1], "arr_comm": s["table"][2],
              "report": np.full(n, 0xEE, np.uint8), "vote_status": np.full(natt, 0x5A5A5A5A, np.int32),
              "pend_take": np.full(natt, 0xEE, np.uint8), "flags": np.zeros(1, np.uint32)}
    arrays = {k: None if v is None else np.ascontiguousarray(v).copy() for k, v in arrays.items()}
    for k in ("committee", "parents_start", "vote_status"):  # required even when no block has a row
        if n and not natt:
            arrays[k] = np.zeros(1, arrays[k].dtype)
    if form == "host":
        held = arrays
        p = {k: _lib.ptr(v) for k, v in held.items()}
    else:
        held = {k: None if v is None else put(v) for k, v in arrays.items()}
        p = {k: _lib.dptr(v) for k, v in held.items()}
    chk = _lib.AttCheckBatch(natt=natt, slot=p["slot"], shard_id=p["shard_id"], n_oblique=p["n_oblique"],
                             block_slot=p["block_slot"], last_justified_slot=0, last_state_recalc=0, n_recent=128,
                             narr=s["narr"], arr_offs=p["arr_offs"], arr_shard=p["arr_shard"], arr_comm=p["arr_comm"],
                             status=p["status"], committee=p["committee"], parents_start=p["parents_start"])
    b = _lib.BlockGateBatch(nblocks=n, att_first=p["att_first"], block_status=p["block_status"], rec_status=p["rec_status"],
                            candidate=p["candidate"], chk=chk, report=p["report"], vote_status=p["vote_status"],
                            pend_take=p["pend_take"], flags=p["flags"])
    if form == "host":
        rc = _lib.lib.dll.pz_block_gate(ctypes.byref(b))
        out = {k: held[k] for k in ("report", "vote_status", "pend_take", "flags", "committee", "parents_start", "status")}
        assert rc == (_lib.PZ_EINDEX if out["flags"][0] & 1 else _lib.PZ_OK)
        return out
    _lib.lib.call("pz_dev_block_gate", ctypes.byref(b), _lib.stream_ptr(0))
    torch.cuda.current_stream().synchronize()
    out = {k: held[k].cpu().numpy() for k in ("report", "vote_status", "pend_take", "flags", "committee", "parents_start",
                                              "status")}
    out["flags"] = out["flags"].view(np.uint32)
    out["committee"] = out["committee"].view(np.uint32)
    out["parents_start"] = out["parents_start"].view(U64)
    return out


def compare(s, st, got, with_rec, with_cand):
    report, take, tallied, status = torch_reference(s, with_rec, with_cand)
    np.testing.assert_array_equal(got["report"], report)
    if not s["natt"]:
        return
    np.testing.assert_array_equal(got["pend_take"], take)
    plain = report[s["att_block"]] != bc.BLOCK_MIXED  # rows of clean and of rejected blocks
    np.testing.assert_array_equal((got["vote_status"] == PROCESSED)[plain], tallied[plain])
    clean = report[s["att_block"]] == bc.BLOCK_TALLIED
    assert (got["vote_status"][clean] == PROCESSED).all()
    np.testing.assert_array_equal(got["status"], status)  # the checks' column is read only
    # rows that are not re-derived keep the checks' committee and parents_start
    kept = ~np.isin(status, [2, 3, 4]) | (report[s["att_block"]] == bc.BLOCK_REJECTED)
    np.testing.assert_array_equal(got["committee"][kept], s["cols"]["committee"][kept])
    np.testing.assert_array_equal(got["parents_start"][kept], s["cols"]["parents_start"][kept])


def sizes_for(rng, nblocks):
    rows = rng.choice([0, 1, 2], nblocks).tolist()
    for k, big in zip(rng.permutation(nblocks)[:4].tolist(), (63, 64, 65, 130)):
        rows[k] = big
    return rows


@pytest.mark.parametrize("nblocks", [0, 1, 63, 64, 65, 257])
def test_gate_outputs_match_the_torch_composition(nblocks):
    import torch

    st = state()
    rng = np.random.default_rng(nblocks)
    s = synthetic(rng, st, sizes_for(rng, nblocks))
    assert nblocks < 4 or {63, 64, 65, 130} <= set(np.diff(s["first"].astype(np.int64)).tolist())
    first = None
    for with_rec, with_cand in ((True, True), (False, False), (True, False), (False, True)):
        got = run_gate(s, st, "device", with_rec, with_cand)
        compare(s, st, got, with_rec, with_cand)
        first = first or got
    # the host form and a caller's stream give the device form's bytes
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() != torch.cuda.default_stream()
        on_side = run_gate(s, st, "device", True, True)
    on_host = run_gate(s, st, "host", True, True)
    for other in (on_side, on_host):
        for k, v in first.items():
            np.testing.assert_array_equal(other[k], v, err_msg=k)


@pytest.mark.parametrize("rows", [0, 1, 2, 63, 64, 65, 130])
def test_gate_outputs_on_one_block(rows):
    st = state()
    rng = np.random.default_rng(1000 + rows)
    seen = set()
    for k in range(6):  # the last row decides: draw until the block has been open and closed
        s = synthetic(rng, st, [rows])
        if k % 2 and rows:
            s["status"][-1], s["top"][0], s["rec"][:] = PROCESSED, _lib.PZ_OK, _lib.PZ_OK
        with_rec, with_cand = bool(k & 1), bool(k & 2)
        got = run_gate(s, st, "device" if k % 3 else "host", with_rec, with_cand)
        compare(s, st, got, with_rec, with_cand)
        seen.add(int(got["report"][0]))
    assert seen == {0} if rows == 0 else seen & {1, 2}


# ---- 2: mixed blocks against the oracle -----------------------------------------------------------------
def rec_of(a, **kw):
    """An oracle-schema record (test_votecache_gpu.att) as a pb.AttestationRecord, edited."""
    f = dict(slot=a.slot, shard_id=a.shard_id, justified_slot=a.justified_slot, attester_bitfield=bytes(a.attester_bitfield),
             oblique_parent_hashes=[bytes(h) for h in a.oblique_parent_hashes])
    f.update(kw)
    return pb.AttestationRecord(**f)


def block(rng, slot, atts):
    return pb.BeaconBlock(parent_hash=rng.bytes(32), slot_number=slot, timestamp=pb.Timestamp(8 * slot, 0), attestations=atts)


class Panic(Exception):
    pass


def oracle_batch(st, blocks):
    """service.go:281-318 over the batch against one state -> (cache, pending, reports); GoPanic
    goes to the caller."""
    cache, pending, reports = {}, [], []
    for b in blocks:
        o = oreplay.to_pb_block(b)
        can, errors, passed = False, 0, []
        for a in o.attestations:
            try:
                ref.process_attestation(st.cs, st.active, o.slot_number, a)
                can = True
                passed.append(a)
            except ref.GoError:
                can = False
                errors += 1
        if not can:
            reports.append(bc.BLOCK_REJECTED)
            continue
        for a in o.attestations:
            try:
                ref.calculate_block_vote_cache(st.cs, st.active, cache, o.slot_number, a)
            except ref.GoError:
                pass  # service.go:315-317 logs it and goes on
        pending += passed
        reports.append(bc.BLOCK_MIXED if errors else bc.BLOCK_TALLIED)
    return cache, pending, reports


def device_batch(st, blocks, cache, pool=None, tally_mixed=True):
    """tally_serialized_blocks over the batch; a ChainPanic, or the tally's sticky PZ_EINDEX at the
    first read of the cache, is the reference's panic."""
    data, offs = bc.serialize_blocks(blocks)
    try:
        report, first, status = bc.tally_serialized_blocks(
            cache, data, offs, st.cs.last_justified_slot, st.cs.last_state_recalc, len(st.recent), st.tab,
            [r.tobytes() for r in st.recent], st.balance, pending=pool, candidate=None if pool is None else [1] * len(blocks),
            tally_mixed=tally_mixed)
        return list(report), status, snapshot(cache)
    except bc.ChainPanic as e:
        raise Panic(str(e)) from None
    except _lib.PzError as e:
        if e.code != _lib.PZ_EINDEX:
            raise
        raise Panic(str(e)) from None


def cases(nval=1024):
    """name -> (state, blocks): one block each, its last attestation passing (or, for the closed
    block, failing) and the named attestation before it."""
    rng = np.random.default_rng(7)
    st = state(nval)
    last = lambda slot: rec_of(att(st, slot, rng, [rng.bytes(33)], j=1))  # noqa: E731
    a5 = att(st, 5, rng)
    short = bytes(a5.attester_bitfield)[:-1]
    out = {
        "justified": [block(rng, 10, [rec_of(att(st, 3, rng), justified_slot=9), last(4)])],
        "slot-low-m1": [block(rng, 70, [rec_of(att(st, 5, rng, [rng.bytes(33)])), last(10)])],
        "slot-low-m0": [block(rng, 70, [rec_of(att(st, 5, rng)), last(10)])],
        "slot-high": [block(rng, 10, [rec_of(att(st, 11, rng)), last(4)])],
        "no-committee": [block(rng, 10, [rec_of(att(st, 3, rng), shard_id=999), last(4)])],
        "bitfield-short": [block(rng, 10, [rec_of(a5, attester_bitfield=short), last(4)])],
        "bitfield-short-all-skipped": [block(rng, 10, [rec_of(a5, attester_bitfield=short,
                                                              oblique_parent_hashes=[rng.bytes(32) for _ in range(64)]), last(4)])],
        "bitfield-long": [block(rng, 10, [rec_of(a5, attester_bitfield=bytes(a5.attester_bitfield) + b"\xff"), last(4)])],
        "erange-in-closed-block": [block(rng, 10, [rec_of(att(st, 3, rng, [rng.bytes(32) for _ in range(65)])),
                                                   rec_of(att(st, 4, rng), justified_slot=9)])],
    }
    twice = att(st, 6, rng, [rng.bytes(33)])
    out["repeated-voters"] = [block(rng, 10, [rec_of(twice, justified_slot=9), rec_of(twice)])]
    return st, out


def recalc64_case():
    """last_state_recalc = 64, slot = 60, block slot 126, m = 2: SLOT_LOW, the slice [66:128] fits,
    idx = 60 - 64 wraps (core.go:367)."""
    rng = np.random.default_rng(8)
    st = State(1024, [rng.bytes(32) for _ in range(128)], balances=rng.integers(1, 1000, size=1024))
    st.cs.last_state_recalc = 64
    a = att(st, 70, rng, [rng.bytes(33), rng.bytes(33)])
    return st, [block(rng, 126, [rec_of(a, slot=60), rec_of(att(st, 100, rng, j=1))])]


def trailing_case():
    rng = np.random.default_rng(9)
    st = state(1000)
    slot = next(s for s in range(1, 60) if len(st.committee(s)[1]) % 8)
    a = att(st, slot, rng, [rng.bytes(33)])
    bits = bytes(a.attester_bitfield)
    return st, [block(rng, 61, [rec_of(a, attester_bitfield=bits[:-1] + bytes([bits[-1] | 1])), rec_of(att(st, slot, rng, j=1))])]


PANICS = {"slot-low-m0", "slot-high", "bitfield-short", "erange-in-closed-block", "recalc64"}
ONE_BLOCK = ["justified", "slot-low-m1", "slot-low-m0", "slot-high", "recalc64", "no-committee", "bitfield-short",
             "bitfield-short-all-skipped", "bitfield-long", "trailing-bits", "repeated-voters", "erange-in-closed-block"]


def one_block(name):
    if name == "recalc64":
        return recalc64_case()
    if name == "trailing-bits":
        return trailing_case()
    st, out = cases()
    return st, out[name]


@pytest.mark.parametrize("name", ONE_BLOCK)
def test_one_block_per_rederivation_case(name):
    st, blocks = one_block(name)
    try:
        o_cache, o_pending, o_reports = oracle_batch(st, blocks)
        o_panic = False
    except ref.GoPanic:
        o_panic = True
    assert o_panic == (name in PANICS)  # (what the issue's arithmetic says; the oracle decides)
    cache, pool = DeviceVoteCache(st.nval, 512), DevicePendingAttestations(POOL_CAPS)
    try:
        report, status, got = device_batch(st, blocks, cache, pool)
        panic = False
    except Panic:
        panic = True
    assert panic == o_panic
    if panic:
        return
    assert report == o_reports == [bc.BLOCK_MIXED]
    assert got == want(o_cache)
    assert pool.records() == [as_pb(a) for a in o_pending]
    # what the named row did, from the oracle alone
    alone = oracle_batch(st, [block(np.random.default_rng(0), blocks[0].slot_number, blocks[0].attestations[1:])])[0]
    o = oreplay.to_pb_block(blocks[0])
    if name in ("no-committee", "bitfield-short-all-skipped"):
        assert want(o_cache) == want(alone)  # nothing came of the failed row
    elif name == "slot-low-m1":
        parents = ref.get_signed_parent_hashes(st.active, 70, o.attestations[0])
        assert parents[:63] == [r.tobytes() for r in st.recent[65:128]] and all(h in o_cache for h in parents)
    elif name == "repeated-voters":
        assert want(o_cache) == want(alone)  # the same voters on the same parents: no total moves
    else:
        assert len(o_cache) > len(alone)
    if name == "bitfield-long":
        assert int(status[0]) == 6
    if name == "trailing-bits":
        assert int(status[0]) == 7


def test_one_batch_of_every_quiet_case():
    """All the cases that do not panic, a clean block, a rejected one (its first row passes) and one
    without attestations, in one batch; tally_mixed=False on a twin leaves the mixed blocks out, as
    before."""
    st, out = cases()
    rng = np.random.default_rng(11)
    quiet = [n for n in ONE_BLOCK if n in out and n not in PANICS]
    blocks = [out[n][0] for n in quiet]
    clean = block(rng, 12, [rec_of(att(st, 7, rng)), rec_of(att(st, 8, rng, [rng.bytes(5)], j=1))])
    rejected = block(rng, 12, [rec_of(att(st, 7, rng, j=1)), rec_of(att(st, 8, rng), justified_slot=9)])
    blocks = blocks[:2] + [clean, rejected, block(rng, 13, [])] + blocks[2:]
    o_cache, o_pending, o_reports = oracle_batch(st, blocks)
    assert o_reports == [2, 2, 1, 0, 0] + [2] * (len(quiet) - 2) and len(quiet) == 6
    cache, pool = DeviceVoteCache(st.nval, 1024), DevicePendingAttestations(POOL_CAPS)
    report, status, got = device_batch(st, blocks, cache, pool)
    assert report == o_reports
    assert got == want(o_cache)
    assert pool.records() == [as_pb(a) for a in o_pending]
    # the default on a twin: the clean block alone, and the same report
    twin = DeviceVoteCache(st.nval, 1024)
    report0, status0, got0 = device_batch(st, blocks, twin, tally_mixed=False)
    assert report0 == o_reports and np.array_equal(status0, status)
    assert got0 == want(oracle_batch(st, [clean])[0]) and got0 != got


# ---- 3: a chain with refused attestations in processed blocks -----------------------------------------------
def test_edited_chain_block_by_block_beside_the_oracle():
    """tests/test_replay.py's edited_chain() (1,000 validators; five refused attestations, four of
    them in blocks the reference processes), block by block with tally_mixed=True against the oracle
    chain's state just before each block, as test_tally_serialized_blocks_matches_the_engine steps.
    A block whose parent was never saved does not reach the attestations (service.go:261-269): the
    walk's decision, taken here from the oracle's record."""
    from test_attcheck_gpu import table
    from test_replay import edited_chain

    nval = 1000
    blocks = edited_chain()
    data, offs = bc.serialize_blocks(blocks)
    engine = bc.BeaconChain(nval)
    engine.process_serialized(data, offs)
    chain = oreplay.Chain(nval)
    cache, pool = DeviceVoteCache(nval, 512), DevicePendingAttestations(POOL_CAPS)
    tables, reports = {}, []
    for i, blk in enumerate(blocks):
        C, A = chain.C, chain.A.data
        if C.last_state_recalc not in tables:
            tables[C.last_state_recalc] = table(C)
        before = (C.last_justified_slot, C.last_state_recalc, tables[C.last_state_recalc],
                  [bytes(h) for h in A.recent_block_hashes], np.array([v.balance for v in C.validators], U64))
        r = chain.process_block(oreplay.to_pb_block(blk))
        if r["status"] == "no_parent":
            continue
        assert not r["transition"]
        lo, hi = int(offs[i]), int(offs[i + 1])
        report, first, status = bc.tally_serialized_blocks(
            cache, data[lo:hi], np.array([0, hi - lo], dtype=U64), before[0], before[1], len(before[3]), before[2],
            before[3], before[4], pending=pool, candidate=[1], tally_mixed=True)
        errors = sum("error" in a for a in r["atts"])
        assert list(report) == [0 if r["status"] == "attestations_rejected" else 2 if errors else 1], i
        assert int((status != PROCESSED).sum()) == errors
        reports.append(int(report[0]))
    assert reports.count(bc.BLOCK_MIXED) == 4 and reports.count(bc.BLOCK_REJECTED) == 1
    _, A, _ = chain.candidate
    assert snapshot(cache) == want(A.cache)
    assert cache.items() == engine.roots()["vote_totals"]
    assert pool.records() == [as_pb(a) for a in A.data.pending_attestations]


# ---- 4: a panicking call leaves nothing behind ------------------------------------------------------------
@pytest.mark.parametrize("name", ["slot-high", "slot-low-m0", "erange-in-closed-block"])
def test_a_panicking_batch_changes_neither_cache_nor_pool(name):
    st, out = cases()
    cache, pool = DeviceVoteCache(st.nval, 512), DevicePendingAttestations(POOL_CAPS)
    twin, twin_pool = DeviceVoteCache(st.nval, 512), DevicePendingAttestations(POOL_CAPS)
    for c, p in ((cache, pool), (twin, twin_pool)):
        device_batch(st, out["justified"], c, p)
    rng = np.random.default_rng(12)
    clean = block(rng, 12, [rec_of(att(st, 7, rng)), rec_of(att(st, 8, rng, j=1))])
    with pytest.raises(Panic):
        device_batch(st, [clean] + out[name], cache, pool)  # (the clean block of the batch does not land either)
    assert snapshot(cache) == snapshot(twin) and snapshot(twin)
    assert pool.records() == twin_pool.records() and len(pool) == 1
