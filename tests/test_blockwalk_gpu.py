"""The block walk and the resident RecentBlockHashes on the GPU (prysm_amd/csrc/blockwalk.hip;
pending.DeviceRecentHashes, blockchain.walk_serialized_blocks):

1. the three kernels on synthetic columns, device and host forms, against a block-by-block Python
   restatement of blockchain/service.go:320-333, with canary bytes behind every output;
2. the ring alone: the append against a list model, its view under pz_dev_active_state_bytes;
3. blocks 1..63 of the 130-block chain in ONE call against oracle.replay.Chain stepped block by block;
4. siblings, a mixed block, a refused block and an ineligible block in one run;
5. the whole chain across both transitions, in calls cut at ``stop``;
6. a panic row in a run leaves cache, pool and ring as they were."""
import ctypes

import numpy as np
import pytest

from oracle import ref
from oracle import replay as oreplay
from prysm_amd import _lib, pb
from prysm_amd import blockchain as bc
from prysm_amd.pending import DevicePendingAttestations, DeviceRecentHashes
from prysm_amd.votes import DeviceVoteCache
from test_attpool_gpu import as_pb, late_chain, table
from test_votecache_gpu import snapshot, want

pytestmark = pytest.mark.gpu

U64 = np.uint64
PROCESSED, NOT_PROCESSED = 0, 1
CAPS = [256, 256 * 32, 256 * 32, 256 * 8, 256, 256 * 32, 512]
CANARY = 0xA5
FAR = 1 << 40  # a lastStateRecalc no slot of the synthetic cases reaches


# ---- 1: the kernels on synthetic columns ------------------------------------------------------------------
def make(rng, n, go, slot_of, has0=0, cslot0=0, lsr=FAR, lag=0):
    """A run of n blocks: go in {"all", "none", "alt", "random"}; 0-3 rows per block."""
    report = {"all": lambda j: 1 + j % 2, "none": lambda j: 0, "alt": lambda j: j % 2,
              "random": lambda j: int(rng.integers(0, 3))}[go]
    rows = rng.integers(0, 4, size=n)
    natt = int(rows.sum())
    ring, ring_len = rng.integers(0, 256, size=(129, 32), dtype=np.uint8), np.full(129, 32, np.uint8)
    if rng.integers(0, 2):  # a ring nothing was appended to yet: any stored lengths, no history
        ring[0], ring_len = 0, np.append(0, rng.integers(0, 33, size=128)).astype(np.uint8)
    return {"n": n, "ring": ring, "ring_len": ring_len, "has0": has0, "cslot0": cslot0, "lsr": lsr, "lag": lag,
            "slot": np.array([slot_of(j) for j in range(n)], U64), "report": np.array([report(j) for j in range(n)], np.uint8),
            "hash": rng.integers(0, 256, size=(n, 32), dtype=np.uint8),
            "att_block": np.repeat(np.arange(n, dtype=np.uint32), rows), "parents_start": rng.integers(0, 65, size=natt).astype(U64),
            "pend_take": rng.integers(0, 2, size=natt).astype(np.uint8),
            "vote_status": rng.choice(np.array([0, 0, 0, 1, 4, 6], np.int32), size=natt)}


def model(r):
    """service.go:320-333 block by block, with a list that only grows (core.go:223-237)."""
    n, lag = r["n"], r["lag"]
    walk, base = np.full(n, 3, np.uint8), np.zeros(n, U64)
    hashes, lens = [h.tobytes() for h in r["ring"]], list(r["ring_len"])
    has, cslot, ncand, stop = bool(r["has0"]), r["cslot0"] if r["has0"] else 0, 0, n
    for j in range(n):
        slot = int(r["slot"][j])
        if lag and ncand:
            stop = j
            break
        base[j] = len(hashes) - 128 - lag
        if not r["report"][j]:
            walk[j] = 0
            continue
        had = has
        if has and slot > cslot and slot > 1:
            has = False
        if has:
            walk[j] = 1
            continue
        if slot >= (r["lsr"] + 64) % (1 << 64):
            has, stop, base[j] = had, j, 0
            break
        hashes.append(r["hash"][j].tobytes())
        lens = [32] * (len(lens) + 1)  # RecentBlockHashes() is stored back whole, every entry 32 bytes
        has, cslot, ncand, walk[j] = True, slot, ncand + 1, 2
    log = np.zeros((129 + n, 32), np.uint8)
    log[:len(hashes)] = np.frombuffer(b"".join(hashes), np.uint8).reshape(-1, 32)
    b = r["att_block"].astype(np.int64)
    live = b < stop
    ps = r["parents_start"] + np.where(live, base[b] if n else 0, 0).astype(U64)
    take = (r["pend_take"] != 0) & (walk[b] == 2) if n else r["pend_take"] != 0
    vs = np.where(~live & (r["vote_status"] == PROCESSED), NOT_PROCESSED, r["vote_status"]).astype(np.int32)
    return {"walk": walk, "base": base, "result": np.array([stop, ncand, has, cslot], U64), "log": log,
            "ring": log[ncand:ncand + 129].copy(), "ring_len": np.array(lens[-129:], np.uint8),
            "parents_start": ps, "pend_take": take.astype(np.uint8), "vote_status": vs}


def padded(a, pad=64):
    """A device copy of ``a`` with canary bytes behind it: ``(whole uint8 buffer, the view)``."""
    import torch

    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    nbytes = raw.size + (-raw.size) % 16
    host = np.full(nbytes + pad, CANARY, np.uint8)
    host[:raw.size] = raw
    return torch.from_numpy(host).cuda(), raw.size


def run_device(r):
    import torch

    n, natt = r["n"], len(r["att_block"])
    ring = ring_of(r["ring"], r["ring_len"])
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    ins = {k: put(r[k]) for k in ("slot", "report", "hash", "att_block")}
    outs = {"walk": padded(np.full(n, CANARY, np.uint8)), "base": padded(np.full(n, 0xA5A5, U64)),
            "result": padded(np.full(4, 0xA5A5, U64)), "log": padded(np.full((129 + n) * 32, CANARY, np.uint8)),
            "parents_start": padded(r["parents_start"]), "pend_take": padded(r["pend_take"]), "vote_status": padded(r["vote_status"])}
    p = {k: (t.data_ptr() if used else None) for k, (t, used) in outs.items()}
    b = _lib.BlockWalkBatch(nblocks=n, slot_number=_lib.dptr(ins["slot"]), report=_lib.dptr(ins["report"]),
                            block_hash=_lib.dptr(ins["hash"]), has_candidate=r["has0"], candidate_slot=r["cslot0"],
                            last_state_recalc=r["lsr"], lag=r["lag"], natt=natt, att_block=_lib.dptr(ins["att_block"]),
                            vote_status=p["vote_status"], pend_take=p["pend_take"], parents_start=p["parents_start"],
                            walk=p["walk"], base=p["base"], result=p["result"], log=outs["log"][0].data_ptr())
    _lib.lib.call("pz_dev_block_walk", ring._h, ctypes.byref(b), _lib.stream_ptr(0))
    torch.cuda.synchronize()
    got = {}
    dtypes = {"walk": np.uint8, "base": U64, "result": U64, "log": np.uint8, "parents_start": U64, "pend_take": np.uint8,
              "vote_status": np.int32}
    for k, (t, used) in outs.items():
        host = t.cpu().numpy()
        assert (host[used:] == CANARY).all(), k  # nothing is written behind an output
        got[k] = host[:used].view(dtypes[k])
    got["log"] = got["log"].reshape(-1, 32)
    got["ring"], got["ring_len"] = ring.read(history=True)
    return got


def ring_of(rows, lens):
    """A ring whose 129 entries, the history entry included, are the given ones: a fresh one (zero
    history), or one made from entries 0..127 and rolled once by the host append of entry 128, after
    which every length is 32."""
    if not lens[0]:
        assert not rows[0].any()
        return DeviceRecentHashes(rows[1:], lens[1:])
    assert (lens == 32).all()
    ring = DeviceRecentHashes(rows[:128])
    ring.append(rows[128:129])
    return ring


def run_host(r):
    n, natt = r["n"], len(r["att_block"])
    ring = ring_of(r["ring"], r["ring_len"])
    got = {"walk": np.full(n, CANARY, np.uint8), "base": np.full(n, 0xA5A5, U64), "result": np.full(4, 0xA5A5, U64),
           "log": np.full((129 + n, 32), CANARY, np.uint8), "parents_start": r["parents_start"].copy(),
           "pend_take": r["pend_take"].copy(), "vote_status": r["vote_status"].copy()}
    hp = _lib.ptr
    b = _lib.BlockWalkBatch(nblocks=n, slot_number=hp(r["slot"]), report=hp(r["report"]), block_hash=hp(r["hash"]),
                            has_candidate=r["has0"], candidate_slot=r["cslot0"], last_state_recalc=r["lsr"], lag=r["lag"],
                            natt=natt, att_block=hp(r["att_block"]), vote_status=hp(got["vote_status"]),
                            pend_take=hp(got["pend_take"]), parents_start=hp(got["parents_start"]), walk=hp(got["walk"]),
                            base=hp(got["base"]), result=got["result"].ctypes.data, log=got["log"].ctypes.data)
    _lib.lib.call("pz_block_walk", ring._h, ctypes.byref(b))
    got["ring"], got["ring_len"] = ring.read(history=True)
    return got


def runs_for(n, rng):
    mk = lambda *a, **kw: make(rng, n, *a, **kw)  # noqa: E731
    up = lambda j: 2 + j  # noqa: E731
    out = [("all", mk("all", up)), ("none", mk("none", up, has0=1, cslot0=1)), ("alternating", mk("alt", up)),
           ("siblings", mk("all", lambda j: 7 + j // 2, has0=1, cslot0=3)), ("decreasing", mk("all", lambda j: 2 + n - j)),
           ("slots 0 and 1", mk("all", lambda j: j % 2)), ("slots 0 and 1, carried 0", mk("all", lambda j: j % 2, has0=1)),
           ("slots 1 and 0, carried 0", mk("alt", lambda j: (j + 1) % 2, has0=1)),
           ("carried above all", mk("all", up, has0=1, cslot0=1 << 50)),
           ("lag, first candidate at 0", mk("all", lambda j: 5 + j, lag=1)),
           ("lag, first candidate at 1024", mk("all", lambda j: 5 if j < 1024 else 6 + j, has0=1, cslot0=5, lag=1)),
           ("lag, no candidate", mk("all", lambda j: 5, has0=1, cslot0=5, lag=1)),
           ("random", mk("random", lambda j: int(rng.integers(0, 140)), has0=int(rng.integers(0, 2)), cslot0=3, lsr=64))]
    for at in sorted({0, n // 2, max(n - 1, 0), 1024, 1025}):
        if at < n:
            out.append(("transition at %d" % at, mk("all", lambda j: 10 + j // 40 if j < at else 10000 + j, has0=at % 2, cslot0=5, lsr=9000)))
            out.append(("transition at %d after candidates" % at, mk("alt", lambda j: 10 + j if j < at else 10000 + j, lsr=9000)))
    return out


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_kernels_on_synthetic_columns(n, form):
    rng = np.random.default_rng(1000 + n)
    classes = set()
    for name, r in runs_for(n, rng):
        want_ = model(r)
        got = (run_device if form == "device" else run_host)(r)
        if n == 0:  # nothing is launched: the outputs and the ring stay as they were
            np.testing.assert_array_equal(got["ring"], r["ring"], name)
            if form == "host":
                assert list(got["result"]) == [0, 0, r["has0"], r["cslot0"] if r["has0"] else 0], name
            continue
        for k in ("walk", "base", "result", "log", "parents_start", "pend_take", "vote_status", "ring"):
            np.testing.assert_array_equal(got[k], want_[k], "%s: %s" % (name, k))
        np.testing.assert_array_equal(got["ring_len"], want_["ring_len"], name)
        classes |= set(want_["walk"].tolist())
    if n >= 63:
        assert classes == {0, 1, 2, 3}


# ---- 2: the ring alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("n", [0, 1, 128, 129, 300])
def test_append_against_a_list(n, form):
    import torch

    rng = np.random.default_rng(n)
    first = [rng.bytes(int(k)) for k in rng.integers(0, 33, size=128)]
    ring = DeviceRecentHashes(first)
    hist = [b""] + first  # 129 entries, the history entry first (zeros, length 0)
    for take in (None, rng.integers(0, 2, size=n).astype(np.uint8), np.zeros(n, np.uint8)):
        h = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        if form == "device":
            ring.append(torch.from_numpy(h).cuda(), None if take is None else torch.from_numpy(take).cuda())
        else:
            ring.append(h, take)
        taken = [h[j].tobytes() for j in range(n) if take is None or take[j]]
        if taken:  # RecentBlockHashes() -- every entry as [32]byte -- plus the new ones is stored back whole
            hist = ([ref.bytes_to_hash(x) for x in hist] + taken)[-129:]
        rows, lens = ring.read(history=True)
        assert [rows[i, 32 - int(lens[i]):].tobytes() for i in range(129)] == hist
        assert all(not rows[i, :32 - int(lens[i])].any() for i in range(129))
        assert ring.hashes() == hist[1:]
        v_rows, v_lens = ring.view()
        np.testing.assert_array_equal(v_rows.cpu().numpy(), rows[1:])
        np.testing.assert_array_equal(v_lens.cpu().numpy(), lens[1:])


def test_view_under_the_active_state_encoder():
    """pz_dev_active_state_bytes over the ring's view gives the bytes the list form gives, stored
    lengths included; the Python face takes the ring in place of the list."""
    import torch

    rng = np.random.default_rng(3)
    stored = [rng.bytes(int(k)) for k in rng.integers(0, 33, size=128)]
    pool = DevicePendingAttestations([4, 64, 64, 64, 4, 64, 4])
    ring = DeviceRecentHashes(stored)
    lens = np.array([len(h) for h in stored], np.uint8)
    assert ring.hashes() == stored and len(set(lens)) > 8  # as stored: lengths of every kind
    assert pool.active_state(ring) == pool.active_state(stored, lens)
    ring.append(rng.integers(0, 256, size=(5, 32), dtype=np.uint8))
    hashes = ring.hashes()
    assert hashes[:123] == [ref.bytes_to_hash(h) for h in stored[5:]] and all(len(h) == 32 for h in hashes)
    ring = DeviceRecentHashes(stored)  # the device encoder below sees lengths of every kind
    hashes = stored
    want_bytes = pool.active_state(hashes, lens)
    assert pool.active_state(ring) == want_bytes and pool.active_state_root(ring) == pool.active_state_root(hashes, lens)
    d_rows, d_lens = ring.view()
    counts = pool.counts()
    cap = int(_lib.lib.dll.pz_active_state_bound(counts.ctypes.data, 128))
    out = torch.full((cap + 16,), CANARY, dtype=torch.uint8, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.lib.call("pz_dev_active_state_bytes", pool._h, d_rows.data_ptr(), d_lens.data_ptr(), 128, out.data_ptr(), cap,
                  total.data_ptr(), _lib.stream_ptr(0))
    got = out.cpu().numpy()
    assert got[:int(total.item())].tobytes() == want_bytes and (got[int(total.item()):] == CANARY).all()


def test_a_shorter_ring_is_refused():
    with pytest.raises(_lib.PzError) as e:
        DeviceRecentHashes([b"\x01" * 32] * 127)
    assert e.value.code == _lib.PZ_EINVAL
    assert DeviceRecentHashes().hashes() == [b""] * 128  # the genesis ring


# ---- 3: one run, one call ------------------------------------------------------------------------------------
def genesis_objects(nval):
    chain = oreplay.Chain(nval)
    C = chain.C
    return chain, DeviceVoteCache(nval, 512), DevicePendingAttestations(CAPS), DeviceRecentHashes(), table(C), \
        np.array([v.balance for v in C.validators], U64)


def check_against(chain, cache, pool, ring):
    _, A, _ = chain.candidate
    assert snapshot(cache) == want(A.cache)
    assert pool.records() == [as_pb(a) for a in A.data.pending_attestations]
    assert ring.hashes() == [bytes(h) for h in A.data.recent_block_hashes]


def check_digests(out, recs):
    """Every row's message digest against the oracle's records: zero where processAttestation
    refused the row or never ran (the parent was not saved)."""
    first = out["att_first"]
    for j, rec in enumerate(recs):
        rows = range(int(first[j]), int(first[j + 1]))
        if rec["status"] == "no_parent":
            assert not out["msg"][list(rows)].any(), j
            continue
        assert len(rec["atts"]) == len(rows), j
        for i, a in zip(rows, rec["atts"]):
            if "msg" in a:
                assert out["msg"][i].tobytes() == a["msg"] and int(out["msg_len"][i]) == a["msg_len"], (j, i)
            else:
                assert not out["msg"][i].any() and out["att_status"][i] != PROCESSED, (j, i)


def test_a_cycle_of_blocks_in_one_call():
    """Blocks 1..63 of late_chain(1024, 130, seed=4) through walk_serialized_blocks in a single call,
    with no hash list from the host, against the oracle stepped block by block.  The same blocks
    through one tally_serialized_blocks call (one window for all) do not reproduce the oracle's
    cache: the oracle's holds the run's own block hashes as keys, which no single window has."""
    nval = 1024
    blocks = late_chain(nval, 130, seed=4)[:63]
    data, offs = bc.serialize_blocks(blocks)
    chain, cache, pool, ring, tab, balance = genesis_objects(nval)
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks]
    assert [r["status"] for r in recs] == ["processed"] * 63 and not any(r["transition"] for r in recs)
    o_cache = chain.candidate[1].cache
    assert sum(r["hash"] in o_cache for r in recs) > 30  # (CPU: the window matters on this input)

    out = bc.walk_serialized_blocks(cache, pool, ring, data, offs, 0, 0, tab, balance, want_digests=True)
    assert out["ncand"] == 63 and out["stop"] == 63 and (out["walk"] == bc.WALK_CANDIDATE).all()
    assert out["has_candidate"] and out["candidate_slot"] == 63
    assert [h.tobytes() for h in out["block_hash"]] == [r["hash"] for r in recs]
    first = out["att_first"]
    starts = {int(out["parents_start"][int(first[j])]) for j in range(63)}
    assert len(starts) >= 2 and (out["att_status"] == PROCESSED).all()
    check_against(chain, cache, pool, ring)
    _, lens = ring.read()
    assert list(lens) == [32] * 128 and ring.hashes()[:65] == [bytes(32)] * 65  # stored back whole, as [32]byte
    check_digests(out, recs)

    single = DeviceVoteCache(nval, 512)
    report, _, _ = bc.tally_serialized_blocks(single, data, offs, 0, 0, 128, tab, [b""] * 128, balance, tally_mixed=True)
    assert (report == bc.BLOCK_TALLIED).all() and snapshot(single) != want(o_cache)


# ---- 4: siblings and refusals in one run ---------------------------------------------------------------------
def test_siblings_refusals_and_an_ineligible_block_in_one_run():
    """The block builders of test_pend_serialized_blocks_rejected_and_mixed_blocks: two blocks at one
    slot, a mixed block, a block whose last attestation fails and an ineligible block between
    candidates, against the oracle with ``saved`` seeded so that the parent check gives ``eligible``."""
    rng = np.random.default_rng(10)
    nval = 1024
    chain, cache, pool, ring, tab, balance = genesis_objects(nval)

    def rec8(slot, j, good=True):
        shard, comm = tab[slot][j % len(tab[slot])]
        bits = rng.random(len(comm)) < 0.6
        return pb.AttestationRecord(slot=slot, shard_id=shard, justified_slot=0 if good else 9,
                                    attester_bitfield=np.packbits(bits.astype(np.uint8)).tobytes(),
                                    oblique_parent_hashes=[rng.bytes(33)])

    def block(slot, atts):
        return pb.BeaconBlock(parent_hash=rng.bytes(32), slot_number=slot, timestamp=pb.Timestamp(8 * slot, 0), attestations=atts)

    blocks = [block(5, [rec8(1, 0), rec8(2, 1)]), block(5, [rec8(2, 0)]), block(6, [rec8(3, 0, good=False), rec8(3, 1)]),
              block(7, [rec8(1, 0), rec8(2, 0, good=False)]), block(8, [rec8(1, 1)]), block(9, [rec8(4, 0), rec8(1, 1)]),
              block(9, [rec8(2, 1)])]
    eligible = [1, 1, 1, 1, 0, 1, 1]
    for b, e in zip(blocks, eligible):
        if e:
            chain.saved.add(ref.copy32(b.parent_hash))
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks]
    assert [r["status"] for r in recs] == ["processed", "saved_not_candidate", "processed", "attestations_rejected", "no_parent",
                                          "processed", "saved_not_candidate"]
    data, offs = bc.serialize_blocks(blocks)
    out = bc.walk_serialized_blocks(cache, pool, ring, data, offs, 0, 0, tab, balance, eligible=eligible, want_digests=True)
    assert list(out["walk"]) == [2, 1, 2, 0, 0, 2, 1] and list(out["report"]) == [1, 1, 2, 0, 0, 1, 1]
    assert (out["stop"], out["ncand"], out["has_candidate"], out["candidate_slot"]) == (7, 3, True, 9)
    first = out["att_first"]
    base = [int(out["parents_start"][int(first[j])]) - (blocks[j].slot_number - blocks[j].attestations[0].slot) for j in range(7)]
    assert base == [1, 2, 2, 3, 3, 3, 4]  # the windows, after the gap too
    check_against(chain, cache, pool, ring)
    check_digests(out, recs)
    assert ring.hashes()[-3:] == [recs[0]["hash"], recs[2]["hash"], recs[5]["hash"]]


# ---- 5: across both transitions --------------------------------------------------------------------------------
def test_the_chain_across_both_transitions():
    """The 130-block chain in calls cut at ``stop``: a transition block goes through the existing
    pieces (the tally, state_recalc_resident over the ring, the pool append, ring.append), the block
    after it is one call with lag=1, the pre-transition scalars and a kept copy of the pre-transition
    balances, and the rest of each cycle is one call."""
    from test_state_wire_gpu import check_states, genesis_resident

    nval, nblocks = 1024, 130
    blocks = late_chain(nval, nblocks, seed=4)
    data, offs = bc.serialize_blocks(blocks)
    chain, cache, pool, ring, _, _ = genesis_objects(nval)
    state, _ = genesis_resident(chain.C)

    def span(lo, hi):
        return data[int(offs[lo]):int(offs[hi])], (offs[lo:hi + 1] - offs[lo]).astype(U64)

    def scalars():
        return (state.last_justified_slot, state.last_state_recalc, table(chain.C), state.balances().copy())

    i, has, cslot, lag, pre = 0, False, 0, 0, None
    calls, transitions, stops = [], 0, []
    while i < nblocks:
        ljs, lsr, tab, balance = pre if lag else scalars()
        d, o = span(i, nblocks)
        out = bc.walk_serialized_blocks(cache, pool, ring, d, o, ljs, lsr, tab, balance, has_candidate=has, candidate_slot=cslot, lag=lag)
        stop = out["stop"]
        calls.append((i, stop, lag))
        assert stop >= 1 and (out["walk"][:stop] == bc.WALK_CANDIDATE).all() and (out["walk"][stop:] == bc.WALK_DEFERRED).all()
        for b in blocks[i:i + stop]:
            r = chain.process_block(oreplay.to_pb_block(b))
            assert r["status"] == "processed" and not r["transition"]
        i, has, cslot = i + stop, out["has_candidate"], out["candidate_slot"]
        if lag:
            assert stop == 1
            lag = 0
            continue
        if i == nblocks:
            break
        # block i is a cycle transition: the existing pieces, in the reference's order
        blk = blocks[i]
        stops.append(blk.slot_number)
        ljs, lsr, tab, balance = pre = scalars()
        assert blk.slot_number >= lsr + 64
        d, o = span(i, i + 1)
        report, _, status = bc.tally_serialized_blocks(cache, d, o, ljs, lsr, 128, tab, ring.read()[0], balance, tally_mixed=True)
        assert list(report) == [bc.BLOCK_TALLIED]
        bc.state_recalc_resident(pool, cache, state, ring, blk.slot_number)
        bc.pend_serialized_blocks(pool, d, o, ljs, lsr, 128, tab, candidate=[1])
        ring.append(out["block_hash"][stop:stop + 1])
        r = chain.process_block(oreplay.to_pb_block(blk))
        assert r["status"] == "processed" and r["transition"]
        transitions += 1
        i, has, cslot, lag = i + 1, True, blk.slot_number, 1
    assert transitions == 2 and stops == [64, 128]
    assert calls == [(0, 63, 0), (64, 1, 1), (65, 62, 0), (128, 1, 1), (129, 1, 0)]
    check_against(chain, cache, pool, ring)
    _, A, C = chain.candidate
    assert tuple(getattr(state, k) for k in state._SCALARS) == tuple(getattr(C, k) for k in state._SCALARS)
    assert [(r.dynasty, r.slot, bytes(r.blockhash)) for r in state.crosslink_records] == \
        [(r.dynasty, r.slot, bytes(r.blockhash)) for r in C.crosslink_records]
    np.testing.assert_array_equal(state.balances(), np.array([v.balance for v in C.validators], U64))
    check_states(pool, state, A.data, C)
    from prysm_amd import wire
    rest = (C.crosslinking_start_shard, bytes(C.dynasty_seed), C.dynasty_seed_last_reset)
    assert bc.resident_state_roots(pool, state, ring, wire.committees_device(table(C)), None, *rest) == \
        (ref.active_state_hash(A.data), ref.crystallized_state_hash(C))


# ---- 6: a panic row in the run ----------------------------------------------------------------------------------
def test_a_panic_row_leaves_cache_pool_and_ring():
    """A run whose third block carries a row that processAttestation refuses (slot above the block's)
    and calculateBlockVoteCache then panics on (slice bounds, core.go:353): ChainPanic, and the three objects equal a twin's that never
    saw the call."""
    nval = 1024
    blocks = late_chain(nval, 130, seed=4)[:8]
    chain, cache, pool, ring, tab, balance = genesis_objects(nval)
    _, twin_cache, twin_pool, twin_ring, _, _ = genesis_objects(nval)
    data, offs = bc.serialize_blocks(blocks[:3])
    for objs in ((cache, pool, ring), (twin_cache, twin_pool, twin_ring)):
        out = bc.walk_serialized_blocks(*objs, data, offs, 0, 0, tab, balance)
        assert out["ncand"] == 3
    good = blocks[5].attestations[-1]
    bad = pb.AttestationRecord(slot=blocks[5].slot_number + 70, shard_id=good.shard_id, justified_slot=good.justified_slot,
                               attester_bitfield=bytes(good.attester_bitfield),
                               oblique_parent_hashes=[bytes(h) for h in good.oblique_parent_hashes])
    blocks[5].attestations = [bad] + list(blocks[5].attestations)  # refused (slot too high), then re-derived: start > end
    for b in blocks[:5]:
        chain.process_block(oreplay.to_pb_block(b))
    with pytest.raises(ref.GoPanic):  # (CPU: the oracle panics at this block)
        chain.process_block(oreplay.to_pb_block(blocks[5]))
    data, offs = bc.serialize_blocks(blocks[3:8])
    with pytest.raises(bc.ChainPanic):
        bc.walk_serialized_blocks(cache, pool, ring, data, offs, 0, 0, tab, balance, has_candidate=True, candidate_slot=3)
    assert snapshot(cache) == snapshot(twin_cache) and cache.items()
    assert pool.records() == twin_pool.records() and len(pool)
    for a, b in zip(ring.read(history=True), twin_ring.read(history=True)):
        np.testing.assert_array_equal(a, b)
    # and the ring still works: the good blocks land as on the twin's side
    data, offs = bc.serialize_blocks(blocks[3:5])
    for objs in ((cache, pool, ring), (twin_cache, twin_pool, twin_ring)):
        bc.walk_serialized_blocks(*objs, data, offs, 0, 0, tab, balance, has_candidate=True, candidate_slot=3)
    assert ring.hashes() == twin_ring.hashes() and snapshot(cache) == snapshot(twin_cache)
