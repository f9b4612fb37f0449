"""A run of blocks through a cycle transition on the GPU (prysm_amd/csrc/blockcycle.hip;
blockchain.ResidentChain):

1. the three launches of pz_[dev_]block_cycle on synthetic columns, device and host forms, against a
   block-by-block Python restatement of blockchain/service.go:320-363 (a pending candidate, a "not
   promoted yet" flag, a last_state_recalc that advances at the transition block, a list that only
   grows), with canary bytes behind every output and behind the log; and on runs without a transition
   block against the launches of pz_dev_block_walk on the same columns;
2. the 130-block chain through ResidentChain.process_all: three calls, cut at (0, 65), (65, 64) and
   (129, 1), against oracle.replay.Chain stepped block by block;
3. the same chain cut right after the transition block: lag 1 comes out, the next call takes it;
4. the rewarded chain of 8 validators: the lagged block tallies against the balances stateRecalc left;
5. a slot jump: the promoting block is a transition itself, deferred, and lands as T of the next call;
6. a panic row anywhere in the run leaves cache, pool, ring, set and state as a twin's;
7. five cycles whose blocks attest their own cycle, handed whole (in section 2), and a panic row past
   ``stop``: neither keeps the blocks before ``stop`` from landing."""
import copy
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
from test_attpool_gpu import as_pb, table
from test_blockparents_gpu import block_hash, chain130
from test_blockwalk_gpu import CANARY, CAPS, check_digests, padded, ring_of
from test_blockwalk_gpu import run_device as walk_device
from test_votecache_gpu import snapshot, want

pytestmark = pytest.mark.gpu

U64 = np.uint64
M64 = (1 << 64) - 1
NONE = M64
PROCESSED, NOT_PROCESSED = 0, 1
FAR = 1 << 40  # a lastStateRecalc no slot of the synthetic cases reaches
SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049]


# ---- 1: the launches on synthetic columns -------------------------------------------------------------------
def make(rng, n, go, slot_of, has0=0, cslot0=0, lsr=FAR, lag=0, panic=0):
    """A run of n blocks: go in {"all", "none", "alt", "random"}; 0-3 rows per block."""
    report = {"all": lambda j: 1 + j % 2, "none": lambda j: 0, "alt": lambda j: j % 2,
              "random": lambda j: int(rng.integers(0, 3))}[go]
    rows = rng.integers(0, 4, size=n)
    natt = int(rows.sum())
    ring, ring_len = rng.integers(0, 256, size=(129, 32), dtype=np.uint8), np.full(129, 32, np.uint8)
    if rng.integers(0, 2):  # a ring nothing was appended to yet: any stored lengths, no history
        ring[0], ring_len = 0, np.append(0, rng.integers(0, 33, size=128)).astype(np.uint8)
    return {"n": n, "ring": ring, "ring_len": ring_len, "has0": has0, "cslot0": cslot0, "lsr": lsr, "lag": lag, "panic": panic,
            "slot": np.array([slot_of(j) % (1 << 64) for j in range(n)], U64),
            "report": np.array([report(j) for j in range(n)], np.uint8), "hash": rng.integers(0, 256, size=(n, 32), dtype=np.uint8),
            "att_block": np.repeat(np.arange(n, dtype=np.uint32), rows), "parents_start": rng.integers(0, 65, size=natt).astype(U64),
            "pend_take": rng.integers(0, 2, size=natt).astype(np.uint8),
            "vote_status": rng.choice(np.array([0, 0, 0, 1, 4, 6], np.int32), size=natt)}


def model(r):
    """service.go:320-363 block by block over a list that only grows (core.go:223-237)."""
    n = r["n"]
    walk, base = np.full(n, 3, np.uint8), np.zeros(n, U64)
    hashes, lens = [h.tobytes() for h in r["ring"]], list(r["ring_len"])
    has, cslot = bool(r["has0"]), r["cslot0"] if r["has0"] else 0
    unpromoted, lsr = bool(r["lag"]), int(r["lsr"])  # the pending candidate's states are not the chain's yet
    ncand, stop, t, t_rank, t_slot = 0, n, None, 0, 0
    for j in range(n):
        slot = int(r["slot"][j])
        base[j] = len(hashes) - 128 - unpromoted  # the chain's RecentBlockHashes lacks the transition block's hash
        if not r["report"][j]:
            walk[j] = 0
            continue
        had = has
        if has and slot > cslot and slot > 1:  # updateHead: the candidate's states are promoted
            has = False
        if has:
            walk[j] = 1
            continue
        was_unpromoted = unpromoted
        if slot >= (lsr + 64) & M64:  # IsCycleTransition on the promoted state
            if t is not None:  # a second stateRecalc: the next call's
                has, stop, base[j] = had, j, 0
                break
            t, t_rank, t_slot, lsr, unpromoted = j, ncand, slot, (lsr + 64) & M64, True
        else:
            unpromoted = False
        hashes.append(r["hash"][j].tobytes())
        lens = [32] * (len(lens) + 1)  # RecentBlockHashes() is stored back whole, every entry 32 bytes
        has, cslot, ncand, walk[j] = True, slot, ncand + 1, 2
        if was_unpromoted:  # this block promoted a transition block's states: the run ends behind it
            stop = j + 1
            break
    log = np.zeros((129 + n, 32), np.uint8)
    log[:len(hashes)] = np.frombuffer(b"".join(hashes), np.uint8).reshape(-1, 32)
    b = r["att_block"].astype(np.int64)
    live = b < stop
    after = live & (b > t) if t is not None else np.zeros(len(b), bool)
    ps = r["parents_start"] + np.where(live, base[b] if n else 0, 0).astype(U64)
    off = np.where(r["vote_status"] == PROCESSED, NOT_PROCESSED, r["vote_status"]).astype(np.int32)
    cand = live & (r["pend_take"] != 0) & ((walk[b] == 2) if n else False)
    at_or_after = (b >= t) if t is not None else np.zeros(len(b), bool)
    rolled = 0 if r["panic"] else ncand
    return {"walk": walk, "base": base, "log": log,
            "result": np.array([stop, ncand, has, cslot, NONE if t is None else t, t_rank, t_slot, unpromoted], U64),
            "ring": log[rolled:rolled + 129].copy(), "ring_len": np.array(lens[-129:] if rolled else r["ring_len"], np.uint8),
            "parents_start": ps, "vote0": np.where(live & ~after, r["vote_status"], off).astype(np.int32),
            "vote1": np.where(after, r["vote_status"], off).astype(np.int32),
            "take0": (cand & ~at_or_after).astype(np.uint8), "take1": (cand & at_or_after).astype(np.uint8)}


OUT_DTYPES = {"walk": np.uint8, "base": U64, "result": U64, "log": np.uint8, "parents_start": U64, "vote0": np.int32, "vote1": np.int32,
              "take0": np.uint8, "take1": np.uint8}


def run_device(r):
    import torch

    n, natt = r["n"], len(r["att_block"])
    ring = ring_of(r["ring"], r["ring_len"])
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    ins = {k: put(r[k]) for k in ("slot", "report", "hash", "att_block", "vote_status", "pend_take")}
    flags = put(np.array([r["panic"]], np.uint32))
    outs = {"walk": padded(np.full(n, CANARY, np.uint8)), "base": padded(np.full(n, 0xA5A5, U64)),
            "result": padded(np.full(8, 0xA5A5, U64)), "log": padded(np.full((129 + n) * 32, CANARY, np.uint8)),
            "parents_start": padded(r["parents_start"]), "vote0": padded(np.full(natt, 0x5A5A, np.int32)),
            "vote1": padded(np.full(natt, 0x5A5A, np.int32)), "take0": padded(np.full(natt, CANARY, np.uint8)),
            "take1": padded(np.full(natt, CANARY, np.uint8))}
    assert outs["log"][1] == int(_lib.lib.dll.pz_block_cycle_scratch_bytes(n, natt))
    p = {k: (t.data_ptr() if used else None) for k, (t, used) in outs.items()}
    b = _lib.BlockCycleBatch(nblocks=n, slot_number=_lib.dptr(ins["slot"]), report=_lib.dptr(ins["report"]),
                             block_hash=_lib.dptr(ins["hash"]), has_candidate=r["has0"], candidate_slot=r["cslot0"],
                             last_state_recalc=r["lsr"], lag=r["lag"], natt=natt, att_block=_lib.dptr(ins["att_block"]),
                             vote_status=_lib.dptr(ins["vote_status"]), pend_take=_lib.dptr(ins["pend_take"]),
                             parents_start=p["parents_start"], vote0=p["vote0"], vote1=p["vote1"], take0=p["take0"], take1=p["take1"],
                             walk=p["walk"], base=p["base"], result=p["result"], log=outs["log"][0].data_ptr(), flags=flags.data_ptr())
    _lib.lib.call("pz_dev_block_cycle", ring._h, ctypes.byref(b), _lib.stream_ptr(0))
    torch.cuda.synchronize()
    got = {}
    for k, (t, used) in outs.items():
        host = t.cpu().numpy()
        assert (host[used:] == CANARY).all(), k  # nothing is written behind an output
        got[k] = host[:used].view(OUT_DTYPES[k])
    for k in ("vote_status", "pend_take"):  # the gate's columns are only read
        np.testing.assert_array_equal(ins[k].cpu().numpy(), np.ascontiguousarray(r[k]).view(np.uint8).reshape(-1), k)
    got["log"] = got["log"].reshape(-1, 32)
    got["ring"], got["ring_len"] = ring.read(history=True)
    return got


def run_host(r):
    n, natt = r["n"], len(r["att_block"])
    ring = ring_of(r["ring"], r["ring_len"])
    init = {"walk": np.full(n, CANARY, np.uint8), "base": np.full(n, 0xA5A5, U64), "result": np.full(8, 0xA5A5, U64),
            "log": np.full((129 + n, 32), CANARY, np.uint8), "parents_start": r["parents_start"],
            "vote0": np.full(natt, 0x5A5A, np.int32), "vote1": np.full(natt, 0x5A5A, np.int32),
            "take0": np.full(natt, CANARY, np.uint8), "take1": np.full(natt, CANARY, np.uint8)}
    whole, got = {}, {}
    for k, a in init.items():  # every output is the head of a host buffer with 64 canary bytes behind it
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        whole[k] = np.concatenate([raw, np.full(64, CANARY, np.uint8)])
        got[k] = whole[k][:raw.size].view(a.dtype).reshape(a.shape)
    hp = _lib.ptr
    flags = np.array([r["panic"]], np.uint32)
    b = _lib.BlockCycleBatch(nblocks=n, slot_number=hp(r["slot"]), report=hp(r["report"]), block_hash=hp(r["hash"]),
                             has_candidate=r["has0"], candidate_slot=r["cslot0"], last_state_recalc=r["lsr"], lag=r["lag"],
                             natt=natt, att_block=hp(r["att_block"]), vote_status=hp(r["vote_status"]), pend_take=hp(r["pend_take"]),
                             parents_start=hp(got["parents_start"]), vote0=hp(got["vote0"]), vote1=hp(got["vote1"]),
                             take0=hp(got["take0"]), take1=hp(got["take1"]), walk=hp(got["walk"]), base=hp(got["base"]),
                             result=got["result"].ctypes.data, log=got["log"].ctypes.data, flags=flags.ctypes.data)
    _lib.lib.call("pz_block_cycle", ring._h, ctypes.byref(b))
    for k, w in whole.items():
        assert (w[got[k].nbytes:] == CANARY).all(), k  # nothing is written behind an output
    got["ring"], got["ring_len"] = ring.read(history=True)
    return got


def runs_for(n, rng):
    """``(name, run, class)``: no T; T on both sides of every tile edge the size has, first, in the
    middle and last, with L plain, a transition, absent, behind siblings and closed blocks; lag 1 with
    L plain and a transition; slots 0 and 1; last_state_recalc near 2^64; a panic flag."""
    mk = lambda *a, **kw: make(rng, n, *a, **kw)  # noqa: E731
    up = lambda j: 2 + j  # noqa: E731
    out = [("all", mk("all", up)), ("none", mk("none", up, has0=1, cslot0=1)), ("alternating", mk("alt", up)),
           ("siblings", mk("all", lambda j: 7 + j // 2, has0=1, cslot0=3)), ("decreasing", mk("all", lambda j: 2 + n - j)),
           ("slots 0 and 1", mk("all", lambda j: j % 2)), ("slots 0 and 1, all transitions", mk("all", lambda j: j % 2, lsr=M64 - 63)),
           ("slots 1 and 0, carried, slot 1 a transition", mk("all", lambda j: (j + 1) % 2, has0=1, lsr=M64 - 62)),
           ("lag, nothing carried", mk("all", lambda j: 5 + j, lag=1)), ("lag, no candidate", mk("all", lambda j: 5, has0=1, cslot0=5, lag=1)),
           ("the sums wrap", mk("all", lambda j: M64 - 200 + j % 190, lsr=M64 - 150)),
           ("lag near 2^64", mk("random", lambda j: M64 - 130 + j % 131, has0=1, cslot0=3, lsr=M64 - 127, lag=1)),
           ("random", mk("random", lambda j: int(rng.integers(0, 200)), has0=int(rng.integers(0, 2)), cslot0=3, lsr=64)),
           ("random, lag", mk("random", lambda j: int(rng.integers(60, 200)), has0=1, cslot0=70, lsr=64, lag=1))]
    for at in sorted({0, n // 2, max(n - 1, 0), 1022, 1023, 1024, 2047, 2048}):
        if at >= n:
            continue
        pre = lambda j: 10 + j // 40  # noqa: E731
        out += [
            ("T at %d, then L" % at, mk("all", lambda j: pre(j) if j < at else 9064 + (j - at), has0=at % 2, cslot0=5, lsr=9000)),
            ("T at %d after candidates, L, a panic flag" % at,
             mk("alt", lambda j: 10 + j if j < at else 9064 + (j - at), lsr=9000, panic=1)),
            ("T at %d, siblings, L" % at, mk("all", lambda j: pre(j) if j < at else 9064 if j < at + 5 else 9065 + j, lsr=9000)),
            ("T at %d, lower slots and closed blocks, L" % at,
             mk("alt", lambda j: 10 if j < at else 9070 - (j - at) if j < at + 7 else 9071, has0=1, cslot0=5, lsr=9000)),
            ("T at %d, L a transition" % at, mk("all", lambda j: 10 + j if j < at else 9064 if j == at else 9128 + j, lsr=9000)),
            ("T at %d, siblings, L a transition" % at,
             mk("all", lambda j: pre(j) if j < at else 9064 if j < at + 3 else 9500 + j, has0=1, cslot0=5, lsr=9000)),
            ("T at %d, no L" % at, mk("all", lambda j: pre(j) if j < at else 9064, lsr=9000)),
            ("lag, L plain at %d" % at, mk("all", lambda j: 5 if j < at else 6 + j, has0=1, cslot0=5, lsr=64, lag=1)),
            ("lag, L a transition at %d" % at, mk("all", lambda j: 5 if j < at else 128 + j, has0=1, cslot0=5, lsr=64, lag=1)),
        ]
    return out


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("n", SIZES)
def test_launches_on_synthetic_columns(n, form):
    rng = np.random.default_rng(2000 + n)
    codes, kinds = set(), set()
    for name, r in runs_for(n, rng):
        want_ = model(r)
        got = (run_device if form == "device" else run_host)(r)
        if n == 0:  # nothing is launched: the outputs and the ring stay as they were
            np.testing.assert_array_equal(got["ring"], r["ring"], name)
            if form == "host":
                assert list(got["result"]) == [0, 0, r["has0"], r["cslot0"] if r["has0"] else 0, NONE, 0, 0, r["lag"]], name
            continue
        for k in ("result", "walk", "base", "log", "parents_start", "vote0", "vote1", "take0", "take1", "ring"):
            np.testing.assert_array_equal(got[k], want_[k], "%s: %s" % (name, k))
        np.testing.assert_array_equal(got["ring_len"], want_["ring_len"], name)
        codes |= set(want_["walk"].tolist())
        stop, _, _, _, t, _, _, lag_out = (int(x) for x in want_["result"])
        kinds.add(("T" if t != NONE else "no T", "lag" if r["lag"] else "no lag", "lag out" if lag_out else "no lag out",
                   "cut" if stop < n else "whole"))
        if t != NONE and (want_["vote1"] == PROCESSED).any():
            kinds.add("rows after T")
    if n >= 63:
        assert codes == {0, 1, 2, 3}
        assert {("T", "no lag", "no lag out", "cut"), ("T", "no lag", "lag out", "cut"), ("T", "no lag", "lag out", "whole"),
                ("no T", "no lag", "no lag out", "whole"), ("T", "lag", "lag out", "cut"), ("no T", "lag", "no lag out", "cut"),
                ("no T", "lag", "lag out", "whole"), "rows after T"} <= kinds


@pytest.mark.parametrize("lag", [0, 1])
@pytest.mark.parametrize("n", [65, 1025])
def test_a_run_without_a_transition_block_is_the_walks(n, lag):
    """Where no candidate reaches last_state_recalc + 64 the cycle's three launches give what the
    walk's give on the same columns: the walk's record, codes, bases, log and ring, phase 0 the
    walk's narrowed columns, phase 1 empty and no T -- past a wave's and a tile's edge, whole
    (lag 0) and stopped behind the first candidate (lag 1)."""
    rng = np.random.default_rng(3000 + 2 * n + lag)
    mk = lambda *a, **kw: make(rng, n, *a, lsr=FAR, lag=lag, **kw)  # noqa: E731
    stops = set()
    for name, r in [("all", mk("all", lambda j: 2 + j)), ("random", mk("random", lambda j: int(rng.integers(0, 90)), has0=1, cslot0=40)),
                    ("the first candidate in the last wave", mk("alt", lambda j: 5 if j < n - 2 else 6 + j, has0=1, cslot0=5))]:
        w, c = walk_device(r), run_device(r)
        np.testing.assert_array_equal(c["result"][:4], w["result"], name)
        assert int(c["result"][4]) == NONE, name
        for k in ("walk", "base", "log", "ring", "ring_len", "parents_start"):
            np.testing.assert_array_equal(c[k], w[k], "%s: %s" % (name, k))
        np.testing.assert_array_equal(c["vote0"], w["vote_status"], name)
        np.testing.assert_array_equal(c["take0"], w["pend_take"], name)
        np.testing.assert_array_equal(c["vote1"], np.where(r["vote_status"] == PROCESSED, NOT_PROCESSED, r["vote_status"]), name)
        assert not c["take1"].any(), name
        stops.add(int(w["result"][0]) < n)
    assert stops == ({True} if lag else {False})  # (lag 1: every run here has a candidate before its last block)


# ---- 2: the 130-block chain in three calls --------------------------------------------------------------------
def genesis_chain(nval, saved=None, slot_cap=512):
    """The oracle's chain at genesis and a ResidentChain over fresh resident objects."""
    from test_state_wire_gpu import genesis_resident

    chain = oreplay.Chain(nval)
    state, tab = genesis_resident(chain.C)
    rc = bc.ResidentChain(DeviceVoteCache(nval, slot_cap), DevicePendingAttestations(CAPS), DeviceRecentHashes(),
                          DeviceSavedBlocks(saved), state, tab)
    return chain, rc


def check_chain(chain, rc):
    """Cache with voters, pool, ring, saved set, scalars, crosslink records, balances and both state
    roots of ``rc`` against the oracle's candidate states."""
    _, A, C = chain.candidate
    state = rc.state
    assert snapshot(rc.cache) == want(A.cache)
    assert rc.pool.records() == [as_pb(a) for a in A.data.pending_attestations]
    assert rc.ring.hashes() == [bytes(h) for h in A.data.recent_block_hashes]
    assert set(rc.saved.hashes()) == chain.saved and rc.saved.count() == len(chain.saved)
    assert tuple(getattr(state, k) for k in state._SCALARS) == tuple(getattr(C, k) for k in state._SCALARS)
    assert [(r.dynasty, r.slot, bytes(r.blockhash)) for r in state.crosslink_records] == \
        [(r.dynasty, r.slot, bytes(r.blockhash)) for r in C.crosslink_records]
    np.testing.assert_array_equal(state.balances(), np.array([v.balance for v in C.validators], U64))
    rest = (C.crosslinking_start_shard, bytes(C.dynasty_seed), C.dynasty_seed_last_reset)
    assert bc.resident_state_roots(rc.pool, state, rc.ring, wire.committees_device(table(C)), None, *rest) == \
        (ref.active_state_hash(A.data), ref.crystallized_state_hash(C))
    # the host carry is the oracle's: the pending candidate, and whether its states are promoted
    assert rc.has_candidate and rc.candidate_slot == chain.candidate[0].slot_number
    assert rc.lag == int(C is not chain.C)
    assert rc.chain_scalars() == (chain.C.last_justified_slot, chain.C.last_state_recalc)


def check_outs(outs, recs, blocks):
    """Every block's status and every message digest of ``process_all``'s dicts against the oracle's records."""
    codes = {"processed": bc.WALK_CANDIDATE, "saved_not_candidate": bc.WALK_SAVED, "attestations_rejected": bc.WALK_OFF,
             "no_parent": bc.WALK_OFF}
    for out in outs:
        lo, stop = out["start"], out["stop"]
        part = recs[lo:lo + stop]
        assert [int(w) for w in out["walk"][:stop]] == [codes[r["status"]] for r in part]
        assert (out["walk"][stop:] == bc.WALK_DEFERRED).all()
        assert [bool(x) for x in out["parent_ok"][:stop]] == [r["status"] != "no_parent" for r in part]
        assert [h.tobytes() for h in out["block_hash"][:stop]] == [r["hash"] for r in part]
        trans = [j for j, r in enumerate(part) if r["transition"]]
        assert trans == ([] if out["t_index"] is None else [out["t_index"]])
        cut = dict(out, att_first=out["att_first"][:stop + 1])
        check_digests(cut, part)
        assert not out["msg"][int(out["att_first"][stop]):].any()  # a deferred block's rows have no digest yet


def test_the_130_block_chain_in_three_calls():
    """late_chain(1024, 130, seed=4) through process_all: three calls, one upload and one read each,
    where the walk takes five calls plus twice the six-call transition sequence."""
    nval = 1024
    blocks = chain130()
    data, offs = bc.serialize_blocks(blocks)
    chain, rc = genesis_chain(nval)
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks]
    assert [r["status"] for r in recs] == ["processed"] * 130 and [j for j, r in enumerate(recs) if r["transition"]] == [63, 127]
    outs = rc.process_all(data, offs, want_digests=True)
    assert [(o["start"], o["stop"]) for o in outs] == [(0, 65), (65, 64), (129, 1)] and rc.calls == 3
    assert [(o["t_index"], o["lag"], o["ncand"]) for o in outs] == [(63, 0, 65), (62, 0, 64), (None, 0, 1)]
    check_outs(outs, recs, blocks)
    check_chain(chain, rc)


def test_five_cycles_whose_blocks_attest_their_own_cycle():
    """synth.chain_blocks(1024, 330): transitions at slots 64 .. 320, the blocks of every cycle
    attesting that cycle's first slot.  Handed all the remaining bytes, a call checks blocks cycles
    ahead of its ``stop`` against scalars they are never processed under: under (0, 0) the rows of
    slot 256 name committee index 256 of a 256-slot table.  The oracle processes every block
    without a panic, and so must the device: such a row raises only in the call that processes its
    block."""
    from prysm_amd import synth

    nval = 1024
    blocks = synth.chain_blocks(nval, 330, seed=4)
    data, offs = bc.serialize_blocks(blocks)
    chain, rc = genesis_chain(nval)
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks]  # (CPU: no GoPanic)
    assert [r["status"] for r in recs] == ["processed"] * 330
    assert [blocks[j].slot_number for j, r in enumerate(recs) if r["transition"]] == [64, 128, 192, 256, 320]
    late = [a for b in blocks for a in b.attestations if a.slot >= 256]
    assert len(late) > 50 and chain.C.last_justified_slot == 0  # (CPU: rows that index past the table under lastStateRecalc 0)
    outs = rc.process_all(data, offs, want_digests=True)
    assert [(o["start"], o["stop"]) for o in outs] == [(0, 65), (65, 64), (129, 64), (193, 64), (257, 64), (321, 9)]
    assert rc.resubmits >= 1 and rc.calls == len(outs) + rc.resubmits  # a run submitted again without its deferred blocks
    check_outs(outs, recs, blocks)
    check_chain(chain, rc)


# ---- 3: the run cut right after T -------------------------------------------------------------------------------
def test_the_run_cut_right_after_the_transition_block():
    nval = 1024
    blocks = chain130()[:80]
    data, offs = bc.serialize_blocks(blocks)
    chain, rc = genesis_chain(nval)
    _, whole = genesis_chain(nval)
    whole.process_all(data, offs)
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks[:64]]
    d, o = bc.serialize_blocks(blocks[:64])
    out = rc.process_serialized(d, o, want_digests=True)
    assert (out["stop"], out["t_index"], out["lag"], out["ncand"]) == (64, 63, 1, 64) and rc.lag == 1
    check_outs([dict(out, start=0)], recs, blocks)
    check_chain(chain, rc)  # the chain's scalars are still the old ones, the candidate's a cycle on
    assert rc.chain_scalars()[1] == 0 and rc.state.last_state_recalc == 64
    recs += [chain.process_block(oreplay.to_pb_block(b)) for b in blocks[64:]]
    outs = rc.process_all(data[int(offs[64]):], offs[64:] - offs[64], want_digests=True)
    assert [(o["start"], o["stop"], o["lag"]) for o in outs] == [(0, 1, 0), (1, 15, 0)]
    for o_ in outs:
        o_["start"] += 64
    check_outs(outs, recs, blocks)
    check_chain(chain, rc)
    assert snapshot(rc.cache) == snapshot(whole.cache) and rc.pool.records() == whole.pool.records()
    for a, b in zip(rc.ring.read(history=True), whole.ring.read(history=True)):
        np.testing.assert_array_equal(a, b)
    assert set(rc.saved.hashes()) == set(whole.saved.hashes())
    np.testing.assert_array_equal(rc.state.read()["scalars"], whole.state.read()["scalars"])
    np.testing.assert_array_equal(rc.state.balances(), whole.state.balances())


# ---- 4: the rewarded chain ----------------------------------------------------------------------------------------
def rewarded_blocks(tab, root):
    """8 validators: one block at each slot 7, 15, ..., 63, 71, each attesting its own slot's one-member
    committee with bitfield 0x80 -- eight attesters, the whole deposit, so the transition at slot 71
    applies the rewards -- then the lagged block at slot 72, which attests slot 15: its window
    (start 57) reaches the first block's hash, which validator 1 has not voted for."""
    blocks, parent = [], root
    for slot, att_slot in [(s, s) for s in range(7, 72, 8)] + [(72, 15)]:
        shard, comm = tab[att_slot][0]
        assert len(comm) == 1
        a = pb.AttestationRecord(slot=att_slot, shard_id=shard, justified_slot=0, attester_bitfield=b"\x80")
        blocks.append(pb.BeaconBlock(parent_hash=parent, slot_number=slot, timestamp=pb.Timestamp(8 * slot, 0), attestations=[a]))
        parent = block_hash(blocks[-1])
    return blocks


def test_the_lagged_block_tallies_against_the_rewarded_balances():
    nval, root = 8, b"\x11" * 32
    chain, rc = genesis_chain(nval, saved=[root], slot_cap=64)
    chain.saved.add(root)
    blocks = rewarded_blocks(table(chain.C), root)
    # -- on the CPU, from the oracle alone --
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks[:-1]]  # (a GoPanic would raise here)
    assert [r["status"] for r in recs] == ["processed"] * 9 and [r["transition"] for r in recs] == [False] * 8 + [True]
    assert [v.balance for v in chain.C.validators] == [33, 31, 31, 31, 31, 31, 31, 31]  # the chain's state shows the new balances
    assert chain.C.last_state_recalc == 0 and chain.candidate[2].last_state_recalc == 64  # while its scalars are the old ones
    assert chain.candidate[2].total_deposits == 250
    stale = copy.deepcopy(chain)
    for v in stale.C.validators:
        v.balance = 32  # what a snapshot taken before the transition block would tally with
    last = oreplay.to_pb_block(blocks[-1])
    recs.append(chain.process_block(last))
    assert recs[-1]["status"] == "processed" and stale.process_block(last)["status"] == "processed"
    first = block_hash(blocks[0])
    o_cache, s_cache = chain.candidate[1].cache, stale.candidate[1].cache
    assert (list(o_cache[first][0]), o_cache[first][1], s_cache[first][1]) == ([1], 31, 32)  # only the in-place balances explain 31
    # -- on the device --
    data, offs = bc.serialize_blocks(blocks)
    outs = rc.process_all(data, offs, want_digests=True)
    assert [(o["start"], o["stop"], o["t_index"], o["lag"]) for o in outs] == [(0, 10, 8, 0)]
    assert rc.cache.total(first) == 31 and snapshot(rc.cache) == want(o_cache)
    check_outs(outs, recs, blocks)
    check_chain(chain, rc)


# ---- 5: a slot jump ---------------------------------------------------------------------------------------------------
def test_a_slot_jump_defers_the_second_transition_block():
    """Blocks of slots 1..64, then the chain's blocks of slots 128..130 chained behind them: the block
    that promotes the first transition block's states is a transition itself."""
    nval = 1024
    all_ = chain130()
    blocks = all_[:64] + all_[127:130]
    for k in (64, 65, 66):
        blocks[k].parent_hash = block_hash(blocks[k - 1])
    chain, rc = genesis_chain(nval)
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks]  # (CPU: the oracle takes the input without a panic)
    assert [r["status"] for r in recs] == ["processed"] * 67 and [j for j, r in enumerate(recs) if r["transition"]] == [63, 64]
    data, offs = bc.serialize_blocks(blocks)
    d, o = bc.serialize_blocks(blocks[:66])
    out = rc.process_serialized(d, o, want_digests=True)
    assert (out["stop"], out["t_index"], out["lag"], out["ncand"]) == (64, 63, 1, 64)  # L deferred
    assert list(out["walk"][64:]) == [bc.WALK_DEFERRED] * 2 and rc.chain_scalars()[1] == 0 and rc.state.last_state_recalc == 64
    outs = [dict(out, start=0)] + rc.process_all(data[int(offs[64]):], offs[64:] - offs[64], want_digests=True)
    # it lands as T with the lag kept; the block behind it promotes its states and ends its own run
    assert [(o_["start"], o_["stop"], o_["t_index"], o_["lag"]) for o_ in outs[1:]] == [(0, 1, 0, 1), (1, 1, None, 0), (2, 1, None, 0)]
    for o_ in outs[1:]:
        o_["start"] += 64
    check_outs(outs, recs, blocks)
    check_chain(chain, rc)
    assert rc.state.last_state_recalc == 128 and rc.calls == 4


# ---- 6: a panic row in the run ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def panic_blocks(at):
    """Blocks 0..69 of the chain with a row in block ``at`` that processAttestation refuses (slot above
    the block's) and calculateBlockVoteCache then panics on (slice bounds, core.go:353)."""
    blocks = chain130()[:70]
    good = blocks[at].attestations[-1]
    bad = pb.AttestationRecord(slot=blocks[at].slot_number + 70, shard_id=good.shard_id, justified_slot=good.justified_slot,
                               attester_bitfield=bytes(good.attester_bitfield),
                               oblique_parent_hashes=[bytes(h) for h in good.oblique_parent_hashes])
    blocks[at].attestations = [bad] + list(blocks[at].attestations)
    for k in range(at + 1, len(blocks)):
        blocks[k].parent_hash = block_hash(blocks[k - 1])
    return blocks


@pytest.mark.parametrize("at", [40, 63, 64])  # before T, in T, in the lagged block
def test_a_panic_row_leaves_every_object_as_a_twins(at):
    nval = 1024
    blocks = panic_blocks(at)
    chain, rc = genesis_chain(nval)
    _, twin = genesis_chain(nval)
    for b in blocks[:at]:
        chain.process_block(oreplay.to_pb_block(b))
    with pytest.raises(ref.GoPanic):  # (CPU: the oracle panics at this block)
        chain.process_block(oreplay.to_pb_block(blocks[at]))
    data, offs = bc.serialize_blocks(blocks[:3])
    for c in (rc, twin):
        assert c.process_serialized(data, offs)["ncand"] == 3
    data, offs = bc.serialize_blocks(blocks[3:])
    with pytest.raises(bc.ChainPanic):
        rc.process_serialized(data, offs)
    assert snapshot(rc.cache) == snapshot(twin.cache) and rc.cache.items()
    assert rc.pool.records() == twin.pool.records() and len(rc.pool)
    for a, b in zip(rc.ring.read(history=True), twin.ring.read(history=True)):
        np.testing.assert_array_equal(a, b)
    assert set(rc.saved.hashes()) == set(twin.saved.hashes()) and rc.saved.count() == 3
    for k in ("scalars", "rec_dynasty", "rec_slot", "rec_hash", "rec_hash_len"):
        np.testing.assert_array_equal(rc.state.read()[k], twin.state.read()[k], k)
    np.testing.assert_array_equal(rc.state.balances(), twin.state.balances())
    assert (rc.has_candidate, rc.candidate_slot, rc.lag, rc.chain_scalars()) == (True, 3, 0, (0, 0)) and not rc.spent
    # and the objects still work: the good blocks land as on the twin's side
    data, offs = bc.serialize_blocks(blocks[3:at])
    for c in (rc, twin):
        assert c.process_serialized(data, offs)["stop"] == at - 3
    assert rc.ring.hashes() == twin.ring.hashes() and snapshot(rc.cache) == snapshot(twin.cache)
    assert set(rc.saved.hashes()) == set(twin.saved.hashes()) and rc.saved.count() == at


def same_objects(rc, twin):
    assert snapshot(rc.cache) == snapshot(twin.cache) and rc.pool.records() == twin.pool.records()
    for a, b in zip(rc.ring.read(history=True), twin.ring.read(history=True)):
        np.testing.assert_array_equal(a, b)
    assert set(rc.saved.hashes()) == set(twin.saved.hashes()) and rc.saved.count() == twin.saved.count()
    for k in ("scalars", "rec_dynasty", "rec_slot", "rec_hash", "rec_hash_len"):
        np.testing.assert_array_equal(rc.state.read()[k], twin.state.read()[k], k)
    np.testing.assert_array_equal(rc.state.balances(), twin.state.balances())
    assert (rc.has_candidate, rc.candidate_slot, rc.lag, rc.chain_scalars()) == \
        (twin.has_candidate, twin.candidate_slot, twin.lag, twin.chain_scalars())


def test_a_panic_row_past_stop_waits_for_its_own_call():
    """The panic row sits in block 67 of 70 submitted at once; the run stops behind block 64.  The
    65 blocks before ``stop`` land as on a twin that was handed only them; the call that processes
    block 67 raises, and lands nothing."""
    nval = 1024
    blocks = panic_blocks(67)
    chain, rc = genesis_chain(nval)
    _, twin = genesis_chain(nval)
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks[:67]]
    with pytest.raises(ref.GoPanic):  # (CPU: the oracle panics at block 67, not before)
        chain.process_block(oreplay.to_pb_block(blocks[67]))
    data, offs = bc.serialize_blocks(blocks)
    out = rc.process_serialized(data, offs, want_digests=True)
    assert (out["stop"], out["t_index"], out["lag"], rc.resubmits, rc.calls) == (65, 63, 0, 1, 2)
    check_outs([dict(out, start=0)], recs[:65], blocks)
    d, o = bc.serialize_blocks(blocks[:65])
    assert twin.process_serialized(d, o)["stop"] == 65 and (twin.resubmits, twin.calls) == (0, 1)
    same_objects(rc, twin)
    d, o = data[int(offs[65]):], offs[65:] - offs[65]
    with pytest.raises(bc.ChainPanic):
        rc.process_serialized(d, o)
    same_objects(rc, twin)
    assert not rc.spent and rc.resubmits == 1  # (that run has no stop to cut at: the bit speaks of its own blocks)
    d, o = bc.serialize_blocks(blocks[65:67])
    for c in (rc, twin):
        assert c.process_serialized(d, o)["stop"] == 2
    same_objects(rc, twin)
