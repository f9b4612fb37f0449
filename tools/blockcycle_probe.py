"""Times the 130-block chain of 1,024 validators (two cycle transitions, at slots 64 and 128) landing
through blockchain.ResidentChain.process_all (blockcycle.hip: three calls, one upload and one host
read each, stateRecalc between the two tallies of a call) against the only exact form there was
before it: blockchain.walk_serialized_blocks_saved cut before every transition block, the transition
block through six separate calls (saved.contains, tally_serialized_blocks, saved.insert,
state_recalc_resident, pend_serialized_blocks, ring.append), the block after it through a call of
its own with lag=1 -- and before every call the balances downloaded and the committee table
flattened again on the host, to be uploaded again.  One process, the two forms alternating, the one
that goes first changing every repetition; each repetition starts both from fresh genesis objects
(made outside the timed region); after the first repetition the outputs and the end states (cache,
pool, ring, saved set, scalars, crosslink records, balances) are compared, before any time is
trusted.  Per measurement: HIP events round the calls and a host clock round the calls plus a device
synchronize, 3 warm-up rounds, then the median of REPS (default 20) with min and max.  The three
launches of pz_dev_block_cycle (scan, rows, roll) get an event pair each through the A/B library's
pz_debug_block_cycle_timed over the decoded columns of the whole chain.  No bar is set.

    python tools/blockcycle_probe.py [--reps REPS] [--out DIR]   # DIR/probe.json, probe.txt"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prysm_amd import _lib  # noqa: E402

_lib.library_path = os.environ.get("PZ_PROBE_LIB") or os.path.join(ROOT, "build", "ab", "libprysm_hip.so")
from oracle import ref  # noqa: E402
from prysm_amd import blockchain as bc  # noqa: E402
from prysm_amd import synth, wire  # noqa: E402
from prysm_amd.pending import DevicePendingAttestations, DeviceRecentHashes, DeviceSavedBlocks, ResidentRecalcState  # noqa: E402
from prysm_amd.votes import DeviceVoteCache  # noqa: E402

NVAL, NBLOCKS = 1024, 130
CAPS = [256, 256 * 32, 256 * 32, 256 * 8, 256, 256 * 32, 512]
U64 = np.uint64


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def timed(fn):
    """(event ms, host ms, result) of fn() on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out


def chain_blocks(cs):
    """synth.chain_blocks with the attestations of the blocks of slots 96..127 moved to slot 65, so
    that the second stateRecalc both keeps and drops pending attestations; parents chained again
    (hashlib: input generation only)."""
    blocks = synth.chain_blocks(NVAL, NBLOCKS, seed=4)
    sc = cs.shard_and_committees_for_slots[1].array_shard_and_committee[0]
    rng = np.random.default_rng(5)
    parent = None
    for b in blocks:
        if parent is not None:
            b.parent_hash = parent
        if 96 <= b.slot_number < 128:
            k = len(sc.committee)
            bits = rng.random(8 * ((k + 7) // 8)) < 0.25
            bits[k:] = False
            a = b.attestations[0]
            a.slot, a.shard_id, a.attester_bitfield = 65, sc.shard_id, np.packbits(bits).tobytes()
        parent = hashlib.blake2b(wire.beacon_block(b), digest_size=64).digest()[:32]
    return blocks


def fresh(cs, tab):
    """Genesis objects: cache, pool, ring, saved set, state."""
    state = ResidentRecalcState(
        [v.balance for v in cs.validators], [v.start_dynasty for v in cs.validators], [v.end_dynasty for v in cs.validators],
        [v for arr in tab for e in arr for v in e[1]], bc._committee_table(tab)[3], cs.crosslink_records,
        last_state_recalc=cs.last_state_recalc, justified_streak=cs.justified_streak, last_justified_slot=cs.last_justified_slot,
        last_finalized_slot=cs.last_finalized_slot, current_dynasty=cs.current_dynasty, total_deposits=cs.total_deposits)
    return DeviceVoteCache(NVAL, 512), DevicePendingAttestations(CAPS), DeviceRecentHashes(), DeviceSavedBlocks(), state


def old_form(objs, blocks, data, offs, tab_of):
    """The parent commit's exact form: walk calls cut at ``stop``, the transition block through the six
    existing pieces in the reference's order, the block after it with lag=1 and the scalars, table and
    balances read before the transition.  ``tab_of()`` flattens the committee table again, as a
    caller holding a CrystallizedState does before every call."""
    cache, pool, ring, saved, state = objs
    n = len(blocks)

    def span(lo, hi):
        return data[int(offs[lo]):int(offs[hi])], (offs[lo:hi + 1] - offs[lo]).astype(U64)

    def scalars():
        return state.last_justified_slot, state.last_state_recalc, tab_of(), state.balances().copy()

    i, has, cslot, lag, pre, calls = 0, False, 0, 0, None, []
    while i < n:
        ljs, lsr, tab, balance = pre if lag else scalars()
        d, o = span(i, n)
        out = bc.walk_serialized_blocks_saved(cache, pool, ring, saved, d, o, ljs, lsr, tab, balance, has_candidate=has,
                                              candidate_slot=cslot, lag=lag)
        stop = out["stop"]
        calls.append((i, stop, lag))
        i, has, cslot = i + stop, out["has_candidate"], out["candidate_slot"]
        if lag:
            lag = 0
            continue
        if i == n:
            break
        blk = blocks[i]
        ljs, lsr, tab, balance = pre = scalars()
        assert list(saved.contains([ref.copy32(blk.parent_hash)])) == [True]
        d, o = span(i, i + 1)
        report, _, _ = bc.tally_serialized_blocks(cache, d, o, ljs, lsr, 128, tab, ring.read()[0], balance, tally_mixed=True)
        assert list(report) == [bc.BLOCK_TALLIED]
        saved.insert(out["block_hash"][stop:stop + 1])
        bc.state_recalc_resident(pool, cache, state, ring, blk.slot_number)
        bc.pend_serialized_blocks(pool, d, o, ljs, lsr, 128, tab, candidate=[1])
        ring.append(out["block_hash"][stop:stop + 1])
        i, has, cslot, lag = i + 1, True, blk.slot_number, 1
    return calls


def new_form(objs, tab, data, offs):
    rc = bc.ResidentChain(*objs, tab)  # (the table's device form is built here, once: inside the timed region)
    outs = rc.process_all(data, offs)
    return [(o["start"], o["stop"]) for o in outs], rc


def end_state(objs):
    cache, pool, ring, saved, state = objs
    r = state.read()
    return {"cache": cache.items(), "pool": {k: v.tolist() for k, v in pool.columns().items()}, "ring": ring.hashes(),
            "ring_len": ring.read(history=True)[1].tolist(), "saved": sorted(saved.hashes()),
            "state": {k: r[k].tolist() for k in ("scalars", "rec_dynasty", "rec_slot", "rec_hash", "rec_hash_len")},
            "balances": state.balances().tolist()}


def launches(tab, data, offs, reps):
    """ms of the cycle's scan, rows and roll launches over the decoded chain (A/B library): 3 warm-ups,
    then ``reps`` samples, as every other figure of the probe."""
    fn = _lib.lib.dll.pz_debug_block_cycle_timed
    fn.argtypes, fn.restype = [_lib.vp, _lib.vp, _lib.vp, _lib.vp], ctypes.c_int
    n = len(offs) - 1
    payload = np.concatenate([data[:int(offs[-1])], np.zeros(4, np.uint8)])
    d = bc._split_decode_check(payload, offs, 0, 0, 128, tab, 0, want_committee=True)
    _, report, vote_status, pend_take, flags = bc._gate(d)
    dev, blk, natt = d["dev"], d["blk"], d["natt"]
    block_hash = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    _lib.lib.call("pz_dev_blake2b512_spans", d["d_bytes"].data_ptr(), d["d_offs"][:-1].data_ptr(), d["d_offs"][1:].data_ptr(), n,
                  block_hash.data_ptr(), 32, _lib.stream_ptr(dev))
    walk = torch.empty(n, dtype=torch.uint8, device=dev)
    base, result = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(8, dtype=torch.int64, device=dev)
    log = torch.empty(int(_lib.lib.dll.pz_block_cycle_scratch_bytes(n, natt)), dtype=torch.uint8, device=dev)
    vote = torch.empty((2, natt), dtype=torch.int32, device=dev)
    take = torch.empty((2, natt), dtype=torch.uint8, device=dev)
    p = _lib.dptr
    ms = (ctypes.c_float * 3)()
    out = []
    for _ in range(3 + reps):
        ring = DeviceRecentHashes()
        ps = d["parents_start"].clone()
        b = _lib.BlockCycleBatch(nblocks=n, slot_number=p(blk["slot_number"]), report=p(report), block_hash=p(block_hash), natt=natt,
                                 att_block=p(blk["att_block"]), vote_status=p(vote_status), pend_take=p(pend_take), parents_start=p(ps),
                                 vote0=vote[0].data_ptr(), vote1=vote[1].data_ptr(), take0=take[0].data_ptr(),
                                 take1=take[1].data_ptr(), walk=p(walk), base=p(base), result=p(result), log=p(log), flags=p(flags))
        rc = fn(ring._h, ctypes.byref(b), _lib.stream_ptr(dev), ms)
        assert rc == 0, rc
        out.append(list(ms))
    assert [int(x) for x in result[:5].cpu()] == [65, 65, 1, 65, 63]  # stop, ncand, has, slot, T
    return [stats([o[k] for o in out[3:]]) for k in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _, cs = ref.new_genesis_states(NVAL)
    tab_of = lambda: [[(sc.shard_id, list(sc.committee)) for sc in arr.array_shard_and_committee]  # noqa: E731
                      for arr in cs.shard_and_committees_for_slots]
    tab = tab_of()
    blocks = chain_blocks(cs)
    data, offs = bc.serialize_blocks(blocks)
    t = {"resident_chain": ([], []), "walk_and_six_calls": ([], [])}
    shape = {}
    for rep in range(3 + args.reps):
        objs_n, objs_o = fresh(cs, tab), fresh(cs, tab)
        run_new = lambda: timed(lambda: new_form(objs_n, tab, data, offs))  # noqa: E731
        run_old = lambda: timed(lambda: old_form(objs_o, blocks, data, offs, tab_of))  # noqa: E731
        if rep % 2:
            (ev_o, host_o, calls_o), (ev_n, host_n, (calls_n, rc)) = run_old(), run_new()
        else:
            (ev_n, host_n, (calls_n, rc)), (ev_o, host_o, calls_o) = run_new(), run_old()
        if rep == 0:  # both forms' outputs and end states, before any time is trusted
            assert calls_n == [(0, 65), (65, 64), (129, 1)] and rc.calls == 3
            assert calls_o == [(0, 63, 0), (64, 1, 1), (65, 62, 0), (128, 1, 1), (129, 1, 0)]
            a, b = end_state(objs_n), end_state(objs_o)
            for k in a:
                assert a[k] == b[k], k
            assert len(a["cache"]) > 64 and len(a["saved"]) == NBLOCKS and a["state"]["scalars"][0] == 128
            shape = {"cache_entries": len(a["cache"]), "pool_rows": len(a["pool"]["slot"]), "saved": len(a["saved"])}
        if rep >= 3:
            t["resident_chain"][0].append(ev_n), t["resident_chain"][1].append(host_n)
            t["walk_and_six_calls"][0].append(ev_o), t["walk_and_six_calls"][1].append(host_o)
    scan, rows, roll = launches(tab, data, offs, args.reps)
    results = {"reps": args.reps, "validators": NVAL, "blocks": NBLOCKS, "end_state": shape,
               "calls": {"resident_chain": 3, "walk_and_six_calls": "5 walk calls + 2 x 6"},
               **{k: {"events": stats(v[0]), "host": stats(v[1])} for k, v in t.items()},
               "launches": {"scan": scan, "rows": rows, "roll": roll}}
    f = lambda x: "%.3f (%.3f-%.3f)" % (x["median_ms"], x["min_ms"], x["max_ms"])  # noqa: E731
    lines = ["chain130  %d blocks, %d validators, transitions at slots 64 and 128 (outputs and end states of both forms equal: "
             "%d cache entries, %d pool rows, %d saved hashes)" % (NBLOCKS, NVAL, shape["cache_entries"], shape["pool_rows"], shape["saved"]),
             "  ResidentChain.process_all, 3 calls           events %s ms   host clock %s ms"
             % (f(results["resident_chain"]["events"]), f(results["resident_chain"]["host"])),
             "  5 walk calls + 2 x the six-call transition   events %s ms   host clock %s ms"
             % (f(results["walk_and_six_calls"]["events"]), f(results["walk_and_six_calls"]["host"])),
             "  the cycle's launches over 130 blocks (medians of %d): scan %s ms, rows %s ms, roll %s ms"
             % (args.reps, f(scan), f(rows), f(roll))]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "probe.json"), "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")
        with open(os.path.join(args.out, "probe.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
