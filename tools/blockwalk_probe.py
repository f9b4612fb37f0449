"""Times a run of consecutive received blocks landing through ONE blockchain.walk_serialized_blocks
call (blockwalk.hip: each block against its own RecentBlockHashes, the ring resident on the device)
against the only exact form there was before it: one
blockchain.tally_serialized_blocks(tally_mixed=True, pending=) call PER BLOCK with the ring kept on
the host (the candidate rule of service.go:320-333 and Block.Hash, by hashlib, on the host too).
One process, the two paths alternating:

    run63     63 blocks of slots 1..63 of a 1,024-validator chain: every block the candidate
    run1024   1,024 blocks over the same 63 slots (16-17 siblings a slot): 63 candidates, the rest
              saved but not the candidate -- still one cycle, so the run needs no transition

Every block carries one attestation of a slot-0 committee with one oblique parent hash.  Each
repetition starts both paths from fresh genesis objects (made outside the timed region); after the
first repetition the two caches, pools and rings are compared, before any time is trusted.  Per
measurement: HIP events round the calls and a host clock round the calls plus a device synchronize,
3 warm-up rounds, then the median of REPS (default 20) with min and max.  The walk's three launches
(scan, rows, roll) get an event pair each through the A/B library's pz_debug_block_walk_timed over
the same decoded columns.  No bar is set.

    python tools/blockwalk_probe.py [--reps REPS] [--out DIR]   # DIR/probe.json, probe.txt"""
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
from prysm_amd import pb  # noqa: E402
from prysm_amd.pending import DevicePendingAttestations, DeviceRecentHashes  # noqa: E402
from prysm_amd.votes import DeviceVoteCache  # noqa: E402

NVAL = 1024
CAPS = [256, 256 * 32, 256 * 32, 256 * 8, 256, 256 * 32, 512]


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


def run_of(nblocks, tab, rng):
    blocks = []
    for j in range(nblocks):
        shard, comm = tab[0][j % len(tab[0])]
        bits = rng.random(len(comm)) < 0.3
        att = pb.AttestationRecord(slot=0, shard_id=shard, justified_slot=0, attester_bitfield=np.packbits(bits.astype(np.uint8)).tobytes(),
                                   shard_block_hash=rng.bytes(32), oblique_parent_hashes=[rng.bytes(32)])
        slot = 1 + j * 63 // nblocks
        blocks.append(pb.BeaconBlock(parent_hash=rng.bytes(32), slot_number=slot, timestamp=pb.Timestamp(8 * slot, 0), attestations=[att]))
    return blocks, bc.serialize_blocks(blocks)


def fresh(slots):
    return DeviceVoteCache(NVAL, slots), DevicePendingAttestations(CAPS)


def per_block(cache, pool, blocks, data, offs, tab, balance):
    """The parent commit's exact form: one call per block, the ring and the candidate on the host."""
    ring, has, cslot = [b""] * 128, False, 0
    for j, blk in enumerate(blocks):
        lo, hi = int(offs[j]), int(offs[j + 1])
        slot = blk.slot_number
        cand = not has or (slot > cslot and slot > 1)  # (every block of these runs goes on)
        report, _, _ = bc.tally_serialized_blocks(cache, data[lo:hi], np.array([0, hi - lo], np.uint64), 0, 0, 128, tab, ring, balance,
                                                  pending=pool, candidate=[int(cand)], tally_mixed=True)
        assert report[0] == bc.BLOCK_TALLIED
        if cand:
            ring = ([ref.bytes_to_hash(h) for h in ring] + [hashlib.blake2b(data[lo:hi].tobytes()).digest()[:32]])[-128:]
            has, cslot = True, slot
    return ring


def launches(data, offs, tab, nblocks):
    """ms of the walk's scan, rows and roll launches over the decoded run (A/B library)."""
    fn = _lib.lib.dll.pz_debug_block_walk_timed
    fn.argtypes, fn.restype = [_lib.vp, _lib.vp, _lib.vp, _lib.vp], ctypes.c_int
    payload = np.concatenate([data[:int(offs[-1])], np.zeros(4, np.uint8)])
    d = bc._split_decode_check(payload, offs, 0, 0, 128, tab, 0, want_committee=True)
    word, report, vote_status, pend_take, flags = bc._gate(d)
    dev, blk, natt = d["dev"], d["blk"], d["natt"]
    block_hash = torch.empty((nblocks, 32), dtype=torch.uint8, device=dev)
    _lib.lib.call("pz_dev_blake2b512_spans", d["d_bytes"].data_ptr(), d["d_offs"][:-1].data_ptr(), d["d_offs"][1:].data_ptr(), nblocks,
                  block_hash.data_ptr(), 32, _lib.stream_ptr(dev))
    walk = torch.empty(nblocks, dtype=torch.uint8, device=dev)
    base, result = torch.empty(nblocks, dtype=torch.int64, device=dev), torch.empty(4, dtype=torch.int64, device=dev)
    log = torch.empty(int(_lib.lib.dll.pz_block_walk_scratch_bytes(nblocks, natt)), dtype=torch.uint8, device=dev)
    p = _lib.dptr
    ms = (ctypes.c_float * 3)()
    out = []
    for _ in range(8):
        ring = DeviceRecentHashes()
        ps = d["parents_start"].clone()
        b = _lib.BlockWalkBatch(nblocks=nblocks, slot_number=p(blk["slot_number"]), report=p(report), block_hash=p(block_hash), natt=natt,
                                att_block=p(blk["att_block"]), vote_status=p(vote_status.clone()), pend_take=p(pend_take.clone()),
                                parents_start=p(ps), walk=p(walk), base=p(base), result=p(result), log=p(log), flags=p(flags))
        rc = fn(ring._h, ctypes.byref(b), _lib.stream_ptr(dev), ms)
        assert rc == 0, rc
        out.append(list(ms))
    assert int(result[1].item()) == 63
    return [stats([o[k] for o in out[3:]]) for k in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(23)
    _, cs = ref.new_genesis_states(NVAL)
    tab = [[(sc.shard_id, list(sc.committee)) for sc in arr.array_shard_and_committee] for arr in cs.shard_and_committees_for_slots]
    balance = np.array([v.balance for v in cs.validators], np.uint64)
    results = {"reps": args.reps, "validators": NVAL, "shapes": {}}
    lines = []
    f = lambda x: "%.3f (%.3f-%.3f)" % (x["median_ms"], x["min_ms"], x["max_ms"])  # noqa: E731

    for nblocks in (63, 1024):
        blocks, (data, offs) = run_of(nblocks, tab, rng)
        slots = 4096 if nblocks > 63 else 512
        t = {"walk": ([], []), "per_block": ([], [])}
        for rep in range(3 + args.reps):
            cache_w, pool_w = fresh(slots)
            ring_w = DeviceRecentHashes()
            cache_p, pool_p = fresh(slots)
            ev_w, host_w, out = timed(lambda: bc.walk_serialized_blocks(cache_w, pool_w, ring_w, data, offs, 0, 0, tab, balance))
            ev_p, host_p, ring_p = timed(lambda: per_block(cache_p, pool_p, blocks, data, offs, tab, balance))
            if rep == 0:  # both paths' objects, before any time is trusted
                assert out["stop"] == nblocks and out["ncand"] == 63
                assert cache_w.items() == cache_p.items() and len(cache_w.items()) > 32  # (the run's own hashes are keys)
                cw, cp = pool_w.columns(), pool_p.columns()
                assert all(np.array_equal(cw[k], cp[k]) for k in cw) and len(pool_w) == 63
                assert ring_w.hashes() == ring_p
            if rep >= 3:
                t["walk"][0].append(ev_w), t["walk"][1].append(host_w)
                t["per_block"][0].append(ev_p), t["per_block"][1].append(host_p)
        scan, rows, roll = launches(data, offs, tab, nblocks)
        row = {"blocks": nblocks, "candidates": 63, **{k: {"events": stats(v[0]), "host": stats(v[1])} for k, v in t.items()},
               "launches": {"scan": scan, "rows": rows, "roll": roll}}
        results["shapes"]["run%d" % nblocks] = row
        lines.append("run%-5d %d blocks, 63 candidates (caches, pools and rings of both paths equal)" % (nblocks, nblocks))
        lines.append("  one walk_serialized_blocks call     events %s ms   host clock %s ms" % (f(row["walk"]["events"]), f(row["walk"]["host"])))
        lines.append("  one tally call per block, host ring events %s ms   host clock %s ms"
                     % (f(row["per_block"]["events"]), f(row["per_block"]["host"])))
        lines.append("  the walk's launches: scan %s ms, rows %s ms, roll %s ms" % (f(scan), f(rows), f(roll)))
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
