"""Times a run of consecutive received blocks landing through ONE
blockchain.walk_serialized_blocks_saved call (blockparents.hip: the saved-block set resident on the
device, the parent check of service.go:261-269 resolved there by pointer jumping) against the only
exact form there was before it: the host building ``eligible`` -- Block.Hash by hashlib per block and
a Python set, in block order -- and then the same walk with the mask
(blockchain.walk_serialized_blocks).  One process, the two forms alternating, the one that goes first
changing every repetition:

    run63     63 blocks of slots 1..63 of a 1,024-validator chain, each block's parent the block
              before it: a dependency chain as long as the run
    run1024   1,024 blocks chained the same way over the same 63 slots (16-17 a slot)

Every block carries one attestation of a slot-0 committee with one oblique parent hash, and every
block is open, which the host form relies on (a host that did not know the gate's answers would
have to decode and check first).  Each repetition starts both forms from fresh genesis objects (made
outside the timed region); after the first repetition the two forms' outputs, caches, pools and rings
are compared and the device set is compared with the host's, before any time is trusted.  Per
measurement: HIP events round the call and a host clock round the call plus a device synchronize, 3
warm-up rounds, then the median of REPS (default 20) with min and max.  The four new launches (open,
link, resolve; the insert after the walk) get an event pair each through the A/B library's
pz_debug_block_parents_timed / pz_debug_block_set_insert_walked_timed over the same decoded columns.
No bar is set.

    python tools/blockparents_probe.py [--reps REPS] [--out DIR]   # DIR/probe.json, probe.txt"""
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
from prysm_amd import pb, wire  # noqa: E402
from prysm_amd.pending import DevicePendingAttestations, DeviceRecentHashes, DeviceSavedBlocks  # noqa: E402
from prysm_amd.votes import DeviceVoteCache  # noqa: E402

NVAL = 1024
CAPS = [2048, 2048 * 32, 2048 * 32, 2048 * 8, 2048, 2048 * 32, 4096]


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
    blocks, parent = [], rng.bytes(32)
    for j in range(nblocks):
        shard, comm = tab[0][j % len(tab[0])]
        bits = rng.random(len(comm)) < 0.3
        att = pb.AttestationRecord(slot=0, shard_id=shard, justified_slot=0, attester_bitfield=np.packbits(bits.astype(np.uint8)).tobytes(),
                                   shard_block_hash=rng.bytes(32), oblique_parent_hashes=[rng.bytes(32)])
        slot = 1 + j * 63 // nblocks
        blocks.append(pb.BeaconBlock(parent_hash=parent, slot_number=slot, timestamp=pb.Timestamp(8 * slot, 0), attestations=[att]))
        parent = hashlib.blake2b(wire.beacon_block(blocks[-1]), digest_size=64).digest()[:32]
    return blocks, bc.serialize_blocks(blocks)


def fresh(slots):
    return DeviceVoteCache(NVAL, slots), DevicePendingAttestations(CAPS), DeviceRecentHashes()


def host_mask(blocks, data, offs, db):
    """service.go:261-269 + :324 on the host, in order: every block of these runs is open."""
    eligible = np.zeros(len(blocks), np.uint8)
    for j, blk in enumerate(blocks):
        if blk.slot_number <= 1 or bytes(blk.parent_hash) in db:
            eligible[j] = 1
            db.add(hashlib.blake2b(data[int(offs[j]):int(offs[j + 1])].tobytes(), digest_size=64).digest()[:32])
    return eligible


def launches(data, offs, tab, nblocks):
    """ms of the open, link and resolve launches and of the insert after the walk (A/B library)."""
    dll = _lib.lib.dll
    parents_timed, insert_timed = dll.pz_debug_block_parents_timed, dll.pz_debug_block_set_insert_walked_timed
    parents_timed.argtypes, parents_timed.restype = [_lib.vp] * 5, ctypes.c_int
    insert_timed.argtypes, insert_timed.restype = [_lib.vp, _lib.vp, _lib.vp, _lib.vp, _lib.u64, _lib.vp, _lib.vp, _lib.vp], ctypes.c_int
    payload = np.concatenate([data[:int(offs[-1])], np.zeros(4, np.uint8)])
    d = bc._split_decode_check(payload, offs, 0, 0, 128, tab, 0, want_committee=True)
    dev, blk, natt = d["dev"], d["blk"], d["natt"]
    sh, p = _lib.stream_ptr(dev), _lib.dptr
    block_hash = torch.empty((nblocks, 32), dtype=torch.uint8, device=dev)
    _lib.lib.call("pz_dev_blake2b512_spans", d["d_bytes"].data_ptr(), d["d_offs"][:-1].data_ptr(), d["d_offs"][1:].data_ptr(), nblocks,
                  block_hash.data_ptr(), 32, sh)
    ok, saved0 = torch.empty(nblocks, dtype=torch.uint8, device=dev), torch.empty(nblocks, dtype=torch.uint8, device=dev)
    status_out = torch.empty(nblocks, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(dll.pz_block_parents_scratch_bytes(nblocks)), dtype=torch.uint8, device=dev)
    status = d["status"].contiguous()
    b = _lib.BlockParentsBatch(nblocks=nblocks, bytes=p(d["d_bytes"]), nbytes=int(offs[-1]), bytes_beg=p(blk["bytes_beg"]),
                               bytes_len=p(blk["bytes_len"]), slot_number=p(blk["slot_number"]), block_hash=p(block_hash),
                               att_first=p(blk["att_first"]), block_status=p(blk["status"]), rec_status=p(d["rec"]),
                               att_status=p(status), natt=natt, parent_ok=p(ok), saved0=p(saved0), block_status_out=p(status_out))
    walk = torch.full((nblocks,), bc.WALK_CANDIDATE, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    ms3, ms1 = (ctypes.c_float * 3)(), (ctypes.c_float * 1)()
    out = []
    for _ in range(8):
        saved = DeviceSavedBlocks(min_keys=2 * nblocks)
        rc = parents_timed(saved._h, ctypes.byref(b), p(scratch), sh, ms3)
        assert rc == 0, rc
        rc = insert_timed(saved._h, p(block_hash), p(walk), None, nblocks, p(count), sh, ms1)
        assert rc == 0, rc
        out.append(list(ms3) + list(ms1))
    assert bool(saved0.all().item()) and int(count.item()) == nblocks
    return [stats([o[k] for o in out[3:]]) for k in range(4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(29)
    _, cs = ref.new_genesis_states(NVAL)
    tab = [[(sc.shard_id, list(sc.committee)) for sc in arr.array_shard_and_committee] for arr in cs.shard_and_committees_for_slots]
    balance = np.array([v.balance for v in cs.validators], np.uint64)
    results = {"reps": args.reps, "validators": NVAL, "shapes": {}}
    lines = []
    f = lambda x: "%.3f (%.3f-%.3f)" % (x["median_ms"], x["min_ms"], x["max_ms"])  # noqa: E731

    for nblocks in (63, 1024):
        blocks, (data, offs) = run_of(nblocks, tab, rng)
        slots = 4096 if nblocks > 63 else 512
        t = {"device_set": ([], []), "host_mask": ([], []), "host_mask_only": ([], [])}
        for rep in range(3 + args.reps):
            cache_d, pool_d, ring_d = fresh(slots)
            saved = DeviceSavedBlocks()
            cache_h, pool_h, ring_h = fresh(slots)
            db = set()

            def host_form():
                t0 = time.perf_counter()
                eligible = host_mask(blocks, data, offs, db)
                t["_mask_ms"] = (time.perf_counter() - t0) * 1e3
                return bc.walk_serialized_blocks(cache_h, pool_h, ring_h, data, offs, 0, 0, tab, balance, eligible=eligible)

            device_form = lambda: bc.walk_serialized_blocks_saved(cache_d, pool_d, ring_d, saved, data, offs, 0, 0, tab, balance)  # noqa: E731
            if rep % 2:  # the forms swap places every repetition: neither always runs behind the other
                ev_h, host_h, out_h = timed(host_form)
                ev_d, host_d, out_d = timed(device_form)
            else:
                ev_d, host_d, out_d = timed(device_form)
                ev_h, host_h, out_h = timed(host_form)
            if rep == 0:  # both forms' outputs and objects, before any time is trusted
                assert out_d["stop"] == nblocks and out_d["ncand"] == 63 and out_d["parent_ok"].all()
                for k, v in out_h.items():
                    assert np.array_equal(np.asarray(out_d[k]), np.asarray(v)), k
                assert cache_d.items() == cache_h.items() and len(cache_d.items()) > 32
                cd, ch = pool_d.columns(), pool_h.columns()
                assert all(np.array_equal(cd[k], ch[k]) for k in cd) and len(pool_d) == 63
                assert ring_d.hashes() == ring_h.hashes()
                assert set(saved.hashes()) == db and len(db) == nblocks
            if rep >= 3:
                t["device_set"][0].append(ev_d), t["device_set"][1].append(host_d)
                t["host_mask"][0].append(ev_h), t["host_mask"][1].append(host_h)
                t["host_mask_only"][1].append(t["_mask_ms"])
        names = ("open", "link", "resolve", "insert_walked")
        row = {"blocks": nblocks, "candidates": 63,
               "device_set": {"events": stats(t["device_set"][0]), "host": stats(t["device_set"][1])},
               "host_mask": {"events": stats(t["host_mask"][0]), "host": stats(t["host_mask"][1]),
                             "mask_alone_host": stats(t["host_mask_only"][1])},
               "launches": dict(zip(names, launches(data, offs, tab, nblocks)))}
        results["shapes"]["run%d" % nblocks] = row
        lines.append("run%-5d %d blocks in one chain, 63 candidates (outputs, caches, pools, rings and sets of both forms equal)" % (nblocks, nblocks))
        lines.append("  walk_serialized_blocks_saved (device set)   events %s ms   host clock %s ms"
                     % (f(row["device_set"]["events"]), f(row["device_set"]["host"])))
        lines.append("  host mask + walk_serialized_blocks          events %s ms   host clock %s ms   (the mask alone: %s ms)"
                     % (f(row["host_mask"]["events"]), f(row["host_mask"]["host"]), f(row["host_mask"]["mask_alone_host"])))
        lines.append("  the new launches: " + ", ".join("%s %s ms" % (k, f(v)) for k, v in row["launches"].items()))
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
