"""Times the block gate (blockgate.hip: one launch, pz_dev_block_gate through
blockchain.gate_blocks) against the torch composition it replaces (blockchain._open_blocks twice,
the report arithmetic and the two gathered takes, as tally_serialized_blocks and _pend form them),
in one process, the two alternating:

    gate64 / gate4096    batches of 64 and 4,096 blocks of 8 attestations (1,024 validators, the
                         genesis committees, 128 recent hashes; every eighth block's last
                         attestation fails, so it is rejected; no block is mixed)
    tally64 / tally4096  blockchain.tally_serialized_blocks over the same bytes with and without
                         tally_mixed: the whole call (upload, split, decode, checks, gate or
                         composition, tally, the reads), i.e. the cost of the gate's extra host read

Per measurement: HIP events round the calls and a host clock round the calls plus a device
synchronize, 3 warm-up rounds, then the median of REPS (default 20) with min and max.  The gate's
report and pend_take are compared with the composition's, so the probe is also a check at these
sizes.  No bar is set: at these sizes the gate is expected to be a launch floor.

    python tools/blockgate_probe.py [--reps REPS] [--out DIR]   # DIR/probe.json, probe.txt"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref  # noqa: E402
from prysm_amd import blockchain as bc  # noqa: E402
from prysm_amd import pb  # noqa: E402
from prysm_amd.votes import DeviceVoteCache  # noqa: E402

NVAL, ATTS = 1024, 8


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def timed(fn):
    """(event ms, host ms) of fn() on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out


def batch(nblocks, tab, rng):
    def rec(slot, good=True):
        shard, comm = tab[slot][0]
        bits = rng.random(len(comm)) < 0.6
        return pb.AttestationRecord(slot=slot, shard_id=shard, justified_slot=0 if good else 9,
                                    attester_bitfield=np.packbits(bits.astype(np.uint8)).tobytes())

    blocks = []
    for b in range(nblocks):
        atts = [rec(1 + (b + k) % 9, good=not (k == ATTS - 1 and b % 8 == 7)) for k in range(ATTS)]
        blocks.append(pb.BeaconBlock(parent_hash=rng.bytes(32), slot_number=10, timestamp=pb.Timestamp(80, 0), attestations=atts))
    return bc.serialize_blocks(blocks)


def composition(d, cand):
    """What tally_serialized_blocks (default) and _pend compute of the decoded batch."""
    open_, att_block, count, nproc = bc._open_blocks(d)
    report = open_.long() * (bc.BLOCK_TALLIED + (bc.BLOCK_MIXED - bc.BLOCK_TALLIED) * (nproc != count).long())
    take = (report == bc.BLOCK_TALLIED)[att_block].to(torch.uint8)
    open_c = bc._open_blocks(d, cand)[0]
    pend = (open_c[att_block] & (d["status"] == bc.ATT_PROCESSED)).to(torch.uint8)
    return report, take, pend


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(21)
    _, cs = ref.new_genesis_states(NVAL)
    tab = [[(sc.shard_id, list(sc.committee)) for sc in arr.array_shard_and_committee] for arr in cs.shard_and_committees_for_slots]
    recent = [rng.bytes(32) for _ in range(128)]
    balance = np.array([v.balance for v in cs.validators], np.uint64)
    results = {"reps": args.reps, "validators": NVAL, "attestations_per_block": ATTS, "shapes": {}}
    lines = []
    f = lambda x: "%.4f (%.4f-%.4f)" % (x["median_ms"], x["min_ms"], x["max_ms"])  # noqa: E731

    for nblocks in (64, 4096):
        data, offs = batch(nblocks, tab, rng)
        cand = (rng.random(nblocks) < 0.9).astype(np.uint8)
        d = bc._split_decode_check(data, offs, 0, 0, 128, tab, 0, want_committee=True)
        t = {"gate": ([], []), "composition": ([], [])}
        for rep in range(3 + args.reps):
            ev_g, host_g, (report, vote_status, pend_take, flags) = timed(lambda: bc.gate_blocks(d, cand))
            ev_c, host_c, (report_c, take_c, pend_c) = timed(lambda: composition(d, cand))
            if rep >= 3:
                t["gate"][0].append(ev_g), t["gate"][1].append(host_g)
                t["composition"][0].append(ev_c), t["composition"][1].append(host_c)
        assert not int(flags.item()) and torch.equal(report.long(), report_c) and torch.equal(pend_take, pend_c)
        assert torch.equal((vote_status == bc.ATT_PROCESSED).to(torch.uint8), take_c)  # (no mixed block here)
        row = {"blocks": nblocks, "rows": d["natt"], "rejected": int((report == 0).sum().item()),
               **{k: {"events": stats(v[0]), "host": stats(v[1])} for k, v in t.items()}}
        results["shapes"]["gate%d" % nblocks] = row
        lines.append("gate%-5d %d blocks, %d rows (%d blocks rejected; report, vote_status and pend_take equal)"
                     % (nblocks, nblocks, d["natt"], row["rejected"]))
        for k in ("gate", "composition"):
            lines.append("  %-12s events %s ms   host clock %s ms" % (k, f(row[k]["events"]), f(row[k]["host"])))

        caches = {False: DeviceVoteCache(NVAL, 512), True: DeviceVoteCache(NVAL, 512)}
        t = {False: ([], []), True: ([], [])}
        for rep in range(3 + args.reps):
            for mixed in (False, True):
                ev, host, out = timed(lambda: bc.tally_serialized_blocks(caches[mixed], data, offs, 0, 0, 128, tab, recent, balance,
                                                                         tally_mixed=mixed))
                if rep >= 3:
                    t[mixed][0].append(ev), t[mixed][1].append(host)
        assert caches[False].items() == caches[True].items() and caches[True].items()
        row = {"blocks": nblocks, "rows": d["natt"],
               "default": {"events": stats(t[False][0]), "host": stats(t[False][1])},
               "tally_mixed": {"events": stats(t[True][0]), "host": stats(t[True][1])}}
        results["shapes"]["tally%d" % nblocks] = row
        lines.append("tally%-4d tally_serialized_blocks over the same bytes (caches equal)" % nblocks)
        for k in ("default", "tally_mixed"):
            lines.append("  %-12s events %s ms   host clock %s ms" % (k, f(row[k]["events"]), f(row[k]["host"])))
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
