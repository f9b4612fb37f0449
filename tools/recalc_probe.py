"""Times the cycle transition over the resident pool and vote cache: blockchain.state_recalc_resident
(ONE ABI call, pz_dev_state_recalc) against blockchain.state_recalc_device (the composition of ABI
calls with host work between them it replaces), in the same process, alternating.

    65,536 validators with the committees of ShuffleIndices(Hash{'A'}), a pool of 4,096 pending rows
    (the committees' attestations round and round, the N-bit attestation last), vote caches of 128
    and of 8,192 slots, every slot filled.

Per cache size: a host clock around each call and the synchronise that ends it (the composition's
host work is the point), 3 warm-ups, then the median of REPS (default 20) with min and max; the
pool and both states are rebuilt, untimed, before every repetition.  Then the resident call's steps,
one event pair per step (fit, justify, epoch count, epoch finish, commit, prune), through the A/B
library's pz_debug_state_recalc_timed (build/ab/libprysm_hip.so, or PZ_PROBE_LIB).  Both paths'
results are compared at every repetition, so the probe is also a check at this size.

    python tools/recalc_probe.py [--reps REPS] [--out DIR]   # DIR/probe.json, probe.txt"""
import argparse
import ctypes
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
from prysm_amd import blockchain as bc  # noqa: E402
from prysm_amd import casper, pb, synth, wire  # noqa: E402
from prysm_amd.pending import DevicePendingAttestations, RecalcState, ResidentRecalcState  # noqa: E402
from prysm_amd.votes import DeviceVoteCache  # noqa: E402

NVAL, ROWS = 65536, 4096
STEPS = ("fit", "justify", "epoch_count", "epoch_finish", "commit", "prune")


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def instance(rng):
    shuffled = casper.shuffle_indices(b"A" + bytes(31), np.arange(NVAL, dtype=np.uint32))
    inst = synth.epoch_batch(NVAL, 1, seed=9, shuffled=shuffled)
    natt = int(inst["natt"])
    bo = inst["boffs"].astype(np.int64)
    pick = np.concatenate([np.arange(ROWS - 1) % (natt - 1), [natt - 1]])  # the N-bit attestation stays last
    recs = [pb.AttestationRecord(slot=int(inst["att_slot"][a]), shard_id=int(inst["att_shard"][a]), shard_block_hash=rng.bytes(32),
                                 attester_bitfield=inst["bits"][bo[a]:bo[a + 1]].tobytes()) for a in pick]
    return inst, recs, inst["att_comm"][pick].astype(np.uint32)


def fill_cache(cache, inst, slots, rng):
    """Fills every slot: calls of one attestation over 64 fresh recent hashes each."""
    nbytes = int(inst["boffs"][1] - inst["boffs"][0])
    cols = wire.attestation_columns([pb.AttestationRecord(slot=0, attester_bitfield=inst["bits"][:nbytes].tobytes())])
    status, comm, pstart = np.zeros(1, np.int32), np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    first = None
    for _ in range(slots // 64):
        recent = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
        first = recent if first is None else first
        cache.tally_host(cols, 1, status, comm, pstart, recent, inst["committee"], inst["coffs"], inst["balance"][0])
    assert len(cache.read()[1]) == slots
    return first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    dll = _lib.lib.dll
    dll.pz_debug_state_recalc_timed.argtypes = [_lib.vp] * 7
    dll.pz_debug_state_recalc_timed.restype = ctypes.c_int
    rng = np.random.default_rng(11)
    inst, recs, att_comm = instance(rng)
    cols = wire.attestation_columns(recs)
    sizes = [len(recs), 0, sum(len(r.shard_block_hash) for r in recs), sum(len(r.attester_bitfield) for r in recs), 0, 0, 0]
    caps = np.array(sizes, np.uint64) + np.uint64(64)
    records = [pb.CrosslinkRecord(0, bytes(32), 0) for _ in range(1024)]
    sargs = (inst["balance"][0], inst["start"][0], inst["end"][0], inst["committee"], inst["coffs"], records)
    skw = dict(last_state_recalc=31, justified_streak=2, last_justified_slot=40, last_finalized_slot=7,
               current_dynasty=int(inst["dynasty"][0]), total_deposits=int(inst["total_deposit"][0]))

    def fresh(kind):
        pool = DevicePendingAttestations(caps)
        pool.append_host(cols, len(recs), np.zeros(len(recs), np.int32), att_comm)
        return pool, kind(*sargs, **skw)

    results = {"reps": args.reps, "nval": NVAL, "rows": ROWS, "caches": {}}
    lines = []
    f = lambda x: "%.4f (%.4f-%.4f)" % (x["median_ms"], x["min_ms"], x["max_ms"])  # noqa: E731
    for slots in (128, 8192):
        cache = DeviceVoteCache(NVAL, slots)
        recent = fill_cache(cache, inst, slots, rng)  # the loop's 64 hashes all have an entry
        t_dev, t_res, launches = [], [], []
        for rep in range(3 + args.reps):
            pool_d, model = fresh(RecalcState)
            pool_r, state = fresh(ResidentRecalcState)
            td, w0 = wall(lambda: bc.state_recalc_device(pool_d, cache, model, recent, 1234))
            tr, w1 = wall(lambda: bc.state_recalc_resident(pool_r, cache, state, recent, 1234))
            got = state.read()
            assert np.array_equal(w0, w1) and np.array_equal(state.balances(), model.balances())
            assert tuple(int(x) for x in got["scalars"][:6]) == (model.last_state_recalc, model.justified_streak,
                                                                 model.last_justified_slot, model.last_finalized_slot,
                                                                 model.current_dynasty, model.total_deposits)
            assert pool_d.records() == pool_r.records() if rep == 0 else True
            # the steps, through the timed entry, on a fresh pool and state
            pool_t, st_t = fresh(ResidentRecalcState)
            d_recent = torch.from_numpy(np.ascontiguousarray(recent)).to(dev)
            b = _lib.RecalcBatch(nval=NVAL, balance=st_t.balance.data_ptr(), start=st_t.start.data_ptr(), end=st_t.end.data_ptr(),
                                 members=st_t.members.data_ptr(), coffs=st_t.coffs.data_ptr(), recent=d_recent.data_ptr(),
                                 n_recent=64, block_slot=1234)
            scratch = torch.empty(int(dll.pz_state_recalc_scratch_bytes(NVAL, int(caps[0]), 1024)), dtype=torch.uint8, device=dev)
            ms = (ctypes.c_float * 6)()
            rc = dll.pz_debug_state_recalc_timed(st_t._h, pool_t._h, cache._h, ctypes.byref(b), scratch.data_ptr(),
                                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), ms)
            assert rc == 0, dll.pz_last_error()
            if rep >= 3:
                t_dev.append(td)
                t_res.append(tr)
                launches.append(list(ms))
        la = np.array(launches)
        row = {"slots": slots, "composition": stats(t_dev), "resident": stats(t_res),
               "steps": {k: stats(la[:, j]) for j, k in enumerate(STEPS)}}
        row["ratio"] = row["resident"]["median_ms"] / row["composition"]["median_ms"]
        results["caches"][str(slots)] = row
        lines.append("cache of %d slots, %d validators, %d pending rows (results equal)" % (slots, NVAL, ROWS))
        lines.append("  state_recalc_device (composition) %s ms  state_recalc_resident (one call) %s ms  ratio %.2f"
                     % (f(row["composition"]), f(row["resident"]), row["ratio"]))
        lines.append("  steps  " + "  ".join("%s %s" % (k, f(v)) for k, v in row["steps"].items()))
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
