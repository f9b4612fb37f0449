"""Times the stored CrystallizedState from the device-resident objects (prysm_amd/csrc/wire_state.hip),
by tools/recalc_probe.py's method: same process, alternating, 3 warm-ups, then the median of REPS
(default 20) with min and max.

    65,536 and 1,048,576 validators with the engine's table shape: 64 slots of committees of 128,
    the table held twice (128 arrays), so every validator is in two entries; 1,024 crosslink records.

(a) A host clock around pz_crystallized_state_read (ResidentRecalcState.wire with field 12 already
    encoded on the device: the table changes only at a dynasty transition) against the composition it
    replaces: pz_recalc_state_read, the three column downloads and wire.crystallized_state in Python
    -- whole, and without field 12 (as if the caller had cached those bytes too).  The two messages
    are compared at every repetition, so the probe is also a check at these sizes.
(b) One event pair each round the field 12 encode (pz_dev_wire_committees) and the head + validators +
    tail chain (pz_dev_crystallized_state_bytes), beside a device-to-device copy of the same number
    of bytes as the floor.  Ratios are reported, not judged.

    python tools/state_wire_probe.py [--reps REPS] [--sizes N,N] [--out DIR]   # DIR/probe.json, probe.txt"""
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
from prysm_amd import _lib, pb, wire  # noqa: E402
from prysm_amd.pending import ResidentRecalcState  # noqa: E402

COMMITTEE, SLOTS, NREC = 128, 64, 1024


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def timed(fn):
    """fn on the current stream between one event pair; milliseconds."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def instance(nval, rng):
    ncomm = nval // COMMITTEE
    members = rng.permutation(nval).astype(np.uint32)
    coffs = (np.arange(ncomm + 1, dtype=np.uint64) * np.uint64(COMMITTEE))
    per = ncomm // SLOTS
    table = {"arr_offs": np.arange(2 * SLOTS + 1, dtype=np.uint64) * np.uint64(per),
             "arr_shard": (np.arange(2 * ncomm, dtype=np.uint64) % np.uint64(1024)),
             "arr_comm": np.concatenate([np.arange(ncomm), np.arange(ncomm)]).astype(np.uint32), "coffs": coffs, "members": members}
    balance = rng.integers(16, 1 << 36, size=nval, dtype=np.uint64)
    start = np.zeros(nval, np.uint64)
    end = np.full(nval, 9999999999999999999, np.uint64)
    records = [pb.CrosslinkRecord(int(s % 3), rng.bytes(32) if s % 2 else b"", int(64 * (s % 5))) for s in range(NREC)]
    state = ResidentRecalcState(balance, start, end, members, coffs, records, last_state_recalc=128, justified_streak=2,
                                last_justified_slot=64, last_finalized_slot=0, current_dynasty=1, total_deposits=int(balance.sum() & ((1 << 64) - 1)))
    arrays = [pb.ShardAndCommitteeArray([pb.ShardAndCommittee(int(table["arr_shard"][e]), members[int(coffs[c]):int(coffs[c + 1])])
                                         for e, c in [(a * per + j, int(table["arr_comm"][a * per + j])) for j in range(per)]])
              for a in range(2 * SLOTS)]
    return table, state, arrays


def composition(state, arrays):
    """What a caller of the parent commit does: the handle's download, the three columns', wire.py."""
    r = state.read()
    s = [int(x) for x in r["scalars"][:6]]
    recs = [pb.CrosslinkRecord(int(r["rec_dynasty"][i]), r["rec_hash"][i, :int(r["rec_hash_len"][i])].tobytes(), int(r["rec_slot"][i]))
            for i in range(state.nrec)]
    vals = pb.Validators(state.nval, balance=state.balances(), start_dynasty=state.start.cpu().numpy().view(np.uint64),
                         end_dynasty=state.end.cpu().numpy().view(np.uint64))
    return wire.crystallized_state(pb.CrystallizedState(s[0], s[1], s[2], s[3], s[4], 0, s[5], b"", 0, recs, vals, arrays))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    dll = _lib.lib.dll
    sh = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731
    f = lambda x: "%.4f (%.4f-%.4f)" % (x["median_ms"], x["min_ms"], x["max_ms"])  # noqa: E731
    results = {"reps": args.reps, "sizes": {}}
    lines = []
    for nval in (int(x) for x in args.sizes.split(",")):
        rng = np.random.default_rng(nval)
        table, state, arrays = instance(nval, rng)
        from prysm_amd.blockchain import _to_device
        d_table = {k: _to_device(v, dev) for k, v in table.items()}
        nent, ncap = len(table["arr_comm"]), 2 * nval
        t = wire._table_struct(d_table, _lib.dptr)
        out12 = torch.empty(int(dll.pz_wire_committees_bound(t.narr, nent, ncap)), dtype=torch.uint8, device=dev)
        scr12 = torch.empty(int(dll.pz_wire_committees_scratch_bytes(t.narr, nent, ncap)), dtype=torch.uint8, device=dev)
        res12 = torch.zeros(2, dtype=torch.int64, device=dev)

        def encode12():
            _lib.lib.call("pz_dev_wire_committees", ctypes.byref(t), nent, ncap, 12, out12.data_ptr(), res12.data_ptr(), scr12.data_ptr(), sh())

        encode12()
        n12, status = (int(x) for x in res12.cpu())
        assert status == 0
        f12 = out12[:n12]
        rest, cols = _lib.CstateRest(), state.validator_cols()
        outcs = torch.empty(int(dll.pz_crystallized_state_bound(NREC, 32, nval, 0, n12)), dtype=torch.uint8, device=dev)
        scrcs = torch.empty(int(dll.pz_crystallized_state_scratch_bytes(nval)), dtype=torch.uint8, device=dev)
        span = torch.zeros(2, dtype=torch.int64, device=dev)

        def chain():
            _lib.lib.call("pz_dev_crystallized_state_bytes", state._h, ctypes.byref(rest), ctypes.byref(cols), nval, f12.data_ptr(), n12,
                          outcs.data_ptr(), span.data_ptr(), scrcs.data_ptr(), sh())

        chain()
        ncs = int(span.cpu()[1])
        # the floors: whole tensors of exactly the byte counts (a copy of a slice is an elementwise kernel, not a device copy)
        src, dst = torch.zeros(ncs, dtype=torch.uint8, device=dev), torch.zeros(ncs, dtype=torch.uint8, device=dev)
        src12, dst12 = torch.zeros(n12, dtype=torch.uint8, device=dev), torch.zeros(n12, dtype=torch.uint8, device=dev)
        t_read, t_comp, t_comp_no12, e12, ecs, ecopy12, ecopycs = ([] for _ in range(7))
        for rep in range(3 + args.reps):
            tr, got = wall(lambda: state.wire(f12))
            tc, want = wall(lambda: composition(state, arrays))
            tn, _ = wall(lambda: composition(state, []))
            assert got == want and len(got) == ncs
            row = (timed(encode12), timed(chain), timed(lambda: dst12.copy_(src12)), timed(lambda: dst.copy_(src)))
            if rep >= 3:
                for lst, v in zip((t_read, t_comp, t_comp_no12, e12, ecs, ecopy12, ecopycs), (tr, tc, tn) + row):
                    lst.append(v)
        r = {"nval": nval, "field12_bytes": n12, "message_bytes": ncs, "read": stats(t_read), "composition": stats(t_comp),
             "composition_without_field12": stats(t_comp_no12), "field12_encode": stats(e12), "field12_copy": stats(ecopy12),
             "state_chain": stats(ecs), "state_copy": stats(ecopycs)}
        r["ratio_read_to_composition"] = r["read"]["median_ms"] / r["composition"]["median_ms"]
        r["ratio_read_to_composition_without_field12"] = r["read"]["median_ms"] / r["composition_without_field12"]["median_ms"]
        r["ratio_field12_to_copy"] = r["field12_encode"]["median_ms"] / r["field12_copy"]["median_ms"]
        r["ratio_chain_to_copy"] = r["state_chain"]["median_ms"] / r["state_copy"]["median_ms"]
        results["sizes"][str(nval)] = r
        lines.append("%d validators: field 12 %d bytes, message %d bytes (messages equal)" % (nval, n12, ncs))
        lines.append("  (a) pz_crystallized_state_read %s ms  composition %s ms (ratio %.3f)  composition without field 12 %s ms (ratio %.3f)"
                     % (f(r["read"]), f(r["composition"]), r["ratio_read_to_composition"], f(r["composition_without_field12"]),
                        r["ratio_read_to_composition_without_field12"]))
        lines.append("  (b) field 12 encode %s ms  copy of %d bytes %s ms (ratio %.1f)" % (f(r["field12_encode"]), n12, f(r["field12_copy"]),
                                                                                           r["ratio_field12_to_copy"]))
        lines.append("      head + validators + tail %s ms  copy of %d bytes %s ms (ratio %.1f)" % (f(r["state_chain"]), ncs, f(r["state_copy"]),
                                                                                                    r["ratio_chain_to_copy"]))
        print("\n".join(lines[-4:]), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "probe.json"), "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")
        with open(os.path.join(args.out, "probe.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
