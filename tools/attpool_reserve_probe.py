"""Times the pending-attestation pool's growth (attpool.hip: pz_dev_att_pool_reserve, one launch of
pz_att_pool_move_kernel; pz_dev_att_pool_need, the need and scan launches) and the chain that needs
it.  No bar is set: the figures are reported.

    reserve  pools holding 128 and 4,096 rows at half their capacities -- (256, ...) and (8,192, ...),
             ResidentChain.CAPS scaled by the rows -- doubled by one reserve.  Every repetition starts
             from a fresh pool filled outside the timed region.  The launch gets one event pair (the
             A/B library's pz_debug_att_pool_reserve_timed), the whole product call one pair more.
             Beside them, in the same run: plain device-to-device copies of the same live bytes (as
             one copy, and as the sixteen columns' copies), and what a caller has to do without the
             call: columns() -- a download -- plus append_host into a larger pool -- an upload --
             on the host clock.
    need     pz_dev_att_pool_need over the same rows (one event pair per launch: the A/B library's
             pz_debug_att_pool_need_timed) beside the size and scan launches of the append of those
             rows (pz_debug_att_pool_timed).
    chain    synth.chain_blocks(1024, 330, seed=4) through ResidentChain.process_all, host clock round
             the call and a device synchronise, fresh genesis objects per repetition: the policies
             given with --chain as policy:rows (default grow:8 and fixed:256; the pool's other
             capacities scale with the rows).  The end states are compared after the first repetition.
             ``fixed`` uses nothing this file's tree added, so the same file times the parent commit's
             tree when it is run from there with --no-moves.

3 warm-up rounds, then the median of REPS (default 20) with min and max.  The first repetition of
every reserve checks the pool against its records before any time is trusted.

    python tools/attpool_reserve_probe.py [--reps REPS] [--chain POLICY:ROWS ...] [--no-moves] [--out DIR]"""
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
from oracle import ref  # noqa: E402
from prysm_amd import blockchain as bc  # noqa: E402
from prysm_amd import pb, synth, wire  # noqa: E402
from prysm_amd.pending import DevicePendingAttestations, DeviceRecentHashes, DeviceSavedBlocks, ResidentRecalcState  # noqa: E402
from prysm_amd.votes import DeviceVoteCache  # noqa: E402

CAPS = np.array([256, 256 * 32, 256 * 32, 256 * 8, 256, 256 * 32, 512], dtype=np.uint64)
WARM = 3


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def fmt(x):
    return "%.4f (%.4f-%.4f)" % (x["median_ms"], x["min_ms"], x["max_ms"])


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def records(rows, rng):
    """Rows as the synthetic chain's blocks carry them: two 32-byte hashes, 4 bitfield bytes, one oblique hash, two sig values."""
    return [pb.AttestationRecord(slot=int(rng.integers(1, 200)), shard_id=int(rng.integers(0, 1024)), justified_slot=1,
                                 justified_block_hash=rng.bytes(32), shard_block_hash=rng.bytes(32), attester_bitfield=rng.bytes(4),
                                 oblique_parent_hashes=[rng.bytes(32)], aggregate_sig=[1, 2]) for _ in range(rows)]


def timed(name, argtypes, *args, n):
    fn = getattr(_lib.lib.dll, name)
    fn.argtypes, fn.restype = argtypes, ctypes.c_int
    ms = (ctypes.c_float * n)()
    rc = fn(*args, ms)
    assert rc == 0, (name, rc, _lib.lib.dll.pz_last_error())
    return list(ms)


def reserve_at(rows, reps, rng):
    dev = torch.device("cuda", 0)
    vp, u64 = _lib.vp, _lib.u64
    recs = records(rows, rng)
    cols = wire.attestation_columns(recs)
    status, comm = np.zeros(rows, np.int32), np.arange(rows, dtype=np.uint32)
    caps = CAPS * np.uint64(max(rows // 128, 1))
    grown = caps * np.uint64(2)

    def fresh(c=caps):
        pool = DevicePendingAttestations(c)
        pool.append_host(cols, rows, status, comm)
        return pool

    n = fresh().counts()
    live = [int(x) for x in (8 * n[0], 8 * n[0], 8 * n[0], n[1], 8 * (n[0] + 1), n[2], 8 * (n[0] + 1), n[3], 8 * (n[0] + 1), n[5],
                             8 * (n[4] + 1), 8 * (n[0] + 1), 8 * n[6], 8 * (n[0] + 1), 4 * n[0], 4 * n[0])]
    out = {"rows": rows, "caps": caps.tolist(), "grown_to": grown.tolist(), "counts": n.tolist(), "live_bytes": sum(live)}
    launch, whole, today = [], [], []
    for rep in range(WARM + reps):
        p = fresh()
        ms = timed("pz_debug_att_pool_reserve_timed", [vp, vp, vp, vp], p._h, grown.ctypes.data, _lib.stream_ptr(0), n=1)
        if rep == 0:
            assert p.records() == recs and p.capacity().tolist() == grown.tolist()
        p2 = fresh()
        w = events(lambda: p2.reserve(grown, device_form=True))
        if rep == 0:
            assert p2.records() == recs

        p3 = fresh()

        def by_hand():  # what a caller does without the call: a download and an upload
            c = p3.columns()
            big = DevicePendingAttestations(grown)
            big.append_host(c, rows, status, c["committee"])
            return big

        t = host_clock(by_hand)
        if rep >= WARM:
            launch.append(ms[0]), whole.append(w), today.append(t)
        del p, p2, p3
    out["move_launch_events"], out["whole_call_events"], out["download_upload_host"] = stats(launch), stats(whole), stats(today)
    src = [torch.empty(max(b, 1), dtype=torch.uint8, device=dev).random_(0, 256) for b in live]
    dst = [torch.empty_like(s) for s in src]
    one_s = torch.empty(sum(live), dtype=torch.uint8, device=dev).random_(0, 256)
    one_d = torch.empty_like(one_s)
    out["copy_one"] = stats([events(lambda: one_d.copy_(one_s)) for _ in range(WARM + reps)][WARM:])
    out["copy_sixteen"] = stats([events(lambda: [d.copy_(s) for d, s in zip(dst, src)]) for _ in range(WARM + reps)][WARM:])
    # need beside the append's size and scan launches, on the same rows
    d = {k: bc._to_device(np.ascontiguousarray(v), dev) for k, v in cols.items()}
    c = _lib.att_cols(d)
    d_status, d_comm = bc._to_device(status, dev), bc._to_device(comm, dev)
    take = torch.ones((2, rows), dtype=torch.uint8, device=dev)
    need = torch.empty(14, dtype=torch.int64, device=dev)
    scr = torch.empty(max(int(_lib.lib.dll.pz_att_pool_need_scratch_bytes(rows)), int(_lib.lib.dll.pz_att_pool_scratch_bytes(rows))),
                      dtype=torch.uint8, device=dev)
    needs, sizes = [], []
    for rep in range(WARM + reps):
        ms = timed("pz_debug_att_pool_need_timed", [vp, u64, vp, vp, vp, vp, vp, vp, vp], ctypes.byref(c), rows, d_status.data_ptr(),
                   take[0].data_ptr(), take[1].data_ptr(), need.data_ptr(), scr.data_ptr(), _lib.stream_ptr(0), n=2)
        if rep == 0:
            assert need.cpu().numpy().view(np.uint64).reshape(2, 7).tolist() == [n.tolist()] * 2
        p = DevicePendingAttestations(grown)
        ap = timed("pz_debug_att_pool_timed", [vp, vp, u64, vp, vp, vp, u64, vp, vp, vp], p._h, ctypes.byref(c), rows,
                   d_status.data_ptr(), d_comm.data_ptr(), take[0].data_ptr(), 0, scr.data_ptr(), _lib.stream_ptr(0), n=4)
        if rep >= WARM:
            needs.append(ms), sizes.append(ap)
        del p
    out["need"] = {"need_launch": stats([m[0] for m in needs]), "scan_launch": stats([m[1] for m in needs]),
                   "sum": stats([m[0] + m[1] for m in needs])}
    out["append_size_scan"] = {"size_launch": stats([m[0] for m in sizes]), "scan_launch": stats([m[1] for m in sizes]),
                               "sum": stats([m[0] + m[1] for m in sizes])}
    return out


# ---- chain --------------------------------------------------------------------------------------------------------
def genesis(nval, rows, policy):
    _, cs = ref.new_genesis_states(nval)
    tab = [[(sc.shard_id, list(sc.committee)) for sc in arr.array_shard_and_committee] for arr in cs.shard_and_committees_for_slots]
    state = ResidentRecalcState(
        [v.balance for v in cs.validators], [v.start_dynasty for v in cs.validators], [v.end_dynasty for v in cs.validators],
        [v for arr in tab for e in arr for v in e[1]], bc._committee_table(tab)[3], cs.crosslink_records,
        last_state_recalc=cs.last_state_recalc, justified_streak=cs.justified_streak, last_justified_slot=cs.last_justified_slot,
        last_finalized_slot=cs.last_finalized_slot, current_dynasty=cs.current_dynasty, total_deposits=cs.total_deposits)
    kw = {} if policy == "fixed" else {"pool_policy": policy}  # (fixed: nothing this tree added)
    caps = (CAPS * np.uint64(rows) // np.uint64(256)).tolist()
    return bc.ResidentChain(DeviceVoteCache(nval, 2048), DevicePendingAttestations(caps), DeviceRecentHashes(), DeviceSavedBlocks(),
                            state, tab, **kw)


def chain_runs(specs, reps):
    nval = 1024
    data, offs = bc.serialize_blocks(synth.chain_blocks(nval, 330, seed=4))
    out, ends = {}, {}
    times = {s: [] for s in specs}
    for rep in range(WARM + reps):
        order = specs if rep % 2 == 0 else specs[::-1]  # neither always runs behind the other
        for spec in order:
            policy, rows = spec.split(":")
            rc = genesis(nval, int(rows), policy)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = rc.process_all(data, offs)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if rep == 0:
                s = rc.state
                ends[spec] = (rc.ring.hashes(), tuple(getattr(s, k) for k in s._SCALARS), s.balances().tobytes(), rc.pool.records(),
                              [(o["start"], o["stop"]) for o in outs])
                out[spec] = {"calls": rc.calls, "resubmits": rc.resubmits, "pool_rows": len(rc.pool),
                             "row_capacity": int(rc.pool.caps[0]), "grows": getattr(rc, "pool_grows", 0)}
            if rep >= WARM:
                times[spec].append(dt)
    assert all(e == ends[specs[0]] for e in ends.values()), "the policies' end states differ"
    for spec in specs:
        out[spec]["process_all_host"] = stats(times[spec])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chain", nargs="*", default=["grow:8", "fixed:256"])
    ap.add_argument("--no-moves", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(37)
    results, lines = {"reps": args.reps, "warmup": WARM}, []
    if not args.no_moves:
        results["reserve"] = [reserve_at(rows, args.reps, rng) for rows in (128, 4096)]
        for m in results["reserve"]:
            lines.append("%d live rows, %d live bytes, row capacity %d -> %d" % (m["rows"], m["live_bytes"], m["caps"][0], m["grown_to"][0]))
            lines.append("  reserve: move launch %s ms, whole call %s ms" % (fmt(m["move_launch_events"]), fmt(m["whole_call_events"])))
            lines.append("  plain copies of the live bytes: one copy %s ms, the sixteen columns' %s ms" % (fmt(m["copy_one"]), fmt(m["copy_sixteen"])))
            lines.append("  columns() + append_host into a larger pool (host clock): %s ms" % fmt(m["download_upload_host"]))
            lines.append("  need: %s ms (need %s, scan %s); the append's size + scan: %s ms (size %s, scan %s)"
                         % (fmt(m["need"]["sum"]), fmt(m["need"]["need_launch"]), fmt(m["need"]["scan_launch"]),
                            fmt(m["append_size_scan"]["sum"]), fmt(m["append_size_scan"]["size_launch"]),
                            fmt(m["append_size_scan"]["scan_launch"])))
    if args.chain:
        results["chain"] = chain_runs(list(args.chain), args.reps)
        for spec, r in results["chain"].items():
            lines.append("chain330 %-10s process_all host clock %s ms; %d calls, %d resubmits, %d rows in a row capacity of %d, %d grows"
                         % (spec, fmt(r["process_all_host"]), r["calls"], r["resubmits"], r["pool_rows"], r["row_capacity"], r["grows"]))
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
