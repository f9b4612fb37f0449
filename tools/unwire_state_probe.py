"""Times the load of a stored CrystallizedState into the resident columns on the device
(unwire_state.hip) at 65,536 and 1,048,576 validators with full records (113 bytes framed: five
10-byte varints, a 20-byte address, a 32-byte commitment) and 64 committee arrays, against two host
yardsticks on the same box:

  (a) unwire_state_dev.h's frame_host alone on the same bytes, one core (the A/B library's
      pz_debug_cstate_frame_host): the sequential walk the framing kernels replace;
  (b) the path a node has today: pz_chain_new_from_state (chain.hip's host parse and its uploads),
      and oracle.schema's parse plus the ResidentRecalcState list constructor (at 65,536 only: a
      million Python objects take minutes); the faster of the two counts.

The device load is timed as a whole (host clock round upload, head, frame, the read, the allocations,
decode and its status read) and per call with HIP events: the upload, pz_dev_cstate_frame (its nine
launches), pz_dev_cstate_decode (its seven); the launches get an event pair each through the A/B
library's pz_debug_cstate_frame_timed / _decode_timed (the one-lane launches paired with their
neighbour), and a sweep from 16,384 to 524,288 validators shows where the frame call crosses (a).
Before any time is trusted the loaded columns are
compared with the ones the bytes were built from.  Medians of REPS (default 10) after 2 warm-ups.
No bar is set.

    python tools/unwire_state_probe.py [--reps REPS] [--out DIR]   # DIR/probe.json, probe.txt"""
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
from prysm_amd import pb, wire  # noqa: E402
from prysm_amd.pending import ResidentRecalcState  # noqa: E402

U64 = np.uint64
SIZES = (65536, 1048576)
SWEEP = (16384, 131072, 262144, 524288)
FRAME_LAUNCHES = ("frame: tile", "frame: group", "frame: chain + entries", "frame: size", "frame: scan", "frame: terms + arrays",
                  "frame: result")
DECODE_LAUNCHES = ("decode: begin + validators", "decode: arrays", "decode: member count", "decode: member scan",
                   "decode: member write", "decode: end")


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def full_state(n, seed=1):
    """The bytes of a state of n full records, built with numpy, and the columns they hold."""
    rng = np.random.default_rng(seed)
    cols = {k: rng.integers(1 << 63, (1 << 64) - 1, size=n, dtype=U64, endpoint=True)
            for k in ("public_key", "withdrawal_shard", "balance", "start_dynasty", "end_dynasty")}
    addr, comm = rng.integers(0, 256, size=(n, 20), dtype=np.uint8), rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    rec = np.zeros((n, 113), np.uint8)
    rec[:, 0], rec[:, 1] = 0x5a, 111
    at = 2

    def varint(key, x):
        nonlocal at
        rec[:, at] = key
        for k in range(9):
            rec[:, at + 1 + k] = ((x >> U64(7 * k)) & U64(0x7f)).astype(np.uint8) | 0x80
        rec[:, at + 10] = 1
        at += 11

    def blob(key, b):
        nonlocal at
        rec[:, at], rec[:, at + 1] = key, b.shape[1]
        rec[:, at + 2:at + 2 + b.shape[1]] = b
        at += 2 + b.shape[1]

    varint(0x08, cols["public_key"]), varint(0x10, cols["withdrawal_shard"])
    blob(0x1a, addr), blob(0x22, comm)
    varint(0x28, cols["balance"]), varint(0x30, cols["start_dynasty"]), varint(0x38, cols["end_dynasty"])
    assert at == 113
    members = rng.permutation(n).astype(np.uint32).reshape(64, -1)
    arrays = [pb.ShardAndCommitteeArray([pb.ShardAndCommittee(a + 1, members[a])]) for a in range(64)]
    head = wire.crystallized_state(pb.CrystallizedState(64, 1, 2, 3, 1, 5, 1 << 40, b"\x07" * 32, 9,
                                                        [pb.CrosslinkRecord(1, bytes([i % 256]) * 32, i) for i in range(1024)]))
    f12 = b"".join(wire._msg(12, wire.shard_and_committee_array(a)) for a in arrays)
    cols.update(withdrawal_address=addr.reshape(-1), randao_commitment=comm.reshape(-1), members=members.reshape(-1))
    return head + rec.tobytes() + f12, cols


def device_load(raw, reps):
    """The load's calls with an event pair each; returns the per-call and whole statistics."""
    dev = torch.device("cuda", 0)
    buf = np.frombuffer(raw, np.uint8)
    dll, sh = _lib.lib.dll, _lib.stream_ptr(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    rows = {"upload": [], "frame": [], "read_and_allocate": [], "decode": [], "whole_host": []}
    for rep in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        head = wire.cstate_head(buf)
        d = wire._upload(buf, dev)
        scr = torch.empty(int(dll.pz_cstate_scratch_bytes(buf.size)), dtype=torch.uint8, device=dev)
        result = torch.empty(_lib.CSF_COUNT, dtype=torch.int64, device=dev)
        ev[1].record()
        _lib.lib.call("pz_dev_cstate_frame", d.data_ptr(), buf.size, head["body_beg"], scr.data_ptr(), result.data_ptr(), sh)
        ev[2].record()
        r = [int(x) for x in result.cpu()]
        assert r[_lib.CSF_STATUS] == 0, r
        size = {k: r[_lib.CSF_NVAL] for k in wire.VALIDATOR_COLS}
        size.update(withdrawal_address=r[_lib.CSF_ADDRESS_BYTES], randao_commitment=r[_lib.CSF_COMMITMENT_BYTES],
                    withdrawal_address_offs=r[_lib.CSF_NVAL] + 1, randao_commitment_offs=r[_lib.CSF_NVAL] + 1,
                    arr_offs=r[_lib.CSF_NARR] + 1, arr_shard=r[_lib.CSF_NENTRIES], arr_comm=r[_lib.CSF_NENTRIES],
                    coffs=r[_lib.CSF_NENTRIES] + 1, members=r[_lib.CSF_NMEMBERS])
        kind = {"withdrawal_address": torch.uint8, "randao_commitment": torch.uint8, "arr_comm": torch.int32, "members": torch.int32}
        cols = {k: torch.empty(max(size[k], 1), dtype=kind.get(k, torch.int64), device=dev) for k in wire.VALIDATOR_COLS + wire.TABLE_COLS}
        v = _lib.ValidatorColsOut(*[cols[k].data_ptr() for k in wire.VALIDATOR_COLS])
        t = _lib.CommitteeTableOut(narr=r[_lib.CSF_NARR], ncomm=r[_lib.CSF_NENTRIES], **{k: cols[k].data_ptr() for k in wire.TABLE_COLS})
        status = torch.empty(2, dtype=torch.int64, device=dev)
        ev[3].record()
        _lib.lib.call("pz_dev_cstate_decode", d.data_ptr(), buf.size, scr.data_ptr(), ctypes.byref(v), ctypes.byref(t),
                      status.data_ptr(), sh)
        ev[4].record()
        assert status.cpu().tolist() == [0, 0]
        whole = (time.perf_counter() - t0) * 1e3
        if rep >= 2:
            for k, name in enumerate(("upload", "frame", "read_and_allocate", "decode")):
                rows[name].append(ev[k].elapsed_time(ev[k + 1]))
            rows["whole_host"].append(whole)
    # the launches one event pair each (the A/B library's timed entries), over the last repetition's buffers
    fms, dms = (ctypes.c_float * 7)(), (ctypes.c_float * 6)()
    per = {name: [] for name in FRAME_LAUNCHES + DECODE_LAUNCHES}
    for rep in range(reps + 2):
        _lib.lib.call("pz_debug_cstate_frame_timed", d.data_ptr(), buf.size, head["body_beg"], scr.data_ptr(), result.data_ptr(), sh, fms)
        _lib.lib.call("pz_debug_cstate_decode_timed", d.data_ptr(), buf.size, scr.data_ptr(), ctypes.byref(v), ctypes.byref(t),
                      status.data_ptr(), sh, dms)
        assert status.cpu().tolist() == [0, 0]
        if rep >= 2:
            for name, ms in zip(FRAME_LAUNCHES + DECODE_LAUNCHES, list(fms) + list(dms)):
                per[name].append(ms)
    out = {k: stats(v) for k, v in rows.items()}
    out["launches"] = {k: stats(v) for k, v in per.items()}
    return out, int(scr.numel())


def host_clock(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unwire_state"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dll = _lib.lib.dll
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    dll.pz_debug_cstate_frame_host.argtypes = [vp, u64, u64, vp]
    dll.pz_debug_cstate_frame_timed.argtypes = [vp, u64, u64, vp, vp, vp, vp]
    dll.pz_debug_cstate_decode_timed.argtypes = [vp, u64, vp, vp, vp, vp, vp, vp]
    report, lines = {"reps": args.reps, "sizes": {}}, []
    for n in SIZES:
        raw, cols = full_state(n)
        buf = np.frombuffer(raw, np.uint8)
        got = wire.unwire_crystallized_state(raw)  # compared before any time is trusted
        assert got["nval"] == n and got["narr"] == 64
        for k, want in cols.items():
            np.testing.assert_array_equal(got[k], want, k)
        body = wire.cstate_head(buf)["body_beg"]
        out = np.zeros(6, U64)

        def frame_host():
            assert dll.pz_debug_cstate_frame_host(buf.ctypes.data, buf.size, body, out.ctypes.data) == 0 and int(out[2]) == n

        row = {"bytes": len(raw)}
        row["device"], row["scratch_bytes"] = device_load(raw, args.reps)
        row["resident_from_state_host"] = host_clock(lambda: ResidentRecalcState.from_state(raw), args.reps)
        row["a_frame_host"] = host_clock(frame_host, args.reps)
        row["b_chain_new_from_state"] = host_clock(lambda: bc.BeaconChain.from_state(raw), max(args.reps // 3, 2))
        if n <= 65536:
            from oracle import schema

            def lists():
                cs = schema.CrystallizedState()
                cs.ParseFromString(raw)
                vs = cs.validators
                tab = [[(e.shard_id, list(e.committee)) for e in a.array_shard_and_committee] for a in cs.shard_and_committees_for_slots]
                ResidentRecalcState([v.balance for v in vs], [v.start_dynasty for v in vs], [v.end_dynasty for v in vs],
                                    bc._members(tab), bc._committee_table(tab)[3], cs.crosslink_records,
                                    last_state_recalc=cs.last_state_recalc, total_deposits=cs.total_deposits)
                torch.cuda.synchronize()

            row["b_schema_parse_and_lists"] = host_clock(lists, max(args.reps // 3, 2))
        report["sizes"][str(n)] = row
        d = row["device"]
        lines.append("%9d validators, %11d bytes, scratch %10d (%.3f x len)" % (n, len(raw), row["scratch_bytes"], row["scratch_bytes"] / len(raw)))
        lines.append("  device: upload %.3f  frame %.3f  read+allocate %.3f  decode %.3f ms (events); whole %.3f ms (host clock)" % (
            d["upload"]["median_ms"], d["frame"]["median_ms"], d["read_and_allocate"]["median_ms"], d["decode"]["median_ms"],
            d["whole_host"]["median_ms"]))
        lines.append("  launches (us): " + ", ".join("%s %.0f" % (k, 1e3 * x["median_ms"])
                                                    for k, x in d["launches"].items()))
        lines.append("  ResidentRecalcState.from_state %.3f ms;  (a) frame_host %.3f ms;  (b) pz_chain_new_from_state %.3f ms%s" % (
            row["resident_from_state_host"]["median_ms"], row["a_frame_host"]["median_ms"], row["b_chain_new_from_state"]["median_ms"],
            ";  schema parse + lists %.3f ms" % row["b_schema_parse_and_lists"]["median_ms"] if "b_schema_parse_and_lists" in row else ""))
    # where the frame call (framing, the records' sizes and field 12) crosses frame_host (framing alone)
    report["crossover"] = {}
    for n in SWEEP:
        raw, _ = full_state(n)
        buf = np.frombuffer(raw, np.uint8)
        body = wire.cstate_head(buf)["body_beg"]
        out = np.zeros(6, U64)
        dev = device_load(raw, args.reps)[0]
        host = host_clock(lambda: dll.pz_debug_cstate_frame_host(buf.ctypes.data, buf.size, body, out.ctypes.data), args.reps)
        assert int(out[2]) == n
        report["crossover"][str(n)] = {"frame": dev["frame"], "a_frame_host": host}
        lines.append("%9d validators: frame %.3f ms (events), (a) frame_host %.3f ms" % (n, dev["frame"]["median_ms"], host["median_ms"]))
    with open(os.path.join(args.out, "probe.json"), "w") as f:
        json.dump(report, f, indent=1)
    with open(os.path.join(args.out, "probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
