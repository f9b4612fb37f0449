"""Times the pending-attestation pool's append and prune (attpool.hip: four launches each -- size,
scan, commit, write) with HIP events:

    bench512   an append of 4,096 rows decoded on the device from the bench's 512-byte records
    configs3   an append of the configs[3] pending list's shape: 4,160 rows of 26-32-byte bitfields
               and one 128 KiB bitfield (the N-bit attestation at 1,048,576 validators), last
    prune      a prune of the configs3 pool that keeps every other row (the long one included)

Per shape: the whole call, one event pair per call, into a pool emptied before every repetition; and
the four launches, one event pair per launch, through the A/B library's pz_debug_att_pool_timed
(build/ab/libprysm_hip.so, or PZ_PROBE_LIB).  3 warm-up calls, then the median of REPS (default 20)
with min and max.  For configs3 the whole call is also timed at other long-range thresholds
(pz_debug_att_pool_long_bytes: the length above which a range is copied by its wave instead of its
lane; 2^40 means every range goes lane by lane).

The yardstick: plain device-to-device copies of the same columns' bytes in the same process (one
torch ``copy_`` per column between contiguous tensors of one dtype, which is one hipMemcpyAsync
each) -- the same traffic with no selection.  The pool's contents are compared with the source
columns, so the probe is also a check at this size.

    python tools/attpool_probe.py [--reps REPS] [--out DIR]   # DIR/probe.json, probe.txt"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prysm_amd import _lib  # noqa: E402

_lib.library_path = os.environ.get("PZ_PROBE_LIB") or os.path.join(ROOT, "build", "ab", "libprysm_hip.so")
from prysm_amd import synth, wire  # noqa: E402
from prysm_amd.pending import DevicePendingAttestations  # noqa: E402

M64 = (1 << 64) - 1
THRESHOLDS = (64, 128, 256, 512, 2048, 16384, 1 << 40)


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def up(a, dev):
    a = np.ascontiguousarray(a)
    a = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
    return torch.from_numpy(a).to(dev)


def bench512(n, dev):
    """n rows decoded on the device from the bench's records; returns (device columns, totals)."""
    recs = synth.attestation_records_512(n)
    d_bytes = up(np.concatenate([recs.reshape(-1), np.zeros(16, np.uint8)]), dev)
    offs = up(np.arange(n + 1, dtype=np.uint64) * recs.shape[1], dev)
    cols = wire.unwire_attestations_device(d_bytes, offs[:-1], offs[1:], n, 0, nbytes=recs.size)
    totals = cols["totals"].cpu().numpy().view(np.uint64)
    assert not int(totals[6]) and not cols["status"][:n].any().item()
    return {k: cols[k] for k in wire.ATT_COLS}, totals[:6]


def configs3(dev, rng):
    n = 4161
    lens = np.concatenate([rng.integers(26, 33, size=n - 1), [128 * 1024]]).astype(np.uint64)
    offs = lambda ls: np.concatenate([[0], np.cumsum(ls)]).astype(np.uint64)  # noqa: E731
    h32 = np.full(n, 32, np.uint64)
    host = {"slot": (np.arange(n, dtype=np.uint64) % 2), "shard_id": rng.integers(0, 1024, size=n).astype(np.uint64),
            "justified_slot": np.zeros(n, np.uint64),
            "justified_block_hash": rng.integers(0, 256, size=32 * n, dtype=np.uint8), "justified_block_hash_offs": offs(h32),
            "shard_block_hash": rng.integers(0, 256, size=32 * n, dtype=np.uint8), "shard_block_hash_offs": offs(h32),
            "attester_bitfield": rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8), "attester_bitfield_offs": offs(lens)}
    host["slot"][-1] = 1  # (the long row survives the prune)
    totals = np.array([32 * n, 32 * n, int(lens.sum()), 0, 0, 0], np.uint64)
    return {k: up(v, dev) for k, v in host.items()}, totals, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sh = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    dll = _lib.lib.dll
    dll.pz_debug_att_pool_timed.argtypes = [_lib.vp, _lib.vp, _lib.u64, _lib.vp, _lib.vp, _lib.vp, _lib.u64, _lib.vp, _lib.vp, _lib.vp]
    dll.pz_debug_att_pool_timed.restype = ctypes.c_int
    dll.pz_debug_att_pool_long_bytes.argtypes = [_lib.u64]
    dll.pz_debug_att_pool_long_bytes.restype = _lib.u64
    default_long = int(dll.pz_debug_att_pool_long_bytes(0))
    dll.pz_debug_att_pool_long_bytes(0)
    rng = np.random.default_rng(11)
    results = {"reps": args.reps, "long_bytes": default_long, "shapes": {}}
    lines = []
    f = lambda x: "%.4f (%.4f-%.4f)" % (x["median_ms"], x["min_ms"], x["max_ms"])  # noqa: E731
    LAUNCHES = ("size", "scan", "commit", "write")

    b_cols, b_tot = bench512(4096, dev)
    c_cols, c_tot, c_host = configs3(dev, rng)
    for name, cols, n, tot in (("bench512", b_cols, 4096, b_tot), ("configs3", c_cols, 4161, c_tot)):
        caps = np.concatenate([[n], tot]).astype(np.uint64) + np.uint64(16)
        pool = DevicePendingAttestations(caps)
        status = torch.zeros(n, dtype=torch.int32, device=dev)  # PZ_ATT_PROCESSED
        comm = torch.arange(n, dtype=torch.int32, device=dev)
        one = torch.zeros(1, dtype=torch.uint8, device=dev)
        ptr = lambda k: (cols[k] if cols[k].numel() else one).data_ptr() if cols.get(k) is not None else None  # noqa: E731
        c = _lib.AttestationCols(*[ptr(k) for k in wire.ATT_COLS])
        scratch = torch.empty(int(dll.pz_att_pool_scratch_bytes(n)), dtype=torch.uint8, device=dev)

        def call():
            _lib.lib.call("pz_dev_att_pool_append", pool._h, ctypes.byref(c), n, status.data_ptr(), comm.data_ptr(), None,
                          scratch.data_ptr(), sh)

        def empty():
            pool.prune(M64)
            torch.cuda.synchronize()

        whole, launches = [], []
        for rep in range(3 + args.reps):
            empty()
            t = timed(call)
            empty()
            ms = (ctypes.c_float * 4)()
            rc = dll.pz_debug_att_pool_timed(pool._h, ctypes.byref(c), n, status.data_ptr(), comm.data_ptr(), None, 0,
                                             scratch.data_ptr(), sh, ms)
            assert rc == 0, dll.pz_last_error()
            if rep >= 3:
                whole.append(t)
                launches.append(list(ms))
        got = pool.columns()
        for k in ("slot", "shard_id", "attester_bitfield_offs", "shard_block_hash_offs"):  # (the probe is also a check)
            assert np.array_equal(got[k], cols[k][:len(got[k])].cpu().numpy().view(np.uint64)), k
        assert np.array_equal(got["attester_bitfield"], cols["attester_bitfield"][:len(got["attester_bitfield"])].cpu().numpy())

        # the yardstick: one device-to-device memcpy per column, the used part of each
        used = {"slot": n, "shard_id": n, "justified_slot": n, "justified_block_hash": int(tot[0]),
                "justified_block_hash_offs": n + 1, "shard_block_hash": int(tot[1]), "shard_block_hash_offs": n + 1,
                "attester_bitfield": int(tot[2]), "attester_bitfield_offs": n + 1, "oblique_parent_hashes": int(tot[4]),
                "oblique_offs": int(tot[3]) + 1, "oblique_first": n + 1, "aggregate_sig": int(tot[5]), "aggregate_sig_first": n + 1}
        pairs = [(cols[k][:used[k]].contiguous(), torch.empty_like(cols[k][:used[k]])) for k in wire.ATT_COLS
                 if cols.get(k) is not None and used[k]]
        nbytes = sum(s.numel() * s.element_size() for s, _ in pairs)
        yard = [timed(lambda: [d.copy_(s) for s, d in pairs]) for _ in range(3 + args.reps)][3:]

        la = np.array(launches)
        row = {"rows": n, "bytes": int(nbytes), "columns": len(pairs), "whole": stats(whole),
               "launches": {k: stats(la[:, j]) for j, k in enumerate(LAUNCHES)}, "yardstick": stats(yard)}
        row["ratio"] = row["whole"]["median_ms"] / row["yardstick"]["median_ms"]
        lines.append("%-8s append of %d rows, %d bytes in %d columns (contents equal)" % (name, n, nbytes, len(pairs)))
        lines.append("  whole %s ms  yardstick (D2D copies) %s ms  ratio %.2f" % (f(row["whole"]), f(row["yardstick"]), row["ratio"]))
        lines.append("  launches  " + "  ".join("%s %s" % (k, f(v)) for k, v in row["launches"].items()))
        if name == "configs3":
            row["thresholds"] = {}
            for thr in THRESHOLDS:
                dll.pz_debug_att_pool_long_bytes(thr)
                ts, ws = [], []
                for rep in range(3 + args.reps):
                    empty()
                    ms = (ctypes.c_float * 4)()
                    rc = dll.pz_debug_att_pool_timed(pool._h, ctypes.byref(c), n, status.data_ptr(), comm.data_ptr(), None, 0,
                                                     scratch.data_ptr(), sh, ms)
                    assert rc == 0, dll.pz_last_error()
                    if rep >= 3:
                        ts.append(sum(ms))
                        ws.append(ms[3])
                row["thresholds"][str(thr)] = {"launches_sum": stats(ts), "write": stats(ws)}
                lines.append("  long_bytes %-14d write %s ms  four launches %s ms" % (thr, f(stats(ws)), f(stats(ts))))
            dll.pz_debug_att_pool_long_bytes(0)
            # the prune that keeps half (slot 1 of slots {0, 1}; the pool holds the appended rows)
            whole, launches = [], []
            for rep in range(3 + args.reps):
                empty()
                call()
                torch.cuda.synchronize()
                t = timed(lambda: pool.prune(0))
                kept = int(pool.counts()[0])
                empty()
                call()
                torch.cuda.synchronize()
                ms = (ctypes.c_float * 4)()
                rc = dll.pz_debug_att_pool_timed(pool._h, None, 0, None, None, None, 0, None, sh, ms)
                assert rc == 0, dll.pz_last_error()
                if rep >= 3:
                    whole.append(t)
                    launches.append(list(ms))
            assert kept == int((c_host["slot"] > 0).sum()) and int(pool.counts()[0]) == kept
            assert np.array_equal(pool.columns()["shard_id"], c_host["shard_id"][c_host["slot"] > 0])
            keep_pairs = [(s[:s.numel() // 2].contiguous(), d[:d.numel() // 2]) for s, d in pairs]
            yard = [timed(lambda: [d.copy_(s) for s, d in keep_pairs]) for _ in range(3 + args.reps)][3:]
            la = np.array(launches)
            prow = {"rows": n, "kept": kept, "whole": stats(whole), "launches": {k: stats(la[:, j]) for j, k in enumerate(LAUNCHES)},
                    "yardstick": stats(yard)}
            prow["ratio"] = prow["whole"]["median_ms"] / prow["yardstick"]["median_ms"]
            results["shapes"]["prune"] = prow
            lines.append("prune    of %d rows keeping %d (every other one and the long one)" % (n, kept))
            lines.append("  whole %s ms  yardstick (D2D copies of half of every column) %s ms  ratio %.2f"
                         % (f(prow["whole"]), f(prow["yardstick"]), prow["ratio"]))
            lines.append("  launches  " + "  ".join("%s %s" % (k, f(v)) for k, v in prow["launches"].items()))
        results["shapes"][name] = row
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
