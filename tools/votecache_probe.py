"""Times the device vote cache's tally (votecache.hip: pz_dev_vote_cache_tally, four launches:
mark, intern, commit, tally) with HIP events on N = 4,096 attestations over the committees of the
genesis split at 65,536 validators (the configs[4] chain's committee sizes), 128 recent hashes:

    m0    no oblique hashes: 64 parents from recent[] per attestation
    m11   11 oblique elements per attestation, of 0, 1, 31, 32, 33 or 40 bytes, drawn from a pool
          of 512 byte strings (equal elements meet in one slot; a 32-byte one skips its parent)

Per shape: the whole call into a fresh cache (every hash new: "cold") and again into the cache it
just filled (every hash found, every voter seen: "warm"), one event pair per call; and the four
phases, one event pair per launch, through the A/B library's pz_debug_vote_cache_tally_timed
(build/ab/libprysm_hip.so, or PZ_PROBE_LIB).  3 warm-up calls, then the median of REPS (default
20) with min and max.

The yardstick: pz_dev_vote_tally over the same batch with the (attestation, slot) work list and
the hash -> slot map built on the host beforehand (not timed) -- the same tally work with no
marking and no interning -- cold and warm alike.  Both caches' totals are compared, so the probe
is also a check at this size.

    python tools/votecache_probe.py [--natt N] [--reps REPS] [--out DIR]   # DIR/probe.json, probe.txt"""
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
from prysm_amd import casper, votes  # noqa: E402
from prysm_amd.types import bytes_to_hash  # noqa: E402

NVAL, N_RECENT, SLOT_CAP = 65536, 128, 2048
LENS = (0, 1, 31, 32, 33, 40)


def build_shape(natt, m, rng):
    """Host columns of one shape and the host-built work list of the yardstick."""
    perm = rng.permutation(NVAL).astype(np.uint32)
    comms = [np.asarray(c, np.uint32) for arr in casper.split_by_slot_shard(list(perm), 0) for _, c in arr]
    coffs = np.zeros(len(comms) + 1, np.uint64)
    coffs[1:] = np.cumsum([len(c) for c in comms])
    members = np.concatenate(comms)
    recent = rng.integers(0, 256, size=(N_RECENT, 32), dtype=np.uint8)
    pool = [rng.bytes(LENS[k % len(LENS)]) for k in range(512)]
    for k in range(0, 512, 16):  # some elements are recent hashes: shared slots and skipped parents
        pool[k] = (b"\x01" if k % 32 else b"") + recent[k % N_RECENT].tobytes()
    comm = (np.arange(natt) % len(comms)).astype(np.uint32)
    pstart = rng.integers(0, N_RECENT - 64 + 1, size=natt).astype(np.uint64)
    bits, boffs, elems, first = [], [0], [], [0]
    for i in range(natt):
        k = len(comms[comm[i]])
        b = rng.random(8 * ((k + 7) // 8)) < 0.6
        b[k:] = False
        bits.append(np.packbits(b))
        boffs.append(boffs[-1] + len(bits[-1]))
        elems += [pool[int(j)] for j in rng.integers(0, 512, size=m)]
        first.append(len(elems))
    ooffs = np.zeros(len(elems) + 1, np.uint64)
    ooffs[1:] = np.cumsum([len(e) for e in elems])
    cols = {"bits": np.concatenate(bits), "boffs": np.array(boffs, np.uint64),
            "obl": np.frombuffer(b"".join(elems) + bytes(4), np.uint8), "ooffs": ooffs,
            "first": np.array(first, np.uint64)}
    # the yardstick's host side: getSignedParentHashes, the skip rule and the interning, in scalar code
    slot_of, item_att, item_slot = {}, [], []
    rec = [r.tobytes() for r in recent]
    for i in range(natt):
        raw = elems[first[i]:first[i + 1]]
        parents = rec[int(pstart[i]):int(pstart[i]) + 64 - m] + [bytes_to_hash(e) for e in raw]
        raw32 = {e for e in raw if len(e) == 32}
        for h in parents:
            if h not in raw32:
                item_att.append(i)
                item_slot.append(slot_of.setdefault(h, len(slot_of)))
    balance = rng.integers(1, 1 << 40, size=NVAL).astype(np.uint64)
    return dict(cols=cols, members=members, coffs=coffs, recent=recent, comm=comm, pstart=pstart, balance=balance,
                slot_of=slot_of, item_att=np.array(item_att, np.uint32), item_slot=np.array(item_slot, np.uint32))


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--natt", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    natt = args.natt
    dev = torch.device("cuda", 0)
    sh = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    dll = _lib.lib.dll
    dll.pz_debug_vote_cache_tally_timed.argtypes = [_lib.vp] * 5
    dll.pz_debug_vote_cache_tally_timed.restype = ctypes.c_int

    def up(a):
        a = np.ascontiguousarray(a)
        a = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
        return torch.from_numpy(a).to(dev)

    results = {"natt": natt, "nval": NVAL, "n_recent": N_RECENT, "reps": args.reps, "shapes": {}}
    lines = []
    for name, m in (("m0", 0), ("m11", 11)):
        s = build_shape(natt, m, np.random.default_rng(7 + m))
        c = s["cols"]
        d = {k: up(v) for k, v in c.items()}
        d_status = torch.zeros(natt, dtype=torch.int32, device=dev)  # PZ_ATT_PROCESSED
        d_comm, d_pstart, d_recent = up(s["comm"]), up(s["pstart"]), up(s["recent"])
        d_members, d_coffs, d_balance = up(s["members"]), up(s["coffs"]), up(s["balance"])
        n_obl = len(c["ooffs"]) - 1
        batch = _lib.VoteColsBatch(
            natt=natt, oblique_parent_hashes=d["obl"].data_ptr() if m else None, oblique_offs=d["ooffs"].data_ptr() if m else None,
            oblique_first=d["first"].data_ptr() if m else None, n_oblique_total=n_obl, bits=d["bits"].data_ptr(),
            boffs=d["boffs"].data_ptr(), status=d_status.data_ptr(), committee=d_comm.data_ptr(),
            parents_start=d_pstart.data_ptr(), recent=d_recent.data_ptr(), n_recent=N_RECENT, members=d_members.data_ptr(),
            coffs=d_coffs.data_ptr(), ncomm=len(s["coffs"]) - 1, balance=d_balance.data_ptr())
        scratch = torch.empty(int(dll.pz_vote_cache_scratch_bytes(natt, N_RECENT, n_obl)), dtype=torch.uint8, device=dev)

        def call(cache):
            _lib.lib.call("pz_dev_vote_cache_tally", cache._h, ctypes.byref(batch), scratch.data_ptr(), sh)

        cold, warm, phases = [], [], []
        cache = None
        for rep in range(3 + args.reps):
            cache = votes.DeviceVoteCache(NVAL, SLOT_CAP)
            tc = timed(lambda: call(cache))
            tw = timed(lambda: call(cache))
            ms = (ctypes.c_float * 4)()
            fresh = votes.DeviceVoteCache(NVAL, SLOT_CAP)
            rc = dll.pz_debug_vote_cache_tally_timed(fresh._h, ctypes.byref(batch), scratch.data_ptr(), sh, ms)
            assert rc == 0, dll.pz_last_error()
            if rep >= 3:
                cold.append(tc)
                warm.append(tw)
                phases.append(list(ms))
        got = cache.items()

        # the yardstick: pz_dev_vote_tally over the host-built work list
        nslots, words = len(s["slot_of"]), (NVAL + 31) // 32
        d_ia, d_is = up(s["item_att"]), up(s["item_slot"])
        bm = torch.zeros((nslots, words), dtype=torch.int32, device=dev)
        tt = torch.zeros(nslots, dtype=torch.int64, device=dev)
        err = torch.zeros(1, dtype=torch.int64, device=dev)
        vb = _lib.VoteBatch(d_members.data_ptr(), d_coffs.data_ptr(), d_comm.data_ptr(), d["bits"].data_ptr(),
                            d["boffs"].data_ptr(), d_ia.data_ptr(), d_is.data_ptr(), len(s["item_att"]),
                            d_balance.data_ptr(), NVAL, bm.data_ptr(), words, tt.data_ptr(), err.data_ptr(), 0, 0)

        def yard():
            _lib.lib.call("pz_dev_vote_tally", ctypes.byref(vb), sh)

        ycold, ywarm = [], []
        for rep in range(3 + args.reps):
            bm.zero_()
            tt.zero_()
            torch.cuda.synchronize()
            tc, tw = timed(yard), timed(yard)
            if rep >= 3:
                ycold.append(tc)
                ywarm.append(tw)
        totals = tt.cpu().numpy().view(np.uint64)
        assert int(err.item()) == 0
        assert got == {h: int(totals[k]) for h, k in s["slot_of"].items()}, "the two caches' totals differ"

        ph = np.array(phases)
        row = {"slots": nslots, "items": int(len(s["item_att"])), "sources": N_RECENT + n_obl,
               "cold": stats(cold), "warm": stats(warm),
               "phases_cold": {k: stats(ph[:, j]) for j, k in enumerate(("mark", "intern", "commit", "tally"))},
               "yardstick_cold": stats(ycold), "yardstick_warm": stats(ywarm)}
        row["ratio_cold"] = row["cold"]["median_ms"] / row["yardstick_cold"]["median_ms"]
        row["ratio_warm"] = row["warm"]["median_ms"] / row["yardstick_warm"]["median_ms"]
        results["shapes"][name] = row
        f = lambda x: "%.4f (%.4f-%.4f)" % (x["median_ms"], x["min_ms"], x["max_ms"])  # noqa: E731
        lines.append("%-4s %d slots, %d items, %d sources (totals equal)" % (name, nslots, row["items"], row["sources"]))
        lines.append("  cold  cache %s ms  yardstick %s ms  ratio %.2f" % (f(row["cold"]), f(row["yardstick_cold"]), row["ratio_cold"]))
        lines.append("  warm  cache %s ms  yardstick %s ms  ratio %.2f" % (f(row["warm"]), f(row["yardstick_warm"]), row["ratio_warm"]))
        lines.append("  cold phases  " + "  ".join("%s %s" % (k, f(v)) for k, v in row["phases_cold"].items()))
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
