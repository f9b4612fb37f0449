"""Times the device vote cache's retirement and growth (votecache.hip: pz_dev_vote_cache_retain, two
memsets and the keep, renumber, move and rehash launches; pz_dev_vote_cache_reserve, one memset and
move and rehash) and the chain that needs them.  No bar is set: the figures are reported.

    moves   at 65,536 and 1,048,576 validators, a cache of 512 entries (every voter row with bits):
            retain 512 -> 129 kept, and reserve 512 -> 1,024 slots.  Every repetition starts from a
            fresh cache filled outside the timed region.  Each step gets one event pair (the A/B
            library's pz_debug_vote_cache_move_timed) and the whole product call one pair more.
            Beside them, in the same run: a plain device-to-device copy of the bytes the move has to
            carry (the kept rows: voters, key and total), one of the bytes it writes (every row of the
            new set, the zeroed ones included), and the floor: the same steps on a cache of 4 slots
            and 32 validators, where they move next to nothing.
    chain   synth.chain_blocks(1024, 330, seed=4) through ResidentChain.process_all, host clock round
            the call and a device synchronise, fresh genesis objects per repetition: the policies
            given with --chain as policy:slots (default retire:256 and fixed:512).  The two end states
            are compared after the first repetition.  ``fixed`` uses nothing this file's tree added,
            so the same file times the parent commit's tree when it is run from there.

3 warm-up rounds, then the median of REPS (default 10) with min and max.  The first repetition of
every move checks the cache against the expected entries before any time is trusted.

    python tools/votecache_retain_probe.py [--reps REPS] [--chain POLICY:SLOTS ...] [--no-moves] [--out DIR]"""
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
from prysm_amd import synth  # noqa: E402
from prysm_amd.pending import DevicePendingAttestations, DeviceRecentHashes, DeviceSavedBlocks, ResidentRecalcState  # noqa: E402
from prysm_amd.votes import DeviceVoteCache  # noqa: E402

CAPS = [256, 256 * 32, 256 * 32, 256 * 8, 256, 256 * 32, 512]
ENTRIES, KEPT, GROWN = 512, 129, 1024
STEPS = ("memset_flags", "keep", "renumber", "memset_table", "move", "rehash")
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


# ---- moves --------------------------------------------------------------------------------------------------------
class Filler:
    """A cache of ``entries`` hashes, each voted for by about half of one committee of 4,096 validators."""

    def __init__(self, nval, slot_cap, entries, rng):
        dev = torch.device("cuda", 0)
        self.nval, self.slot_cap, self.entries = nval, slot_cap, entries
        self.hashes = rng.integers(0, 256, size=(max(entries, 64), 32), dtype=np.uint8)
        self.hashes[entries:] = self.hashes[0]  # (a window is 64 hashes: a smaller cache repeats one)
        k = len(self.hashes)
        starts = list(range(0, k - 63, 64)) + [k - 64]
        csize = min(4096, nval)
        bits = [np.packbits(rng.random(csize) < 0.5) for _ in starts]
        t = lambda a: bc._to_device(np.ascontiguousarray(a), dev)  # noqa: E731
        self.cols = {"attester_bitfield": t(np.concatenate(bits)),
                     "attester_bitfield_offs": t(np.arange(len(starts) + 1, dtype=np.uint64) * np.uint64(len(bits[0])))}
        self.n = len(starts)
        self.status = t(np.zeros(self.n, np.int32))
        self.comm = t(np.zeros(self.n, np.uint32))
        self.pstart = t(np.array(starts, np.uint64))
        self.recent = t(self.hashes)
        self.members = t(rng.permutation(nval)[:csize].astype(np.uint32))
        self.coffs = t(np.array([0, csize], np.uint64))
        self.balance = t(rng.integers(1, 1 << 30, size=nval).astype(np.uint64))

    def fresh(self):
        cache = DeviceVoteCache(self.nval, self.slot_cap)
        cache.tally_columns(self.cols, self.n, self.status, self.comm, self.pstart, self.recent, self.members, self.coffs, self.balance)
        torch.cuda.synchronize()
        return cache


def timed_move(cache, min_slots, keep, scratch):
    fn = _lib.lib.dll.pz_debug_vote_cache_move_timed
    fn.argtypes, fn.restype = [_lib.vp, _lib.u32, ctypes.c_int, _lib.vp, _lib.u64, _lib.vp, _lib.vp, _lib.vp], ctypes.c_int
    ms = (ctypes.c_float * 6)()
    n = 0 if keep is None else int(keep.numel()) // 32
    rc = fn(cache._h, min_slots, int(keep is not None), _lib.dptr(keep), n, _lib.dptr(scratch), _lib.stream_ptr(0), ms)
    assert rc == 0, (rc, _lib.lib.dll.pz_last_error())
    return list(ms)


def moves_at(nval, slot_cap, entries, kept, grown, reps, rng):
    """Step and whole-call times of retain entries -> kept and reserve slot_cap -> grown."""
    dev = torch.device("cuda", 0)
    fill = Filler(nval, slot_cap, entries, rng)
    keys = fill.hashes[:entries]
    pick = np.sort(rng.choice(entries, kept, replace=False))
    keep = bc._to_device(np.ascontiguousarray(keys[pick]), dev)
    scratch = torch.empty(int(_lib.lib.dll.pz_vote_cache_retain_scratch_bytes(slot_cap, kept)), dtype=torch.uint8, device=dev)
    words = (nval + 31) // 32
    row = 4 * words + 40
    out = {"validators": nval, "slots": slot_cap, "entries": entries, "kept": kept, "grown_to": grown, "row_bytes": row,
           "retain_carried_bytes": kept * row, "retain_written_bytes": slot_cap * row,
           "reserve_carried_bytes": entries * row, "reserve_written_bytes": grown * row}
    steps = {"retain": [], "reserve": []}
    whole = {"retain": [], "reserve": []}
    for rep in range(WARM + reps):
        c = fill.fresh()
        before = c.read()
        ms = timed_move(c, 0, keep, scratch)
        if rep == 0:
            h, t = c.read()
            assert np.array_equal(h, keys[pick]) and np.array_equal(t, before[1][pick]) and c._capacity() == slot_cap
        c2 = fill.fresh()
        w = events(lambda: c2.retain(keep))
        if rep == 0:
            assert np.array_equal(c2.read()[0], keys[pick])
        c3 = fill.fresh()
        ms_r = timed_move(c3, grown, None, None)
        if rep == 0:
            h, t = c3.read()
            assert np.array_equal(h, before[0]) and np.array_equal(t, before[1]) and c3._capacity() == grown
        c4 = fill.fresh()
        w_r = events(lambda: c4.reserve(grown, device_form=True))
        if rep >= WARM:
            steps["retain"].append(ms), steps["reserve"].append(ms_r)
            whole["retain"].append(w), whole["reserve"].append(w_r)
        del c, c2, c3, c4
    for what in ("retain", "reserve"):
        first = 0 if what == "retain" else 3
        out[what] = {"steps": {STEPS[k]: stats([s[k] for s in steps[what]]) for k in range(first, 6)},
                     "steps_sum": stats([sum(s[first:]) for s in steps[what]]), "whole_call_events": stats(whole[what])}
    # plain device-to-device copies of the same bytes, in the same run
    for name in ("retain_carried_bytes", "retain_written_bytes", "reserve_carried_bytes", "reserve_written_bytes"):
        src = torch.empty(out[name], dtype=torch.uint8, device=dev).random_(0, 256)
        dst = torch.empty_like(src)
        ts = [events(lambda: dst.copy_(src)) for _ in range(WARM + reps)][WARM:]
        out["copy_" + name] = stats(ts)
        out["copy_" + name]["gb_per_s"] = out[name] / (np.median(ts) * 1e-3) / 1e9
        del src, dst
    return out


# ---- chain --------------------------------------------------------------------------------------------------------
def genesis(nval, slots, policy):
    _, cs = ref.new_genesis_states(nval)
    tab = [[(sc.shard_id, list(sc.committee)) for sc in arr.array_shard_and_committee] for arr in cs.shard_and_committees_for_slots]
    state = ResidentRecalcState(
        [v.balance for v in cs.validators], [v.start_dynasty for v in cs.validators], [v.end_dynasty for v in cs.validators],
        [v for arr in tab for e in arr for v in e[1]], bc._committee_table(tab)[3], cs.crosslink_records,
        last_state_recalc=cs.last_state_recalc, justified_streak=cs.justified_streak, last_justified_slot=cs.last_justified_slot,
        last_finalized_slot=cs.last_finalized_slot, current_dynasty=cs.current_dynasty, total_deposits=cs.total_deposits)
    kw = {} if policy == "fixed" else {"cache_policy": policy}  # (fixed: nothing this tree added)
    return bc.ResidentChain(DeviceVoteCache(nval, slots), DevicePendingAttestations(CAPS), DeviceRecentHashes(), DeviceSavedBlocks(),
                            state, tab, **kw)


def chain_runs(specs, reps):
    nval = 1024
    data, offs = bc.serialize_blocks(synth.chain_blocks(nval, 330, seed=4))
    out, ends = {}, {}
    times = {s: [] for s in specs}
    for rep in range(WARM + reps):
        order = specs if rep % 2 == 0 else specs[::-1]  # neither always runs behind the other
        for spec in order:
            policy, slots = spec.split(":")
            rc = genesis(nval, int(slots), policy)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = rc.process_all(data, offs)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if rep == 0:
                s = rc.state
                ends[spec] = (rc.ring.hashes(), tuple(getattr(s, k) for k in s._SCALARS), s.balances().tobytes(),
                              [(o["start"], o["stop"]) for o in outs])
                out[spec] = {"calls": rc.calls, "entries": len(rc.cache.read()[1]), "capacity": int(rc.cache.slot_cap),
                             "retains": getattr(rc, "cache_retains", 0), "grows": getattr(rc, "cache_grows", 0)}
            if rep >= WARM:
                times[spec].append(dt)
    assert all(e == ends[specs[0]] for e in ends.values()), "the policies' end states differ"
    for spec in specs:
        out[spec]["process_all_host"] = stats(times[spec])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--chain", nargs="*", default=["retire:256", "fixed:512"])
    ap.add_argument("--no-moves", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(31)
    results, lines = {"reps": args.reps, "warmup": WARM}, []
    if not args.no_moves:
        results["floor"] = moves_at(32, 4, 2, 1, 8, args.reps, rng)
        results["moves"] = [moves_at(nval, ENTRIES, ENTRIES, KEPT, GROWN, args.reps, rng) for nval in (65536, 1048576)]
        fl = results["floor"]
        lines.append("floor: the same steps on 4 slots of 32 validators: retain %s ms (whole call %s), reserve %s ms (whole call %s)"
                     % (fmt(fl["retain"]["steps_sum"]), fmt(fl["retain"]["whole_call_events"]), fmt(fl["reserve"]["steps_sum"]),
                        fmt(fl["reserve"]["whole_call_events"])))
        for m in results["moves"]:
            lines.append("%d validators, %d-byte rows" % (m["validators"], m["row_bytes"]))
            for what, a, b in (("retain", "%d -> %d kept" % (m["entries"], m["kept"]), "retain"),
                               ("reserve", "%d -> %d slots" % (m["slots"], m["grown_to"]), "reserve")):
                r = m[what]
                lines.append("  %s %s: steps %s ms, whole call %s ms" % (what, a, fmt(r["steps_sum"]), fmt(r["whole_call_events"])))
                lines.append("    " + ", ".join("%s %s" % (k, fmt(v)) for k, v in r["steps"].items()))
                for kind in ("carried", "written"):
                    c = m["copy_%s_%s_bytes" % (b, kind)]
                    lines.append("    plain copy of the %s bytes (%.1f MB): %s ms, %.0f GB/s"
                                 % (kind, m["%s_%s_bytes" % (b, kind)] / 1e6, fmt(c), c["gb_per_s"]))
    if args.chain:
        results["chain"] = chain_runs(list(args.chain), args.reps)
        for spec, r in results["chain"].items():
            lines.append("chain330 %-11s process_all host clock %s ms; %d calls, %d entries in %d slots, %d retains, %d grows"
                         % (spec, fmt(r["process_all_host"]), r["calls"], r["entries"], r["capacity"], r["retains"], r["grows"]))
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
