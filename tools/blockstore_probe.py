"""Times the attestation store batch (blockstore.hip: pz_dev_block_store_select, four launches;
pz_dev_block_store_digests, three) and the chain that asks for it.  No bar is set: the figures are
reported.

    launches  over the decoded columns of (a) synth.chain_blocks(1024, 130, seed=4), one row a block,
              and (b) a synthetic run of 1,024 blocks x 64 rows, every row saved: select under one event
              pair, the three digest launches (the span hash over the pairs, the key kernel through the
              row list, the list entries) under one pair each (the A/B library's
              pz_debug_block_store_select_timed / _digests_timed).  Beside them the same rows through
              blockchain.digest_serialized_blocks -- a second upload and decode of the same bytes, then
              every row of every block hashed: how a caller gets Key and Hash without the store --
              under one event pair and on the host clock.  The first repetition compares the store's
              key and hash with that call's.
    chain     synth.chain_blocks(1024, 330, seed=4) through ResidentChain.process_all, host clock round
              the call and a device synchronise, fresh genesis objects per repetition, with the store
              off, on, or both alternating (--store).  With ``--store off`` the file uses nothing the
              store added, so it times the parent commit's tree when it is run from there with
              ``--chain-only``, which also keeps to the product library.

3 warm-up rounds, then the median of REPS (default 20) with min and max.

    python tools/blockstore_probe.py [--reps REPS] [--store off|on|both] [--chain-only] [--out DIR] [--tag TAG]"""
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

if os.environ.get("PZ_PROBE_LIB"):
    _lib.library_path = os.environ["PZ_PROBE_LIB"]
elif "--chain-only" not in sys.argv:
    _lib.library_path = os.path.join(ROOT, "build", "ab", "libprysm_hip.so")
from oracle import ref  # noqa: E402
from prysm_amd import blockchain as bc  # noqa: E402
from prysm_amd import pb, synth  # noqa: E402
from prysm_amd.pending import DevicePendingAttestations, DeviceRecentHashes, DeviceSavedBlocks, ResidentRecalcState  # noqa: E402
from prysm_amd.votes import DeviceVoteCache  # noqa: E402

NVAL = 1024
CAPS = [256, 256 * 32, 256 * 32, 256 * 8, 256, 256 * 32, 512]
WARM = 3


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def fmt(x):
    return "%.4f (%.4f-%.4f)" % (x["median_ms"], x["min_ms"], x["max_ms"])


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


def table_of(cs):
    return [[(sc.shard_id, list(sc.committee)) for sc in arr.array_shard_and_committee] for arr in cs.shard_and_committees_for_slots]


def wide_blocks(nblocks, rows, seed=9):
    """``nblocks`` blocks of ``rows`` attestations: two 32-byte hashes, 4 bitfield bytes, one oblique hash, two sig values."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(1, nblocks + 1):
        atts = [pb.AttestationRecord(slot=0, shard_id=int(rng.integers(0, 1024)), justified_slot=0, justified_block_hash=rng.bytes(32),
                                     shard_block_hash=rng.bytes(32), attester_bitfield=rng.bytes(4), oblique_parent_hashes=[rng.bytes(32)],
                                     aggregate_sig=[int(x) for x in rng.integers(0, 1 << 62, size=2)]) for _ in range(rows)]
        out.append(pb.BeaconBlock(parent_hash=rng.bytes(32), slot_number=s, timestamp=pb.Timestamp(8 * s, 0), attestations=atts))
    return out


def launches(name, blocks, tab, reps):
    """Select and the three digest launches over every row of ``blocks``, all saved, beside
    digest_serialized_blocks over the same bytes."""
    sel = _lib.lib.dll.pz_debug_block_store_select_timed
    sel.argtypes, sel.restype = [_lib.vp, _lib.vp, _lib.vp, _lib.vp], ctypes.c_int
    dig = _lib.lib.dll.pz_debug_block_store_digests_timed
    dig.argtypes, dig.restype = [_lib.vp, _lib.vp, _lib.u64, _lib.vp, _lib.vp], ctypes.c_int
    data, offs = bc.serialize_blocks(blocks)
    n = len(offs) - 1
    payload = np.concatenate([data[:int(offs[-1])], np.zeros(4, np.uint8)])
    d = bc._split_decode_check(payload, offs, 0, 0, 128, tab, 0, want_committee=False)
    dev, blk, natt = d["dev"], d["blk"], d["natt"]
    p = _lib.dptr
    ok_rows = torch.zeros(natt, dtype=torch.int32, device=dev)  # every row saved, whatever the checks said
    parent_ok = torch.ones(n, dtype=torch.uint8, device=dev)
    rows = torch.empty(natt, dtype=torch.int32, device=dev)
    span = torch.empty((natt, 2), dtype=torch.int64, device=dev)
    first = torch.empty(n + 1, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    key, hash_ = (torch.empty((natt, 32), dtype=torch.uint8, device=dev) for _ in range(2))
    lists = torch.empty(34 * natt + 2, dtype=torch.uint8, device=dev)
    scratch = torch.empty(int(_lib.lib.dll.pz_block_store_scratch_bytes(n, natt)), dtype=torch.uint8, device=dev)
    b = _lib.BlockStoreBatch(nblocks=n, att_first=p(blk["att_first"]), block_status=p(d["block_status"]), parent_ok=p(parent_ok), natt=natt,
                             att_block=p(blk["att_block"]), att_status=p(ok_rows), att_beg=p(blk["att_beg"]), att_end=p(blk["att_end"]),
                             rows=p(rows), span=p(span), first=p(first), count=p(count), bytes=p(d["d_bytes"]), key=p(key), hash=p(hash_),
                             lists=p(lists))
    cols = _lib.att_cols(d["att"], ("slot", "shard_id", "shard_block_hash", "shard_block_hash_offs", "oblique_parent_hashes",
                                    "oblique_offs", "oblique_first"))
    ms1, ms3 = (ctypes.c_float * 1)(), (ctypes.c_float * 3)()
    t = {"select": [], "hash": [], "key": [], "lists": [], "digest_serialized_blocks_events": [], "digest_serialized_blocks_host": []}
    recent = np.zeros((128, 32), np.uint8)
    for rep in range(WARM + reps):
        assert sel(ctypes.byref(b), p(scratch), _lib.stream_ptr(dev), ms1) == 0
        assert dig(ctypes.byref(b), ctypes.byref(cols), natt, _lib.stream_ptr(dev), ms3) == 0
        ev, host, out = timed(lambda: bc.digest_serialized_blocks(data, offs, 0, 0, 128, tab, recent))
        if rep == 0:  # the store's digests are the ones a caller gets today
            assert int(count.item()) == natt and (out["block_status"] == 0).all()
            np.testing.assert_array_equal(key.cpu().numpy(), out["key"])
            np.testing.assert_array_equal(hash_.cpu().numpy(), out["hash"])
            want = np.concatenate([np.tile(np.array([0x0a, 0x20], np.uint8), (natt, 1)), out["hash"]], axis=1).reshape(-1)
            np.testing.assert_array_equal(lists[:34 * natt].cpu().numpy(), want)
        if rep >= WARM:
            for k, v in zip(t, (ms1[0], ms3[0], ms3[1], ms3[2], ev, host)):
                t[k].append(v)
    res = {"blocks": n, "rows": natt, **{k: stats(v) for k, v in t.items()}}
    line = ("%s  %d blocks, %d rows, all saved: select %s ms; digests: span hash %s, key through the row list %s, list entries %s ms;\n"
            "    digest_serialized_blocks over the same bytes: events %s ms, host clock %s ms"
            % (name, n, natt, fmt(res["select"]), fmt(res["hash"]), fmt(res["key"]), fmt(res["lists"]),
               fmt(res["digest_serialized_blocks_events"]), fmt(res["digest_serialized_blocks_host"])))
    return res, line


def fresh(cs, tab):
    """Genesis objects: cache, pool, ring, saved set, state."""
    state = ResidentRecalcState(
        [v.balance for v in cs.validators], [v.start_dynasty for v in cs.validators], [v.end_dynasty for v in cs.validators],
        [v for arr in tab for e in arr for v in e[1]], bc._committee_table(tab)[3], cs.crosslink_records,
        last_state_recalc=cs.last_state_recalc, justified_streak=cs.justified_streak, last_justified_slot=cs.last_justified_slot,
        last_finalized_slot=cs.last_finalized_slot, current_dynasty=cs.current_dynasty, total_deposits=cs.total_deposits)
    return DeviceVoteCache(NVAL, 2048), DevicePendingAttestations(CAPS), DeviceRecentHashes(), DeviceSavedBlocks(), state


def chain(cs, tab, reps, modes):
    """process_all over five cycles, the modes alternating inside every repetition."""
    blocks = synth.chain_blocks(NVAL, 330, seed=4)
    data, offs = bc.serialize_blocks(blocks)
    t, shape = {m: [] for m in modes}, {}
    for rep in range(WARM + reps):
        for m in (modes if rep % 2 == 0 else modes[::-1]):
            objs = fresh(cs, tab)

            def run():
                rc = bc.ResidentChain(*objs, tab)
                if m == "on":
                    rc.store = True
                return rc, rc.process_all(data, offs)

            _, host, (rc, outs) = timed(run)
            if rep == 0:
                shape[m] = {"calls": rc.calls, "resubmits": rc.resubmits, "cuts": [(o["start"], o["stop"]) for o in outs],
                            "saved_rows": sum(int(o["store"]["first"][-1]) for o in outs) if m == "on" else None}
                assert ("store" in outs[0]) == (m == "on")
            if rep >= WARM:
                t[m].append(host)
    res = {m: {"host": stats(v), **shape[m]} for m, v in t.items()}
    lines = ["chain330  store %-3s  process_all host clock %s ms   %d submissions (%d resubmitted)%s"
             % (m, fmt(r["host"]), r["calls"], r["resubmits"], "" if m == "off" else ", %d rows saved" % r["saved_rows"]) for m, r in res.items()]
    if len(modes) == 2:
        add = res["on"]["host"]["median_ms"] - res["off"]["host"]["median_ms"]
        lines.append("chain330  the store adds %.4f ms, %.4f ms a submission" % (add, add / res["on"]["calls"]))
    return res, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--store", choices=("off", "on", "both"), default="both")
    ap.add_argument("--chain-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="probe")
    args = ap.parse_args()
    _, cs = ref.new_genesis_states(NVAL)
    tab = table_of(cs)
    results, lines = {"reps": args.reps}, []
    if not args.chain_only:
        for name, blocks in (("chain130 ", synth.chain_blocks(NVAL, 130, seed=4)), ("wide1024 ", wide_blocks(1024, 64))):
            results[name.strip()], line = launches(name, blocks, tab, args.reps)
            lines.append(line)
    results["chain330"], more = chain(cs, tab, args.reps, ["off", "on"] if args.store == "both" else [args.store])
    lines += more
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, args.tag + ".json"), "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")
        with open(os.path.join(args.out, args.tag + ".txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
