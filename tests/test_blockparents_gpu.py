"""The resident saved-block set and the parent check on the GPU (prysm_amd/csrc/blockparents.hip;
pending.DeviceSavedBlocks, blockchain.walk_serialized_blocks_saved):

1. the three launches of pz_[dev_]block_parents and the insert after the walk on synthetic columns,
   device and host forms, against a block-by-block Python restatement of blockchain/service.go:261-269
   + :324 over a set that only grows (copies whose caller masks differ included), with canary bytes
   behind every output;
2. the set alone: contains / insert / reserve against a Python set -- keys sharing a home cell in an
   8-cell table, the zero hash, duplicates inside one insert, a full table's capacity bit;
3. blocks 1..63 of the 130-block chain in ONE call with the set in place of the mask: every output
   equals the all-eligible call's, and cache, pool, ring and set equal oracle.replay.Chain's;
4. the same run with a block removed, two swapped, one delivered late and again, and a block whose
   last attestation fails before its child, each against the oracle stepped block by block;
5. the siblings run of test_blockwalk_gpu.py with the set seeded instead of a mask;
6. the whole chain across both transitions with the set; 7. a panic row leaves the set too."""
import copy
import ctypes
import functools
import hashlib

import numpy as np
import pytest

from oracle import ref
from oracle import replay as oreplay
from prysm_amd import _lib, pb, wire
from prysm_amd import blockchain as bc
from prysm_amd.pending import DeviceSavedBlocks
from test_attpool_gpu import late_chain, table
from test_blockwalk_gpu import CANARY, check_against, check_digests, genesis_objects, padded
from test_votecache_gpu import snapshot

pytestmark = pytest.mark.gpu

U64 = np.uint64
PROCESSED = 0
SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049]


# ---- 1: the kernels on synthetic columns ------------------------------------------------------------------
def blk(hash_, parent, slot=10, rows=1, last_ok=True, rec_bad=False, status=0):
    return {"hash": bytes(hash_), "parent": bytes(parent), "slot": slot, "rows": rows, "last_ok": last_ok, "rec_bad": rec_bad,
            "status": status}


def chain(rng, n, root):
    out, parent = [], root
    for j in range(n):
        out.append(blk(rng.bytes(32), parent, slot=2 + j, rows=int(rng.integers(1, 4))))
        parent = out[-1]["hash"]
    return out


def runs_for(n, rng):
    """``(name, blocks, initial keys)``: the cases of the stand-alone CPU check, at one size."""
    root = rng.bytes(32)
    db = [root, rng.bytes(32), bytes(32)]
    out = [("linear chain", chain(rng, n, root), db), ("unknown root", chain(rng, n, rng.bytes(32)), db)]
    if n >= 2:
        k = n // 2 - 1
        c = chain(rng, n + 1, root)
        out.append(("one block removed", c[:n // 2] + c[n // 2 + 1:], db))
        c = chain(rng, n, root)
        out.append(("a child before its parent", c[:k] + [c[k + 1], c[k]] + c[k + 2:], db))
        out.append(("delivered twice", c[:k + 1] + [c[k + 1], c[k]] + c[k + 1:], db))
        for masks in ((1, 0), (0, 1)):  # copies whose caller masks differ, in both orders
            a, b = dict(c[k], status=masks[0]), dict(c[k], status=masks[1])
            out.append(("masks %r" % (masks,), c[:k] + [a, c[k + 1], b] + c[k + 1:], db))
        c = chain(rng, n, root)
        c[n // 2]["last_ok"], c[n // 3]["rows"], c[n - 1 - n // 4]["rec_bad"] = False, 0, True
        out.append(("closed parents", c, db))
    if n >= 1:
        c = chain(rng, n, rng.bytes(32))
        for j in range(0, n, 5):
            c[j]["slot"] = (j // 5) % 2
        out.append(("slots 0 and 1", c, db))
        c = chain(rng, n, root)  # parent spans of 0, 31, 32 and 33 bytes; block 2 carries the zero hash
        for j in range(1, n):
            if j % 4 == 1:
                c[j - 1]["hash"] = b"\x00" + c[j - 1]["hash"][1:]
            if j == 3:
                c[j - 1]["hash"] = bytes(32)
        for j in range(1, n):
            h = c[j - 1]["hash"]
            c[j]["parent"] = b"" if j == 3 else h[1:] if j % 4 == 1 else b"\x07" + h if j % 4 == 2 else h
        out.append(("spans of 0, 31, 32, 33 bytes", c, [root]))
        z = chain(rng, n, b"")
        out.append(("the zero hash in the set", z, db))
        out.append(("the zero hash not in the set", z, [root]))
    # a random mix over a small universe: copies, forks, early children, closed parents, masks
    uni = []
    for k in range(max(2, n // 2)):
        pick = int(rng.integers(0, 10))
        par = uni[int(rng.integers(0, k))]["hash"] if pick < 7 and k else db[int(rng.integers(0, 3))] if pick < 9 else rng.bytes(32)
        uni.append(blk(rng.bytes(32), par, slot=int(rng.integers(0, 2)) if rng.integers(0, 12) == 0 else 2 + k,
                       rows=int(rng.integers(0, 4)), last_ok=bool(rng.integers(0, 6)), rec_bad=not rng.integers(0, 12)))
    mix = [dict(uni[min(len(uni) - 1, j // 2 + int(rng.integers(0, 3)))], status=int(rng.integers(0, 7) == 0)) for j in range(n)]
    out.append(("random", mix, db))
    return out


def assemble(rng, blocks):
    n = len(blocks)
    r = {"n": n, "slot": np.array([b["slot"] for b in blocks], U64), "status": np.array([b["status"] for b in blocks], np.int32),
         "hash": np.frombuffer(b"".join(b["hash"] for b in blocks), np.uint8).reshape(n, 32).copy()}
    beg, ln, data = np.full(5 * n, (1 << 64) - 1, U64), np.full(5 * n, 0xFFFFFFFF, np.uint32), bytearray(rng.bytes(3))
    att, rec, first = [], [], [0]
    for j, b in enumerate(blocks):
        beg[5 * j], ln[5 * j] = len(data) if b["parent"] else int(rng.integers(0, 1000)), len(b["parent"])
        data += b["parent"] + rng.bytes(int(rng.integers(0, 3)))
        for k in range(b["rows"]):
            last = k == b["rows"] - 1
            att.append(PROCESSED if (b["last_ok"] if last else rng.integers(0, 3)) else int(rng.choice([1, 4, 6])))
            rec.append(_lib.PZ_EINVAL if b["rec_bad"] and k == 0 else 0)
        first.append(len(att))
    r.update(bytes=np.frombuffer(bytes(data), np.uint8).copy(), bytes_beg=beg, bytes_len=ln, att_first=np.array(first, U64),
             att_status=np.array(att, np.int32), rec_status=np.array(rec, np.int32), natt=len(att))
    return r


def model(blocks, initial):
    """service.go:261-269 + :324 block by block, with a set that only grows."""
    db = set(initial)
    ok, saved = np.zeros(len(blocks), np.uint8), np.zeros(len(blocks), np.uint8)
    for j, b in enumerate(blocks):
        ok[j] = b["slot"] <= 1 or ref.bytes_to_hash(b["parent"]) in db
        if ok[j] and b["status"] == 0 and not b["rec_bad"] and b["rows"] > 0 and b["last_ok"]:
            saved[j] = 1
            db.add(b["hash"])
    return ok, saved


def run_parents(form, r, saved):
    """``(parent_ok, saved0, block_status_out)`` of pz_dev_block_parents / pz_block_parents."""
    import torch

    n = r["n"]
    if form == "host":
        pad = 16  # canary elements behind every output: the staging copy-back writes n elements and no more
        whole = {"parent_ok": np.full(n + pad, CANARY, np.uint8), "saved0": np.full(n + pad, CANARY, np.uint8),
                 "status_out": np.full(n + pad, 0x5A5A5A5A, np.int32)}
        got = {k: v[:n] for k, v in whole.items()}
        hp = lambda a: a.ctypes.data if a.size else None  # noqa: E731  (views of the padded arrays included)
        b = _lib.BlockParentsBatch(nblocks=n, bytes=hp(r["bytes"]), nbytes=r["bytes"].size, bytes_beg=hp(r["bytes_beg"]),
                                   bytes_len=hp(r["bytes_len"]), slot_number=hp(r["slot"]), block_hash=hp(r["hash"]),
                                   att_first=r["att_first"].ctypes.data, block_status=hp(r["status"]), rec_status=hp(r["rec_status"]),
                                   att_status=hp(r["att_status"]), natt=r["natt"], parent_ok=hp(got["parent_ok"]),
                                   saved0=hp(got["saved0"]), block_status_out=hp(got["status_out"]))
        _lib.lib.call("pz_block_parents", saved._h, ctypes.byref(b))
        for k, v in whole.items():
            assert (v[n:] == (0x5A5A5A5A if k == "status_out" else CANARY)).all(), k  # nothing is written behind an output
        return got
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    ins = {k: put(r[k]) for k in ("bytes", "bytes_beg", "bytes_len", "slot", "hash", "att_first", "status", "rec_status", "att_status")}
    outs = {"parent_ok": padded(np.full(n, CANARY, np.uint8)), "saved0": padded(np.full(n, CANARY, np.uint8)),
            "status_out": padded(np.full(n, 0x5A5A, np.int32))}
    nscr = int(_lib.lib.dll.pz_block_parents_scratch_bytes(n))
    scratch = torch.full((nscr + 64,), CANARY, dtype=torch.uint8, device="cuda")
    p = {k: (t.data_ptr() if used else None) for k, (t, used) in outs.items()}
    d = _lib.dptr
    b = _lib.BlockParentsBatch(nblocks=n, bytes=d(ins["bytes"]), nbytes=r["bytes"].size, bytes_beg=d(ins["bytes_beg"]),
                               bytes_len=d(ins["bytes_len"]), slot_number=d(ins["slot"]), block_hash=d(ins["hash"]),
                               att_first=d(ins["att_first"]), block_status=d(ins["status"]), rec_status=d(ins["rec_status"]),
                               att_status=d(ins["att_status"]), natt=r["natt"], parent_ok=p["parent_ok"], saved0=p["saved0"],
                               block_status_out=p["status_out"])
    _lib.lib.call("pz_dev_block_parents", saved._h, ctypes.byref(b), scratch.data_ptr(), _lib.stream_ptr(0))
    torch.cuda.synchronize()
    assert (scratch[nscr:].cpu().numpy() == CANARY).all()  # nothing is written behind the scratch
    got = {}
    for k, (t, used) in outs.items():
        host = t.cpu().numpy()
        assert (host[used:] == CANARY).all(), k  # nor behind an output
        got[k] = host[:used].view(np.int32 if k == "status_out" else np.uint8)
    return got


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("n", SIZES)
def test_kernels_on_synthetic_columns(n, form):
    import torch

    rng = np.random.default_rng(2000 + n)
    classes = set()
    for name, blocks, initial in runs_for(n, rng):
        r = assemble(rng, blocks)
        n_run = r["n"]
        ok, saved0 = model(blocks, initial)
        dev_set = DeviceSavedBlocks(initial, min_keys=4)
        got = run_parents(form, r, dev_set)
        if n_run == 0:  # nothing is launched
            assert dev_set.count() == len(set(initial)), name
            continue
        np.testing.assert_array_equal(got["parent_ok"], ok, name)
        np.testing.assert_array_equal(got["saved0"], saved0, name)
        np.testing.assert_array_equal(got["status_out"], np.where(ok != 0, r["status"], _lib.PZ_ENOTFOUND), name)
        classes |= {(int(a), int(b)) for a, b in zip(ok, saved0)}
        # the insert after a walk that stops somewhere; every fourth case the gate's panic bit
        stop = n_run if rng.integers(0, 3) else int(rng.integers(0, n_run + 1))
        walk = np.where(np.arange(n_run) >= stop, 3, np.where(saved0 != 0, 1 + rng.integers(0, 2, n_run), 0)).astype(np.uint8)
        panic = int(rng.integers(0, 4) == 0)
        want = set(initial) | ({b["hash"] for j, b in enumerate(blocks) if saved0[j] and j < stop} if not panic else set())
        dev_set.reserve(len(set(initial)) + n_run)
        word, used = padded(np.zeros(1, U64))
        d_hash, d_walk, d_flags = torch.from_numpy(r["hash"]).cuda(), torch.from_numpy(walk).cuda(), torch.tensor([panic], dtype=torch.int32).cuda()
        _lib.lib.call("pz_dev_block_set_insert_walked", dev_set._h, d_hash.data_ptr(), d_walk.data_ptr(), d_flags.data_ptr(), n_run,
                      word.data_ptr(), _lib.stream_ptr(0))
        host = word.cpu().numpy()
        assert int(host[:8].view(U64)[0]) == len(want) and (host[used:] == CANARY).all(), name
        assert set(dev_set.hashes()) == want and dev_set.count() == len(want), name
        probe = [b["hash"] for b in blocks[:64]] + [ref.bytes_to_hash(b["parent"]) for b in blocks[:64]]
        assert list(dev_set.contains(probe)) == [h in want for h in probe], name
    if n >= 63:
        assert classes == {(0, 0), (1, 0), (1, 1)}


# ---- 2: the set alone -----------------------------------------------------------------------------------------
def homed(rng, home, tag):
    return bytes([home]) + rng.bytes(23) + tag.to_bytes(8, "little")


@pytest.mark.parametrize("form", ["device", "host"])
def test_the_set_against_a_python_set(form):
    import torch

    rng = np.random.default_rng(7)
    dev = lambda hs: torch.from_numpy(np.frombuffer(b"".join(hs), np.uint8).reshape(-1, 32).copy()).cuda()  # noqa: E731
    put = (lambda s, hs, take=None: s.insert(dev(hs), None if take is None else torch.from_numpy(take).cuda())) if form == "device" \
        else (lambda s, hs, take=None: s.insert(hs, take))
    has = (lambda s, hs: list(s.contains(dev(hs)).cpu().numpy() != 0)) if form == "device" else (lambda s, hs: list(s.contains(hs)))
    s = DeviceSavedBlocks(min_keys=1)  # 8 cells
    assert s.count() == 0 and s.hashes() == []
    keys = [homed(rng, 6, k) for k in range(4)] + [bytes(32)]  # four keys of home cell 6 (the probes wrap) and the zero hash
    want = set()
    assert has(s, keys) == [False] * 5
    put(s, keys[:3])
    want |= set(keys[:3])
    assert s.count() == 3 and set(s.hashes()) == want and has(s, keys) == [True, True, True, False, False]
    put(s, [keys[1], keys[3], keys[3], keys[4], keys[1], keys[4]])  # old and new, each new one twice: the count rises once each
    want |= set(keys)
    assert s.count() == 5 and set(s.hashes()) == want and has(s, keys) == [True] * 5
    take = np.array([1, 0, 1, 0], np.uint8)
    more = [homed(rng, 6, 10 + k) for k in range(4)]
    put(s, more, take)
    want |= {more[0], more[2]}
    assert s.count() == 7 and set(s.hashes()) == want and has(s, more) == [True, False, True, False]
    s.reserve(2048, device_form=form == "device")  # 8 (or the 16 the inserts reserved) -> 4,096 cells, rehashed on the device
    assert s.count() == 7 and set(s.hashes()) == want and has(s, keys + more) == [True] * 5 + [True, False, True, False]
    s.reserve(100, device_form=form == "device")  # no-op
    big = [rng.bytes(32) for _ in range(3000)]  # past 1,024: several tiles in one insert, and a reserve inside it
    put(s, big + big[:100])
    want |= set(big)
    assert s.count() == len(want) and set(s.hashes()) == want
    assert has(s, big[:50] + [rng.bytes(32)]) == [True] * 50 + [False]
    seeded = DeviceSavedBlocks(big[:2000] + big[:10], min_keys=1)  # Chain.reload's set, duplicates once
    assert seeded.count() == 2000 and set(seeded.hashes()) == set(big[:2000])


def test_a_full_table_sets_the_capacity_bit_and_never_spins():
    """Eight keys fill the eight cells through the raw device entry (no reserve); a lookup of an
    absent key walks all eight and ends; the ninth key finds no cell: the sticky PZ_ERANGE, the eight
    stay.  A reserve and the ninth key fits."""
    import torch

    rng = np.random.default_rng(8)
    s = DeviceSavedBlocks(min_keys=1)
    keys = [homed(rng, 5, k) for k in range(9)]
    d = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()).cuda()
    _lib.lib.call("pz_dev_block_set_insert", s._h, d.data_ptr(), None, 8, _lib.stream_ptr(0))
    assert s.count() == 8 and list(s.contains(keys)) == [True] * 8 + [False]
    _lib.lib.call("pz_dev_block_set_insert", s._h, d[256:].data_ptr(), None, 1, _lib.stream_ptr(0))
    with pytest.raises(_lib.PzError) as e:
        s.count()
    assert e.value.code == _lib.PZ_ERANGE
    assert s.count(strict=False) == 8 and set(s.hashes(strict=False)) == set(keys[:8])
    s.reserve(9)
    s.insert(keys[8:])
    assert s.count(strict=False) == 9 and list(s.contains(keys)) == [True] * 9


# ---- 3: one run, one call, no mask ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain130():
    return late_chain(1024, 130, seed=4)


def chain130():
    return copy.deepcopy(_chain130())


def block_hash(b):
    return hashlib.blake2b(wire.beacon_block(b), digest_size=64).digest()[:32]  # (input generation only)


WALK_OF = {"processed": bc.WALK_CANDIDATE, "saved_not_candidate": bc.WALK_SAVED, "attestations_rejected": bc.WALK_OFF,
           "no_parent": bc.WALK_OFF}


def against_the_oracle(blocks, want_statuses=None):
    """One walk_serialized_blocks_saved call over ``blocks`` from genesis against the oracle stepped
    block by block: statuses (no_parent included), walk codes, cache, pool, ring and the saved set."""
    nval = 1024
    data, offs = bc.serialize_blocks(blocks)
    chain, cache, pool, ring, tab, balance = genesis_objects(nval)
    saved = DeviceSavedBlocks()
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks]
    assert not any(r["transition"] for r in recs)
    if want_statuses is not None:
        assert [r["status"] for r in recs] == want_statuses  # (CPU: the input is the case it claims to be)
    out = bc.walk_serialized_blocks_saved(cache, pool, ring, saved, data, offs, 0, 0, tab, balance, want_digests=True)
    assert list(out["parent_ok"]) == [int(r["status"] != "no_parent") for r in recs]
    assert list(out["walk"]) == [WALK_OF[r["status"]] for r in recs]
    assert [h.tobytes() for h in out["block_hash"]] == [r["hash"] for r in recs]
    check_against(chain, cache, pool, ring)
    check_digests(out, recs)
    assert set(saved.hashes()) == chain.saved and saved._count == len(chain.saved)
    return out, recs, chain


def test_a_cycle_of_blocks_in_one_call_without_a_mask():
    blocks = chain130()[:63]
    out, recs, chain = against_the_oracle(blocks, ["processed"] * 63)
    assert out["ncand"] == 63 and out["stop"] == 63 and len(chain.saved) == 63
    # every output equals the existing all-eligible call's
    data, offs = bc.serialize_blocks(blocks)
    _, cache, pool, ring, tab, balance = genesis_objects(1024)
    old = bc.walk_serialized_blocks(cache, pool, ring, data, offs, 0, 0, tab, balance, want_digests=True)
    assert "parent_ok" not in old and set(out) == set(old) | {"parent_ok"}
    for k, v in old.items():
        np.testing.assert_array_equal(np.asarray(out[k]), np.asarray(v), k)


# ---- 4: the run out of order ------------------------------------------------------------------------------------
def test_a_removed_block_refuses_everything_after_it():
    blocks = chain130()[:63]
    del blocks[20]
    against_the_oracle(blocks, ["processed"] * 20 + ["no_parent"] * 42)


def test_two_swapped_blocks():
    blocks = chain130()[:63]
    blocks[30], blocks[31] = blocks[31], blocks[30]
    against_the_oracle(blocks, ["processed"] * 30 + ["no_parent", "processed"] + ["no_parent"] * 31)


def test_a_late_block_and_a_second_delivery():
    blocks = chain130()[:63]
    blocks = blocks[:10] + [blocks[11], blocks[10], blocks[11]] + blocks[12:]
    out, recs, _ = against_the_oracle(blocks, ["processed"] * 10 + ["no_parent"] + ["processed"] * 53)
    assert recs[10]["hash"] == recs[12]["hash"]  # one block, refused and then saved


def test_a_block_whose_last_attestation_fails_and_its_child():
    blocks = chain130()[:63]
    good = blocks[40].attestations[-1]
    blocks[40].attestations = list(blocks[40].attestations) + [pb.AttestationRecord(
        slot=good.slot, shard_id=good.shard_id, justified_slot=9, attester_bitfield=bytes(good.attester_bitfield),
        oblique_parent_hashes=[bytes(h) for h in good.oblique_parent_hashes])]
    for j in range(41, 63):  # the chain goes on from the block as it now is
        blocks[j].parent_hash = block_hash(blocks[j - 1])
    against_the_oracle(blocks, ["processed"] * 40 + ["attestations_rejected"] + ["no_parent"] * 22)


# ---- 5: siblings, refusals and an ineligible block -----------------------------------------------------------------
def test_siblings_with_the_set_seeded_instead_of_a_mask():
    """The run of test_siblings_refusals_and_an_ineligible_block_in_one_run: the set holds the eligible
    blocks' parents, so the device's parent check gives what the mask gave."""
    rng = np.random.default_rng(10)
    nval = 1024
    chain, cache, pool, ring, tab, balance = genesis_objects(nval)

    def rec8(slot, j, good=True):
        shard, comm = tab[slot][j % len(tab[slot])]
        bits = rng.random(len(comm)) < 0.6
        return pb.AttestationRecord(slot=slot, shard_id=shard, justified_slot=0 if good else 9,
                                    attester_bitfield=np.packbits(bits.astype(np.uint8)).tobytes(),
                                    oblique_parent_hashes=[rng.bytes(33)])

    def block(slot, atts):
        return pb.BeaconBlock(parent_hash=rng.bytes(32), slot_number=slot, timestamp=pb.Timestamp(8 * slot, 0), attestations=atts)

    blocks = [block(5, [rec8(1, 0), rec8(2, 1)]), block(5, [rec8(2, 0)]), block(6, [rec8(3, 0, good=False), rec8(3, 1)]),
              block(7, [rec8(1, 0), rec8(2, 0, good=False)]), block(8, [rec8(1, 1)]), block(9, [rec8(4, 0), rec8(1, 1)]),
              block(9, [rec8(2, 1)])]
    eligible = [1, 1, 1, 1, 0, 1, 1]
    parents = [ref.copy32(b.parent_hash) for b, e in zip(blocks, eligible) if e]
    chain.saved |= set(parents)
    saved = DeviceSavedBlocks(parents)
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in blocks]
    assert [r["status"] for r in recs] == ["processed", "saved_not_candidate", "processed", "attestations_rejected", "no_parent",
                                          "processed", "saved_not_candidate"]
    data, offs = bc.serialize_blocks(blocks)
    out = bc.walk_serialized_blocks_saved(cache, pool, ring, saved, data, offs, 0, 0, tab, balance, want_digests=True)
    assert list(out["walk"]) == [2, 1, 2, 0, 0, 2, 1] and list(out["report"]) == [1, 1, 2, 0, 0, 1, 1]
    assert list(out["parent_ok"]) == eligible
    assert (out["stop"], out["ncand"], out["has_candidate"], out["candidate_slot"]) == (7, 3, True, 9)
    first = out["att_first"]
    base = [int(out["parents_start"][int(first[j])]) - (blocks[j].slot_number - blocks[j].attestations[0].slot) for j in range(7)]
    assert base == [1, 2, 2, 3, 3, 3, 4]
    check_against(chain, cache, pool, ring)
    check_digests(out, recs)
    assert set(saved.hashes()) == chain.saved
    # CanProcessBlock as a mask beside the set: block 5 refused by the caller, so its sibling's slot wins nothing new
    _, cache2, pool2, ring2, _, _ = genesis_objects(nval)
    out2 = bc.walk_serialized_blocks_saved(cache2, pool2, ring2, DeviceSavedBlocks(parents), data, offs, 0, 0, tab, balance,
                                           eligible=[1, 1, 1, 1, 1, 0, 1])
    assert list(out2["parent_ok"]) == eligible and list(out2["walk"]) == [2, 1, 2, 0, 0, 0, 2]


# ---- 6: across both transitions ------------------------------------------------------------------------------------
def test_the_chain_across_both_transitions_with_the_set():
    """test_the_chain_across_both_transitions with no mask: five calls, the transition block checked
    with ``saved.contains`` and stored with ``saved.insert``."""
    from test_state_wire_gpu import check_states, genesis_resident

    nval, nblocks = 1024, 130
    blocks = chain130()
    data, offs = bc.serialize_blocks(blocks)
    chain, cache, pool, ring, _, _ = genesis_objects(nval)
    saved = DeviceSavedBlocks()
    state, _ = genesis_resident(chain.C)

    def span(lo, hi):
        return data[int(offs[lo]):int(offs[hi])], (offs[lo:hi + 1] - offs[lo]).astype(U64)

    def scalars():
        return (state.last_justified_slot, state.last_state_recalc, table(chain.C), state.balances().copy())

    i, has, cslot, lag, pre = 0, False, 0, 0, None
    calls, stops = [], []
    while i < nblocks:
        ljs, lsr, tab, balance = pre if lag else scalars()
        d, o = span(i, nblocks)
        out = bc.walk_serialized_blocks_saved(cache, pool, ring, saved, d, o, ljs, lsr, tab, balance, has_candidate=has,
                                              candidate_slot=cslot, lag=lag)
        stop = out["stop"]
        calls.append((i, stop, lag))
        assert stop >= 1 and (out["walk"][:stop] == bc.WALK_CANDIDATE).all() and (out["walk"][stop:] == bc.WALK_DEFERRED).all()
        assert out["parent_ok"].all()  # (a deferred block's parent counts the blocks before it as saved)
        for b in blocks[i:i + stop]:
            r = chain.process_block(oreplay.to_pb_block(b))
            assert r["status"] == "processed" and not r["transition"]
        i, has, cslot = i + stop, out["has_candidate"], out["candidate_slot"]
        assert saved._count == len(chain.saved) == i
        if lag:
            lag = 0
            continue
        if i == nblocks:
            break
        blk_ = blocks[i]  # a cycle transition: the existing pieces, in the reference's order
        stops.append(blk_.slot_number)
        ljs, lsr, tab, balance = pre = scalars()
        assert list(saved.contains([ref.copy32(blk_.parent_hash)])) == [True]  # service.go:261-269
        d, o = span(i, i + 1)
        report, _, _ = bc.tally_serialized_blocks(cache, d, o, ljs, lsr, 128, tab, ring.read()[0], balance, tally_mixed=True)
        assert list(report) == [bc.BLOCK_TALLIED]
        saved.insert(out["block_hash"][stop:stop + 1])  # service.go:324
        bc.state_recalc_resident(pool, cache, state, ring, blk_.slot_number)
        bc.pend_serialized_blocks(pool, d, o, ljs, lsr, 128, tab, candidate=[1])
        ring.append(out["block_hash"][stop:stop + 1])
        r = chain.process_block(oreplay.to_pb_block(blk_))
        assert r["status"] == "processed" and r["transition"]
        i, has, cslot, lag = i + 1, True, blk_.slot_number, 1
    assert stops == [64, 128] and calls == [(0, 63, 0), (64, 1, 1), (65, 62, 0), (128, 1, 1), (129, 1, 0)]
    check_against(chain, cache, pool, ring)
    assert set(saved.hashes()) == chain.saved and saved.count() == 130
    _, A, C = chain.candidate
    assert tuple(getattr(state, k) for k in state._SCALARS) == tuple(getattr(C, k) for k in state._SCALARS)
    assert [(r.dynasty, r.slot, bytes(r.blockhash)) for r in state.crosslink_records] == \
        [(r.dynasty, r.slot, bytes(r.blockhash)) for r in C.crosslink_records]
    np.testing.assert_array_equal(state.balances(), np.array([v.balance for v in C.validators], U64))
    check_states(pool, state, A.data, C)
    rest = (C.crosslinking_start_shard, bytes(C.dynasty_seed), C.dynasty_seed_last_reset)
    assert bc.resident_state_roots(pool, state, ring, wire.committees_device(table(C)), None, *rest) == \
        (ref.active_state_hash(A.data), ref.crystallized_state_hash(C))


# ---- 7: a panic row in the run ----------------------------------------------------------------------------------
def test_a_panic_row_leaves_the_set_too():
    """The run of test_a_panic_row_leaves_cache_pool_and_ring with the set: ChainPanic, and set, cache,
    pool and ring equal a twin's that never saw the call."""
    nval = 1024
    blocks = chain130()[:8]
    _, cache, pool, ring, tab, balance = genesis_objects(nval)
    _, twin_cache, twin_pool, twin_ring, _, _ = genesis_objects(nval)
    saved, twin_saved = DeviceSavedBlocks(min_keys=1), DeviceSavedBlocks(min_keys=1)
    data, offs = bc.serialize_blocks(blocks[:3])
    for objs in ((cache, pool, ring, saved), (twin_cache, twin_pool, twin_ring, twin_saved)):
        out = bc.walk_serialized_blocks_saved(*objs, data, offs, 0, 0, tab, balance)
        assert out["ncand"] == 3
    good = blocks[5].attestations[-1]
    bad = pb.AttestationRecord(slot=blocks[5].slot_number + 70, shard_id=good.shard_id, justified_slot=good.justified_slot,
                               attester_bitfield=bytes(good.attester_bitfield),
                               oblique_parent_hashes=[bytes(h) for h in good.oblique_parent_hashes])
    blocks[5].attestations = [bad] + list(blocks[5].attestations)  # refused (slot too high), then re-derived: start > end
    data, offs = bc.serialize_blocks(blocks[3:8])
    with pytest.raises(bc.ChainPanic):
        bc.walk_serialized_blocks_saved(cache, pool, ring, saved, data, offs, 0, 0, tab, balance, has_candidate=True, candidate_slot=3)
    assert set(saved.hashes()) == set(twin_saved.hashes()) and saved.count() == 3
    assert snapshot(cache) == snapshot(twin_cache) and cache.items()
    assert pool.records() == twin_pool.records() and len(pool)
    for a, b in zip(ring.read(history=True), twin_ring.read(history=True)):
        np.testing.assert_array_equal(a, b)
    # and the set still works: the good blocks land as on the twin's side
    data, offs = bc.serialize_blocks(blocks[3:5])
    for objs in ((cache, pool, ring, saved), (twin_cache, twin_pool, twin_ring, twin_saved)):
        out = bc.walk_serialized_blocks_saved(*objs, data, offs, 0, 0, tab, balance, has_candidate=True, candidate_slot=3)
        assert out["parent_ok"].all()
    assert set(saved.hashes()) == set(twin_saved.hashes()) and saved.count() == 5
    assert ring.hashes() == twin_ring.hashes() and snapshot(cache) == snapshot(twin_cache)
