"""The attestation store batch on the GPU (prysm_amd/csrc/blockstore.hip; ResidentChain.store):

1. pz_[dev_]block_store_select and pz_[dev_]block_store_digests on synthetic columns, device and host
   forms, against a numpy model of the rule plus hashlib and oracle.ref.attestation_key /
   attestation_hash, with canary bytes behind every output: entries past m and bytes past 34 m stay
   as they were;
2. the case chain (blockstore_cases.py) through ResidentChain.process_all with the store on: the
   database built from blockchain.store_writes equals the model database driven by the oracle's
   records, key for key and byte for byte -- also when the chain is split so that the duplicate block
   arrives in a later call, and over five cycles handed whole;
3. the resubmission path: the store is the landed submission's; a panic before ``stop`` raises and
   returns nothing;
4. the store leaves the rest alone: the same chain with it on and off gives equal outputs, objects,
   calls and resubmits, and with it off the dicts have no "store" key."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import ref
from oracle import replay as oreplay
from prysm_amd import _lib, pb, wire
from prysm_amd import blockchain as bc
from blockstore_cases import ModelDB, case_chain, five_cycles, model_db, oracle_records, saved_rows
from test_attdigest_gpu import to_device
from test_blockcycle_gpu import check_chain, genesis_chain, panic_blocks
from test_blockwalk_gpu import CANARY, padded

pytestmark = pytest.mark.gpu

U64 = np.uint64
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
EINVAL = _lib.PZ_EINVAL


# ---- 1: select and digests on synthetic columns ---------------------------------------------------------
def make(rng, natt, mode, stop_at):
    """``natt`` rows in blocks of 0-4 rows, with blocks of no rows at the front, in the middle and at
    the end.  mode "random": every status drawn; "all": every row saved; "none": no parent anywhere.
    ``stop_at``: "whole" (a NULL stop), "end" (the word holds nblocks), "inside" (the block of a row
    two thirds in: inside a tile), "zero"."""
    counts, left = [0], natt
    while left:
        k = min(left, int(rng.integers(0, 5)))
        counts.append(k)
        left -= k
    counts.insert(len(counts) // 2, 0)
    counts.append(0)
    nb = len(counts)
    att_block = np.repeat(np.arange(nb, dtype=np.uint32), counts)
    att_first = np.concatenate([[0], np.cumsum(counts)]).astype(U64)
    if mode == "random":
        att_status = rng.choice(np.array([0, 0, 0, 0, 1, 2, 4, 6, EINVAL], np.int32), size=natt)
        block_status = rng.choice(np.array([0, 0, 0, 0, 0, EINVAL], np.int32), size=nb)
        parent_ok = (rng.integers(0, 5, size=nb) != 0).astype(np.uint8)
    else:
        att_status, block_status = np.zeros(natt, np.int32), np.zeros(nb, np.int32)
        parent_ok = np.full(nb, 1 if mode == "all" else 0, np.uint8)
    rec_status = np.where(att_status == EINVAL, EINVAL, 0).astype(np.int32)
    block_status[att_block[rec_status != 0]] = EINVAL  # folded: a bad record refuses its block
    stop = {"whole": None, "end": nb, "inside": int(att_block[2 * natt // 3]) if natt else 0, "zero": 0}[stop_at]
    # the records: ShardBlockHash of 0, 31, 32, 33 bytes, 0, 1 or 64 oblique hashes of 0-33 bytes, and
    # their encodings with gaps between them
    atts, spans, chunks, at = [], [], [], 0
    for r in range(natt):
        n_obl = 64 if r % 97 == 5 else int(rng.integers(0, 2))
        a = pb.AttestationRecord(slot=int(rng.integers(0, 1 << 40)), shard_id=int(rng.integers(0, 1 << 20)), justified_slot=r,
                                 justified_block_hash=rng.bytes(32), shard_block_hash=rng.bytes((0, 31, 32, 33)[r % 4]),
                                 attester_bitfield=rng.bytes(int(rng.integers(0, 5))),
                                 oblique_parent_hashes=[rng.bytes(int(rng.integers(0, 34))) for _ in range(n_obl)],
                                 aggregate_sig=[int(rng.integers(0, 1 << 62))] * int(rng.integers(0, 3)))
        enc, gap = wire.attestation_record(a), int(rng.integers(0, 7))
        chunks += [b"\xCC" * gap, enc]
        spans.append((at + gap, at + gap + len(enc)))
        at += gap + len(enc)
        atts.append(a)
    spans = np.array(spans, U64).reshape(natt, 2)
    return {"nb": nb, "natt": natt, "att_block": att_block, "att_first": att_first, "att_status": att_status, "rec_status": rec_status,
            "block_status": block_status, "parent_ok": parent_ok, "stop": stop, "atts": atts, "bytes": np.frombuffer(b"".join(chunks), np.uint8),
            "att_beg": np.ascontiguousarray(spans[:, 0]), "att_end": np.ascontiguousarray(spans[:, 1])}


def model(r):
    nb, natt = r["nb"], r["natt"]
    stop = nb if r["stop"] is None else r["stop"]
    b = r["att_block"].astype(np.int64)
    flag = (b < stop) & (r["block_status"][b] == 0) & (r["parent_ok"][b] != 0) & (r["att_status"] == 0) & (r["rec_status"] == 0)
    rows = np.nonzero(flag)[0].astype(np.uint32)
    rank = np.concatenate([[0], np.cumsum(flag)]).astype(U64)
    oatts = oreplay.to_pb_block(pb.BeaconBlock(attestations=[r["atts"][i] for i in rows])).attestations
    key = [ref.attestation_key(a) for a in oatts]
    hash_ = [ref.attestation_hash(a) for a in oatts]
    data = r["bytes"].tobytes()
    for i, h in zip(rows, hash_):  # Attestation.Hash is the hash of the bytes where they lie
        assert h == hashlib.blake2b(data[int(r["att_beg"][i]):int(r["att_end"][i])], digest_size=64).digest()[:32]
    return {"m": len(rows), "rows": rows, "first": rank[r["att_first"].astype(np.int64)] if natt else np.zeros(nb + 1, U64),
            "span": np.stack([r["att_beg"][rows], r["att_end"][rows]], axis=1).reshape(-1, 2),
            "key": np.frombuffer(b"".join(key), np.uint8).reshape(-1, 32), "hash": np.frombuffer(b"".join(hash_), np.uint8).reshape(-1, 32),
            "lists": np.frombuffer(b"".join(b"\x0a\x20" + h for h in hash_), np.uint8)}


def check(got, want, name):
    m = want["m"]
    assert got["m"] == m, name
    for k in ("rows", "first", "span", "key", "hash", "lists"):
        np.testing.assert_array_equal(got[k], want[k], "%s: %s" % (name, k))


def run_device(r, with_rec):
    import torch

    nb, natt = r["nb"], r["natt"]
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    ins = {k: put(r[k]) for k in ("att_first", "block_status", "parent_ok", "att_block", "att_status", "rec_status", "att_beg", "att_end")}
    stop = None if r["stop"] is None else put(np.array([r["stop"]], U64))
    outs = {"rows": padded(np.full(natt, 0xA5A5A5A5, np.uint32)), "span": padded(np.full(2 * natt, 0xA5A5A5A5A5A5A5A5, U64)),
            "first": padded(np.full(nb + 1, 0xA5A5A5A5A5A5A5A5, U64)), "count": padded(np.full(1, 0xA5A5A5A5A5A5A5A5, U64))}
    scratch = torch.empty(int(_lib.lib.dll.pz_block_store_scratch_bytes(nb, natt)), dtype=torch.uint8, device="cuda")
    p = _lib.dptr
    b = _lib.BlockStoreBatch(nblocks=nb, att_first=p(ins["att_first"]), block_status=p(ins["block_status"]), parent_ok=p(ins["parent_ok"]),
                             stop=p(stop), natt=natt, att_block=p(ins["att_block"]), att_status=p(ins["att_status"]),
                             rec_status=p(ins["rec_status"]) if with_rec else None, att_beg=p(ins["att_beg"]), att_end=p(ins["att_end"]),
                             **{k: t.data_ptr() for k, (t, _) in outs.items()})
    _lib.lib.call("pz_dev_block_store_select", ctypes.byref(b), scratch.data_ptr(), _lib.stream_ptr(0))
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, (t, _) in outs.items()}
    for k, (_, used) in outs.items():
        assert (host[k][used:] == CANARY).all(), k  # nothing is written behind an output
    if natt == 0:  # nothing is launched: every output stays as it was
        assert all((h == CANARY).all() for h in host.values())
        return {"m": 0, "rows": np.zeros(0, np.uint32), "first": np.zeros(nb + 1, U64), "span": np.zeros((0, 2), U64),
                "key": np.zeros((0, 32), np.uint8), "hash": np.zeros((0, 32), np.uint8), "lists": np.zeros(0, np.uint8)}
    m = int(host["count"][:8].view(U64)[0])
    assert m <= natt
    assert (host["rows"][4 * m:] == CANARY).all() and (host["span"][16 * m:] == CANARY).all()  # entries past m stay untouched
    got = {"m": m, "rows": host["rows"][:4 * m].view(np.uint32), "first": host["first"][:8 * (nb + 1)].view(U64),
           "span": host["span"][:16 * m].view(U64).reshape(m, 2)}
    # digests over the rows select left where they lie; bytes with the 4 readable bytes of the contract
    cols = to_device(wire.attestation_columns(r["atts"]))
    d_bytes = put(np.concatenate([r["bytes"], np.full(4, 0x5C, np.uint8)]))
    douts = {"key": padded(np.full(32 * m, CANARY, np.uint8)), "hash": padded(np.full(32 * m, CANARY, np.uint8)),
             "lists": padded(np.full(34 * m, CANARY, np.uint8))}
    b = _lib.BlockStoreBatch(natt=natt, rows=outs["rows"][0].data_ptr(), span=outs["span"][0].data_ptr(), bytes=d_bytes.data_ptr(),
                             **{k: t.data_ptr() for k, (t, _) in douts.items()})
    c = _lib.att_cols(cols)
    _lib.lib.call("pz_dev_block_store_digests", ctypes.byref(b), ctypes.byref(c), m, _lib.stream_ptr(0))
    torch.cuda.synchronize()
    for k, (t, used) in douts.items():
        h = t.cpu().numpy()
        assert (h[used:] == CANARY).all(), k  # bytes past 34 m (and past 32 m) stay untouched
        got[k] = h[:used].reshape(-1, 32) if k != "lists" else h[:used]
    return got


def run_host(r, with_rec):
    nb, natt = r["nb"], r["natt"]
    tail = np.full(64, CANARY, np.uint8)
    whole = {"rows": np.concatenate([np.full(4 * natt, CANARY, np.uint8), tail]), "span": np.concatenate([np.full(16 * natt, CANARY, np.uint8), tail]),
             "first": np.concatenate([np.full(8 * (nb + 1), CANARY, np.uint8), tail]), "count": np.concatenate([np.full(8, CANARY, np.uint8), tail])}
    hp = _lib.ptr
    stop = None if r["stop"] is None else np.array([r["stop"]], U64)
    b = _lib.BlockStoreBatch(nblocks=nb, att_first=hp(r["att_first"]), block_status=hp(r["block_status"]), parent_ok=hp(r["parent_ok"]),
                             stop=hp(stop), natt=natt, att_block=hp(r["att_block"]), att_status=hp(r["att_status"]),
                             rec_status=hp(r["rec_status"]) if with_rec else None, att_beg=hp(r["att_beg"]), att_end=hp(r["att_end"]),
                             **{k: w.ctypes.data for k, w in whole.items()})
    _lib.lib.call("pz_block_store_select", ctypes.byref(b))
    m = int(whole["count"][:8].view(U64)[0])
    assert m <= natt and (whole["count"][8:] == CANARY).all() and (whole["first"][8 * (nb + 1):] == CANARY).all()
    assert (whole["rows"][4 * m:] == CANARY).all() and (whole["span"][16 * m:] == CANARY).all()  # entries past m stay untouched
    got = {"m": m, "rows": whole["rows"][:4 * m].view(np.uint32).copy(), "first": whole["first"][:8 * (nb + 1)].view(U64).copy(),
           "span": whole["span"][:16 * m].view(U64).reshape(m, 2).copy()}
    cols = wire.attestation_columns(r["atts"])
    dw = {"key": np.concatenate([np.full(32 * m, CANARY, np.uint8), tail]), "hash": np.concatenate([np.full(32 * m, CANARY, np.uint8), tail]),
          "lists": np.concatenate([np.full(34 * m, CANARY, np.uint8), tail])}
    b = _lib.BlockStoreBatch(natt=natt, rows=hp(got["rows"]), span=hp(got["span"]), bytes=hp(r["bytes"]), nbytes=r["bytes"].size,
                             **{k: w.ctypes.data for k, w in dw.items()})
    c = _lib.att_cols(cols)
    _lib.lib.call("pz_block_store_digests", ctypes.byref(b), ctypes.byref(c), m)
    for k, size in (("key", 32 * m), ("hash", 32 * m), ("lists", 34 * m)):
        assert (dw[k][size:] == CANARY).all(), k
        got[k] = dw[k][:size].reshape(-1, 32).copy() if k != "lists" else dw[k][:size].copy()
    return got


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("natt", SIZES)
def test_select_and_digests_on_synthetic_columns(natt, form):
    rng = np.random.default_rng(7000 + natt)
    run = run_device if form == "device" else run_host
    seen = set()
    for mode, stop_at, with_rec in [("random", "whole", True), ("random", "inside", False), ("all", "end", True), ("none", "end", True),
                                    ("all", "inside", False), ("random", "zero", True)]:
        r = make(rng, natt, mode, stop_at)
        want = model(r)
        check(run(r, with_rec), want, "%s, stop %s" % (mode, stop_at))
        if mode == "all" and stop_at == "end":
            assert want["m"] == natt
        if mode == "none" or stop_at == "zero":
            assert want["m"] == 0
        if stop_at == "inside" and natt >= 257:  # the stop falls inside a tile, with saved rows on both sides of it in the run
            edge = int(r["att_first"][r["stop"]])
            assert edge % 256 != 0 and 0 < want["m"] and edge < natt
        seen.add(0 < want["m"] < natt)
        counts = np.diff(r["att_first"].astype(np.int64))
        assert counts[0] == 0 and counts[-1] == 0 and (counts[1:-1] == 0).any()  # blocks of no rows at the front, inside and at the end
    if natt >= 63:
        assert True in seen  # some run saves a part of its rows


def test_the_row_list_is_checked_on_the_device():
    """A list entry that names no row gets a zero key and reads nothing; the rows around it are right."""
    import torch

    rng = np.random.default_rng(11)
    r = make(rng, 5, "all", "end")
    want = model(r)
    cols = to_device(wire.attestation_columns(r["atts"]))
    rows = torch.tensor([0, 4, 5, 1 << 30, 2], dtype=torch.int32, device="cuda")
    span = torch.from_numpy(np.stack([r["att_beg"], r["att_end"]], axis=1).astype(np.int64)).cuda()
    d_bytes = torch.from_numpy(np.concatenate([r["bytes"], np.zeros(4, np.uint8)])).cuda()
    key, hash_, lists = (torch.zeros(n, dtype=torch.uint8, device="cuda") for n in (160, 160, 172))
    b = _lib.BlockStoreBatch(natt=5, rows=rows.data_ptr(), span=span.data_ptr(), bytes=d_bytes.data_ptr(), key=key.data_ptr(),
                             hash=hash_.data_ptr(), lists=lists.data_ptr())
    c = _lib.att_cols(cols)
    _lib.lib.call("pz_dev_block_store_digests", ctypes.byref(b), ctypes.byref(c), 5, _lib.stream_ptr(0))
    got = key.cpu().numpy().reshape(5, 32)
    np.testing.assert_array_equal(got[[0, 1, 4]], want["key"][[0, 4, 2]])
    assert not got[2:4].any()


# ---- 2: the case chain through process_all -------------------------------------------------------------------
def store_db(outs, data, offs):
    """The database the calls' store_writes build, each call over its own bytes."""
    db = ModelDB()
    for out in outs:
        lo = int(offs[out["start"]])
        db.apply_writes(bc.store_writes(out, data[lo:]))
    return db


def check_store_shape(out, saved):
    """``first`` against the oracle's per-block counts of the blocks the call processed."""
    st, lo, stop = out["store"], out["start"], out["stop"]
    assert list(np.diff(st["first"].astype(np.int64))[:stop]) == saved[lo:lo + stop]
    assert (st["first"][stop:] == st["first"][stop]).all() and len(st["first"]) == len(out["walk"]) + 1  # deferred blocks save nothing yet
    m = int(st["first"][-1])
    assert st["rows"].shape == (m,) and st["span"].shape == (m, 2) and st["key"].shape == (m, 32) and st["lists"].shape == (34 * m,)
    assert (np.diff(st["rows"].astype(np.int64)) > 0).all()


def test_the_case_chain_gives_the_model_database():
    blocks, eligible, at = case_chain()
    recs, chain = oracle_records(blocks, eligible)
    want = model_db(blocks, recs).data
    saved = saved_rows(recs)
    data, offs = bc.serialize_blocks(blocks)
    _, rc = genesis_chain(1024)
    rc.store = True
    outs = rc.process_all(data, offs, eligible=eligible, want_digests=True)
    assert [o["start"] for o in outs][:2] == [0, at["chain 64"] + 1] and len(outs) >= 2
    for out in outs:
        check_store_shape(out, saved)
    # the ineligible block saves its row while want_digests gives it no message
    first = outs[0]["store"]["first"]
    j = at["ineligible"]
    assert first[j + 1] - first[j] == 1 and not outs[0]["msg"][int(outs[0]["att_first"][j]):int(outs[0]["att_first"][j + 1])].any()
    got = store_db(outs, data, offs).data
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], k
    check_chain(chain, rc)
    # the same chain split so that the duplicate block arrives in a later call
    _, rc2 = genesis_chain(1024)
    rc2.store = True
    cut = at["twice"]
    outs2 = rc2.process_all(data[:int(offs[cut])], offs[:cut + 1], eligible=eligible[:cut])
    tail = rc2.process_all(data[int(offs[cut]):], offs[cut:] - offs[cut], eligible=eligible[cut:])
    for o in tail:
        o["start"] += cut
    got2 = store_db(outs2 + tail, data, offs).data
    assert got2 == want
    check_chain(chain, rc2)


def test_five_cycles_handed_whole_give_the_model_database():
    """synth.chain_blocks(1024, 330): six calls, at least one of them submitted twice; every store is
    the landed submission's."""
    blocks = five_cycles()
    recs, chain = oracle_records(blocks)
    want = model_db(blocks, recs).data
    data, offs = bc.serialize_blocks(blocks)
    _, rc = genesis_chain(1024)
    rc.store = True
    outs = rc.process_all(data, offs)
    assert rc.resubmits >= 1 and len(outs) == 6
    saved = saved_rows(recs)
    for out in outs:
        check_store_shape(out, saved)
    assert store_db(outs, data, offs).data == want
    check_chain(chain, rc)


# ---- 3: the resubmission path -----------------------------------------------------------------------------------
def test_the_store_is_the_landed_submissions():
    blocks = panic_blocks(67)  # the panic row sits past the stop at 65: the run is submitted again without it
    recs, _ = oracle_records(blocks[:65])
    want = model_db(blocks[:65], recs).data
    data, offs = bc.serialize_blocks(blocks)
    _, rc = genesis_chain(1024)
    rc.store = True
    out = rc.process_serialized(data, offs)
    assert (out["stop"], rc.resubmits, rc.calls) == (65, 1, 2)
    out["start"] = 0
    check_store_shape(out, saved_rows(recs) + [0] * 5)
    assert store_db([out], data, offs).data == want and len(want) == 2 * 65


@pytest.mark.parametrize("at", [40, 64])
def test_a_panic_before_stop_returns_nothing(at):
    blocks = panic_blocks(at)
    data, offs = bc.serialize_blocks(blocks)
    _, rc = genesis_chain(1024)
    rc.store = True
    with pytest.raises(bc.ChainPanic):
        rc.process_serialized(data, offs)
    assert not rc.spent and not rc.has_candidate  # nothing landed, and the object still works
    d, o = bc.serialize_blocks(blocks[:at])
    out = rc.process_serialized(d, o)
    assert out["stop"] == at and int(out["store"]["first"][-1]) == at


# ---- 4: the store leaves the rest alone -------------------------------------------------------------------------
def test_the_store_leaves_the_rest_alone():
    blocks, eligible, _ = case_chain()
    recs, chain = oracle_records(blocks, eligible)
    data, offs = bc.serialize_blocks(blocks)
    _, on = genesis_chain(1024)
    _, off = genesis_chain(1024)
    on.store = True
    a = on.process_all(data, offs, eligible=eligible, want_digests=True)
    b = off.process_all(data, offs, eligible=eligible, want_digests=True)
    assert len(a) == len(b) and (on.calls, on.resubmits) == (off.calls, off.resubmits)
    for x, y in zip(a, b):
        assert "store" in x and "store" not in y and set(x) == set(y) | {"store"}
        for k in y:
            np.testing.assert_array_equal(np.asarray(x[k]), np.asarray(y[k]), k)
    check_chain(chain, on)
    check_chain(chain, off)
    # the switch is read at each call: off again, the next dict has no store
    on.store = False
    d, o = bc.serialize_blocks(blocks[-1:])
    assert "store" not in on.process_serialized(d, o)
