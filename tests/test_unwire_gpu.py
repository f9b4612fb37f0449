"""Device proto3 decoder (prysm_amd/csrc/unwire.hip): AttestationRecords back into the columns
of pz_attestation_cols, and the top level of serialized BeaconBlocks.

What "canonical" means is decided (tests/canon_corpus.py) by Google's protobuf runtime over the
oracle schema (oracle/schema.py), independently of the code under test: a record is canonical
iff it parses, holds no unknown field and serializes back to the same bytes.  Decoded fields are
compared with the runtime's parse of the same bytes, and with the device encoder (wire_att.hip)
both ways."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

from canon_corpus import CANONICAL, CANONICAL_CASES, CORPUS, FRAMED, NONCANONICAL, UNKNOWN_FIELD_BLOCK, canonical
from oracle import ref
from oracle import schema as opb
from prysm_amd import _lib, pb, synth, wire
from prysm_amd.blockchain import check_attestations, check_serialized_blocks, serialize_blocks
from test_attcheck_gpu import random_batch, table
from test_wire import rand_att

pytestmark = pytest.mark.gpu

U64 = np.uint64
TILE = 256  # unwire.hip kTile: records per workgroup
SCAN = 1024  # unwire.hip kScanThreads: tiles per round of the scan kernel
BYTES = (("justified_block_hash", "justified_block_hash_offs"), ("shard_block_hash", "shard_block_hash_offs"),
         ("attester_bitfield", "attester_bitfield_offs"), ("oblique_parent_hashes", "oblique_offs"))
RANGES = ("justified_block_hash_offs", "shard_block_hash_offs", "attester_bitfield_offs", "oblique_first",
          "aggregate_sig_first")
PER_RECORD = ("slot", "shard_id", "justified_slot", "n_oblique", "last_byte", "status")


# ---- the oracle ---------------------------------------------------------------------------------
def parse(raw):
    m = opb.AttestationRecord()
    m.ParseFromString(raw)
    return m


def runtime_columns(records):
    """The runtime's parse of bare records, as trimmed pz_attestation_cols columns."""
    return trimmed(wire.attestation_columns([parse(r) for r in records]))


def trimmed(cols):
    """wire.attestation_columns pads its data columns: keep what the offsets cover."""
    c = {k: np.asarray(cols[k]) for k in wire.ATT_COLS}
    for d, o in BYTES:
        c[d] = c[d][:int(c[o][-1])]
    c["aggregate_sig"] = c["aggregate_sig"][:int(c["aggregate_sig_first"][-1])]
    return c


def assert_columns(got, want):
    for k in wire.ATT_COLS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got["n_oblique"], np.diff(got["oblique_first"]))
    bo, bf = got["attester_bitfield_offs"].astype(np.int64), got["attester_bitfield"]
    np.testing.assert_array_equal(got["last_byte"], [bf[e - 1] if e > b else 0 for b, e in zip(bo[:-1], bo[1:])])


def batch(spans):
    offs = np.zeros(len(spans) + 1, dtype=U64)
    offs[1:] = np.cumsum([len(s) for s in spans], dtype=U64)
    return np.frombuffer(b"".join(spans) + bytes(16), dtype=np.uint8), offs


def framed(field_num, rec):
    return wire._msg(field_num, rec) if field_num else rec


@functools.lru_cache(None)
def rand_records(n):
    rng = np.random.default_rng(100 + n)
    return tuple(wire.attestation_record(rand_att(rng)) for _ in range(n))


@functools.lru_cache(None)
def rand_columns(n):
    return runtime_columns(rand_records(n))


# ---- 1. fields against the runtime --------------------------------------------------------------
@pytest.mark.parametrize("field_num", [0, 8, 1, 16, (1 << 29) - 1])
@pytest.mark.parametrize("n", [1, 7, 300, 2000])
def test_fields_match_protobuf_runtime(n, field_num):
    recs = rand_records(n)
    got = wire.unwire_attestations(*batch([framed(field_num, r) for r in recs]), field_num)
    assert not got["status"].any() and got["totals"][6] == 0
    assert_columns(got, rand_columns(n))
    want = rand_columns(n)
    assert list(got["totals"][:6]) == [len(want["justified_block_hash"]), len(want["shard_block_hash"]),
                                       len(want["attester_bitfield"]), len(want["oblique_offs"]) - 1,
                                       len(want["oblique_parent_hashes"]), len(want["aggregate_sig"])]


# ---- 2. inverse of the encoder, both ways -------------------------------------------------------
@pytest.mark.parametrize("n", [TILE + 1, 3 * TILE + 5])
def test_inverse_of_the_encoder(n):
    cols = synth.attestation_columns_512(n, seed=3)
    raw, offs = wire.attestations_device(cols, n, 0)
    got = wire.unwire_attestations(np.frombuffer(raw + bytes(16), dtype=np.uint8), offs)
    assert not got["status"].any()
    assert_columns(got, trimmed(cols))
    recs = synth.attestation_records_512(n, seed=3)
    back = wire.unwire_attestations(recs.reshape(-1), np.arange(n + 1, dtype=U64) * U64(512))
    assert not back["status"].any()
    raw2, offs2 = wire.attestations_device({k: back[k] for k in wire.ATT_COLS}, n, 0)
    assert raw2 == recs.tobytes()
    np.testing.assert_array_equal(offs2, np.arange(n + 1, dtype=U64) * U64(512))


# ---- 3. the non-canonical corpus (tests/canon_corpus.py) ----------------------------------------
NEIGHBOURS = rand_records(7)[:6]


def assert_bad_rows_contribute_nothing(got, bad, rest):
    """``got``: the decode of a batch whose rows ``bad`` failed; ``rest``: the decode of the same
    batch without them."""
    for k in bad:
        assert got["status"][k] == _lib.PZ_EINVAL
        assert not any(got[c][k] for c in PER_RECORD[:5])
        assert all(got[o][k] == got[o][k + 1] for o in RANGES)
    for c in PER_RECORD:
        np.testing.assert_array_equal(np.delete(got[c], bad), rest[c], err_msg=c)
    for o in RANGES:
        np.testing.assert_array_equal(np.delete(np.diff(got[o]), bad), np.diff(rest[o]), err_msg=o)
    for c in ("justified_block_hash", "shard_block_hash", "attester_bitfield", "oblique_parent_hashes",
              "oblique_offs", "aggregate_sig"):
        np.testing.assert_array_equal(got[c], rest[c], err_msg=c)
    np.testing.assert_array_equal(got["totals"][:6], rest["totals"][:6])


@pytest.mark.parametrize("name,field_num", [(k, 0) for k in CORPUS] + [(k, 8) for k in FRAMED])
def test_corpus_case_among_valid_neighbours(name, field_num):
    span = FRAMED[name] if field_num else CORPUS[name]
    ok = canonical(span, opb.BeaconBlock if field_num else opb.AttestationRecord)
    assert ok == (name in CANONICAL_CASES)  # the outcomes recorded in the issue
    good = [framed(field_num, r) for r in NEIGHBOURS]
    rest = wire.unwire_attestations(*batch(good), field_num)
    assert not rest["status"].any()
    for k in (0, 3, len(good)):  # first, inside, last
        got = wire.unwire_attestations(*batch(good[:k] + [span] + good[k:]), field_num)
        want = [_lib.PZ_OK] * (len(good) + 1)
        want[k] = _lib.PZ_OK if ok else _lib.PZ_EINVAL
        assert list(got["status"]) == want
        assert got["totals"][6] == (0 if ok else 1)
        if ok:
            assert_columns(got, runtime_columns(list(NEIGHBOURS[:k]) + [CORPUS[name]] + list(NEIGHBOURS[k:])))
        else:
            assert_bad_rows_contribute_nothing(got, [k], rest)


@pytest.mark.parametrize("field_num", [0, 8])
def test_corpus_across_tiles(field_num):
    """Every case among valid records over five tiles: bad rows in every tile, counted once."""
    cases = FRAMED if field_num else CORPUS
    oracle_cls = opb.BeaconBlock if field_num else opb.AttestationRecord
    spans, good = [], []
    for rep in range(48):
        for j, (name, c) in enumerate(cases.items()):
            spans += [framed(field_num, NEIGHBOURS[(rep + j) % 6]), c]
            good += [True, canonical(c, oracle_cls)]
    assert len(spans) > 4 * TILE
    got = wire.unwire_attestations(*batch(spans), field_num)
    assert list(got["status"] == 0) == good
    bad = [i for i, g in enumerate(good) if not g]
    assert got["totals"][6] == len(bad)
    rest = wire.unwire_attestations(*batch([s for s, g in zip(spans, good) if g]), field_num)
    assert_bad_rows_contribute_nothing(got, bad, rest)


# ---- 4. shapes at the edges ---------------------------------------------------------------------
def test_empty_batch():
    got = wire.unwire_attestations(np.zeros(16, dtype=np.uint8), np.zeros(1, dtype=U64))
    assert all(list(got[o]) == [0] for o in RANGES + ("oblique_offs",))
    assert not got["totals"].any() and all(len(got[c]) == 0 for c in PER_RECORD)


def edge_records():
    rng = np.random.default_rng(4)
    rb = lambda k: rng.integers(0, 256, size=k, dtype=np.uint8).tobytes()  # noqa: E731
    atts = [pb.AttestationRecord(), pb.AttestationRecord(oblique_parent_hashes=[b"", b"", b""]),
            pb.AttestationRecord(slot=1, oblique_parent_hashes=[b"", rb(5), b""], aggregate_sig=[0])]
    for w in range(1, 11):  # every varint width, at its smallest and its largest value
        for v in (1 << (7 * (w - 1)), min((1 << (7 * w)) - 1, (1 << 64) - 1)):
            atts.append(pb.AttestationRecord(slot=v, shard_id=v, justified_slot=v, aggregate_sig=[v, 0, v]))
    atts.append(pb.AttestationRecord(slot=1, oblique_parent_hashes=[rb(40) for _ in range(20)]))  # over 768 bytes
    atts.append(pb.AttestationRecord(attester_bitfield=rb(300)))
    atts.append(pb.AttestationRecord(justified_block_hash=rb(15), shard_block_hash=rb(16), attester_bitfield=rb(17)))
    for nob, nsig in ((13, 16), (14, 17), (150, 200)):  # where the encoder's row path gives way
        atts.append(pb.AttestationRecord(shard_id=2, shard_block_hash=rb(32), oblique_parent_hashes=[rb(int(k)) for k in
                                         rng.integers(0, 40, size=nob)], aggregate_sig=[int(x) for x in
                                         rng.integers(0, 1 << 64, size=nsig, dtype=np.uint64)]))
    return atts


@pytest.mark.parametrize("field_num", [0, 8])
def test_edge_shapes(field_num):
    recs = [wire.attestation_record(a) for a in edge_records()]
    assert {(1 << 63), (1 << 64) - 1} <= {a.slot for a in edge_records()}
    assert max(len(r) for r in recs) > 768 and recs[0] == b""
    got = wire.unwire_attestations(*batch([framed(field_num, r) for r in recs]), field_num)
    assert not got["status"].any()
    assert_columns(got, runtime_columns(recs))


def test_more_tiles_than_one_scan_round():
    """Over 1,024 tiles of tiny records: the scan kernel carries from one round to the next."""
    n = SCAN * TILE + 300
    kinds = (b"", b"\x08\x01", b"\x3a\x00", b"\x42\x01\x05")
    kind = np.arange(n) % 4
    bad = np.arange(n) % 1001 == 7
    spans = [b"\x08\x00" if b else kinds[k] for k, b in zip(kind, bad)]
    got = wire.unwire_attestations(*batch(spans))
    ok = ~bad
    np.testing.assert_array_equal(got["status"], np.where(ok, 0, _lib.PZ_EINVAL))
    np.testing.assert_array_equal(got["slot"], (ok & (kind == 1)).astype(U64))
    for col, k in (("oblique_first", 2), ("aggregate_sig_first", 3)):
        np.testing.assert_array_equal(got[col], np.concatenate([[0], np.cumsum(ok & (kind == k))]).astype(U64))
    np.testing.assert_array_equal(got["aggregate_sig"], np.full(int((ok & (kind == 3)).sum()), 5, dtype=U64))
    assert not got["oblique_offs"].any() and got["totals"][6] == bad.sum()


def to_host(out, n):
    """A device decode (torch tensors at their bounds) as the host form's dict."""
    totals = out["totals"].cpu().numpy().view(U64)
    cols = wire._att_trim({k: out[k] for k in wire.ATT_OUT_COLS}, n, totals)
    host = {k: v.cpu().numpy() for k, v in cols.items()}
    host = {k: v.view(U64) if v.dtype == np.int64 else v for k, v in host.items()}
    host["totals"] = totals
    return host


def device_decode(spans, fill=0):
    """pz_dev_unwire_attestations on a buffer that ends 16 bytes after the last record."""
    import torch

    data, offs = batch(spans)
    buf = torch.full((int(offs[-1]) + 16,), fill, dtype=torch.uint8, device="cuda")
    buf[:int(offs[-1])] = torch.from_numpy(data[:int(offs[-1])].copy()).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    out = wire.unwire_attestations_device(buf, d_offs[:-1], d_offs[1:], len(spans), 0)
    torch.cuda.synchronize()
    return to_host(out, len(spans))


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_last_record_ends_16_bytes_before_the_end_of_the_buffer(fill):
    """The device form on a buffer with exactly the documented pad, whatever the pad holds; the
    last record ends in a bytes field, so its last copy ends at the record's end."""
    recs = list(rand_records(300)) + [wire.attestation_record(pb.AttestationRecord(attester_bitfield=b"\x5a" * 33))]
    got = device_decode(recs, fill)
    assert not got["status"].any()
    assert_columns(got, runtime_columns(recs))


# ---- 5. blocks ----------------------------------------------------------------------------------
BLOCK_FIELDS = ("parent_hash", "randao_reveal", "pow_chain_ref", "active_state_hash", "crystallized_state_hash")


@functools.lru_cache(None)
def chain():
    blocks = synth.chain_blocks(1024, 130)
    return (blocks,) + serialize_blocks(blocks)


def device_blocks(data, offs):
    import torch

    d = torch.from_numpy(np.array(data)).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    return d, wire.unwire_blocks_device(d, d_offs, len(offs) - 1)


def test_blocks_match_the_objects():
    blocks, data, offs = chain()
    got = wire.unwire_blocks(data, offs)
    atts = [a for b in blocks for a in b.attestations]
    assert not got["status"].any() and got["natt"] == len(atts)
    assert list(got["slot_number"]) == [b.slot_number for b in blocks]
    assert list(got["ts_seconds"]) == [b.timestamp.seconds for b in blocks]
    assert list(got["ts_nanos"]) == [b.timestamp.nanos for b in blocks] and got["has_timestamp"].all()
    raw = data.tobytes()
    for i, b in enumerate(blocks):
        for s, f in enumerate(BLOCK_FIELDS):
            beg, ln = int(got["bytes_beg"][i, s]), int(got["bytes_len"][i, s])
            assert raw[beg:beg + ln] == getattr(b, f), (i, f)
    counts = [len(b.attestations) for b in blocks]
    assert list(got["att_first"]) == [0] + list(np.cumsum(counts))
    assert list(got["att_block"]) == list(np.repeat(np.arange(len(blocks)), counts))
    assert list(got["att_block_slot"]) == list(np.repeat([b.slot_number for b in blocks], counts))
    for a, beg, end in zip(atts, got["att_beg"], got["att_end"]):
        assert raw[int(beg):int(end)] == wire.attestation_record(a)


def test_attestation_hashes_over_the_spans():
    """Attestation.Hash() of every attestation of the batch where it lies: one launch."""
    import torch

    blocks, data, offs = chain()
    d, blk = device_blocks(data, offs)
    natt = int(blk["natt"].item())
    dig = torch.empty(natt * 32, dtype=torch.uint8, device="cuda")
    _lib.lib.call("pz_dev_blake2b512_spans", d.data_ptr(), blk["att_beg"].data_ptr(), blk["att_end"].data_ptr(), natt,
                  dig.data_ptr(), 32, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    want = b"".join(hashlib.blake2b(wire.attestation_record(a)).digest()[:32] for b in blocks for a in b.attestations)
    assert dig.cpu().numpy().tobytes() == want


def test_timestamp_and_absent_fields():
    blocks = [pb.BeaconBlock(), pb.BeaconBlock(timestamp=pb.Timestamp()),
              pb.BeaconBlock(timestamp=pb.Timestamp(-5, -3)),
              pb.BeaconBlock(slot_number=(1 << 64) - 1, pow_chain_ref=b"x", timestamp=pb.Timestamp(1 << 40, 999999999))]
    got = wire.unwire_blocks(*serialize_blocks(blocks))
    assert not got["status"].any() and got["natt"] == 0 and not got["att_first"].any()
    assert list(got["has_timestamp"]) == [0, 1, 1, 1]
    assert list(got["ts_seconds"]) == [0, 0, -5, 1 << 40] and list(got["ts_nanos"]) == [0, 0, -3, 999999999]
    assert list(got["slot_number"]) == [0, 0, 0, (1 << 64) - 1]
    assert got["bytes_len"].tolist() == [[0] * 5] * 3 + [[0, 0, 1, 0, 0]]


def folded_status(raws):
    """The folded status of each block of a batch, computed on the device."""
    import torch

    offs = np.zeros(len(raws) + 1, dtype=U64)
    offs[1:] = np.cumsum([len(r) for r in raws], dtype=U64)
    d, blk = device_blocks(np.frombuffer(b"".join(raws) + bytes(16), dtype=np.uint8), offs)
    natt = int(blk["natt"].item())
    att = wire.unwire_attestations_device(d, blk["att_beg"], blk["att_end"], natt, 0)
    st = wire.folded_block_status(blk["status"], blk["att_block"][:natt], att["status"][:natt])
    torch.cuda.synchronize()
    return [int(x) for x in st.cpu().numpy()]


def test_folded_status_is_the_engines_verdict():
    """PZ_EINVAL exactly where the engine raises it (tests/test_canonical_gpu.py's tables, the
    unknown-field block included), alone and as one batch."""
    want = {k: _lib.PZ_EINVAL for k, v in NONCANONICAL.items() if v is not None}
    want.update({k: _lib.PZ_OK for k in CANONICAL})
    want["unknown field 9 appended"] = _lib.PZ_EINVAL
    raws = {**{k: v for k, v in NONCANONICAL.items() if v is not None}, **CANONICAL,
            "unknown field 9 appended": UNKNOWN_FIELD_BLOCK}
    assert dict(zip(raws, folded_status(list(raws.values())))) == want
    assert {k: folded_status([v])[0] for k, v in raws.items()} == want


# ---- 6. end to end ------------------------------------------------------------------------------
def test_check_serialized_blocks_matches_the_checks_from_objects():
    """A seeded batch that reaches every PZ_ATT_* status and both panic codes, wrapped into
    blocks of 0-3 attestations and serialized, at 1,024 validators; two blocks whose bytes the
    engine rejects ride along."""
    lsr, ljs, n_recent = 64, 60, 128
    active, cstate = ref.new_genesis_states(1024)
    cstate.last_state_recalc, cstate.last_justified_slot = lsr, ljs
    del active.recent_block_hashes[n_recent:]
    for arr in cstate.shard_and_committees_for_slots:  # 13 members: bitfields with trailing bits
        for sc in arr.array_shard_and_committee:
            del sc.committee[-3:]
    atts, bslots = random_batch(np.random.default_rng(77), cstate, 1500, lsr, n_recent)
    enc, counts, i = [], [], 0
    while i < len(atts):
        g = min((1, 2, 0, 3)[len(enc) % 4], len(atts) - i)
        bslots[i:i + g] = [bslots[i]] * g  # a block's attestations share its slot
        enc.append(wire.beacon_block(pb.BeaconBlock(parent_hash=b"\x01" * 32, slot_number=bslots[i] if g else 9,
                                                    timestamp=pb.Timestamp(8, 0), attestations=atts[i:i + g])))
        counts.append(g)
        i += g
    want_st, want_ci, want_ps = check_attestations(atts, bslots, ljs, lsr, n_recent, table(cstate))
    assert {0, 2, 3, 4, 5, 6, 7, _lib.PZ_ERANGE, _lib.PZ_EINDEX} <= set(int(x) for x in want_st)
    # a block with a non-canonical attestation body, and one whose top level is not canonical
    enc += [NONCANONICAL["attestation: explicit zero slot"], NONCANONICAL["slot field repeated at the end"]]
    offs = np.zeros(len(enc) + 1, dtype=U64)
    offs[1:] = np.cumsum([len(e) for e in enc], dtype=U64)
    data = np.frombuffer(b"".join(enc) + bytes(16), dtype=np.uint8)
    bst, first, st, ci, ps = check_serialized_blocks(data, offs, ljs, lsr, n_recent, table(cstate))
    assert list(bst) == [_lib.PZ_OK] * len(counts) + [_lib.PZ_EINVAL] * 2
    assert list(first) == [0] + list(np.cumsum(counts + [1, 0]))
    n = len(atts)
    assert list(st[:n]) == list(want_st) and list(st[n:]) == [_lib.PZ_EINVAL]
    np.testing.assert_array_equal(ci[:n], want_ci)
    np.testing.assert_array_equal(ps[:n], want_ps)


# ---- 7. host forms ------------------------------------------------------------------------------
def test_host_form_equals_device_form():
    spans = list(rand_records(300)) + [CORPUS["08 00"], CORPUS["a length of 2^63"]] + list(rand_records(7))
    host, dev = wire.unwire_attestations(*batch(spans)), device_decode(spans)
    assert set(host) == set(dev)
    for k in host:
        np.testing.assert_array_equal(host[k], dev[k], err_msg=k)


def test_block_host_form_equals_device_form():
    import torch

    blocks, data, offs = chain()
    host = wire.unwire_blocks(data, offs)
    _, blk = device_blocks(data, offs)
    torch.cuda.synchronize()
    natt = int(blk["natt"].item())
    assert natt == host["natt"]
    for k in wire.BLOCK_COLS:
        d = blk[k][:natt] if k in ("att_beg", "att_end", "att_block_slot", "att_block") else blk[k]
        np.testing.assert_array_equal(host[k].astype(np.int64), d.cpu().numpy().astype(np.int64), err_msg=k)
    # a batch that does not start at its buffer's first byte: spans are positions in the buffer
    shifted = wire.unwire_blocks(np.concatenate([np.full(5, 0xEE, dtype=np.uint8), data]), offs + U64(5))
    np.testing.assert_array_equal(shifted["att_beg"], host["att_beg"] + U64(5))
    np.testing.assert_array_equal(shifted["att_end"], host["att_end"] + U64(5))
    np.testing.assert_array_equal(shifted["bytes_beg"], host["bytes_beg"] + U64(5))


@pytest.mark.parametrize("short", range(6))
def test_short_capacity(short):
    """PZ_ERANGE with the totals filled and no output touched when one capacity is short."""
    recs = rand_records(300)
    data, offs = batch(recs)
    full = wire.unwire_attestations(data, offs)
    nbytes = int(offs[-1])
    size = wire._att_out_sizes(len(recs), nbytes)
    cols = {k: np.full(size[k] * (8 if k not in wire._BYTES_COLS + ("last_byte",) else 1), 0xAB, dtype=np.uint8)
            for k in wire.ATT_OUT_COLS}
    c = _lib.AttestationColsOut(*[cols[k].ctypes.data for k in wire.ATT_OUT_COLS])
    caps = np.array([nbytes, nbytes, nbytes, nbytes // 2, nbytes, nbytes], dtype=U64)
    assert full["totals"][short] > 0
    caps[short] = full["totals"][short] - U64(1)
    totals = np.zeros(7, dtype=U64)
    with pytest.raises(_lib.PzError) as e:
        _lib.lib.call("pz_unwire_attestations", data.ctypes.data, offs.ctypes.data, len(recs), 0, ctypes.byref(c),
                      caps.ctypes.data, totals.ctypes.data)
    assert e.value.code == _lib.PZ_ERANGE
    np.testing.assert_array_equal(totals, full["totals"])
    assert all((v == 0xAB).all() for v in cols.values())


def test_short_attestation_capacity():
    blocks, data, offs = chain()
    n, natt = len(blocks), sum(len(b.attestations) for b in blocks)
    cap = natt - 1
    size = dict(slot_number=n, ts_seconds=n, ts_nanos=n, has_timestamp=n, bytes_beg=5 * n, bytes_len=5 * n,
                att_first=n + 1, att_beg=cap, att_end=cap, att_block_slot=cap, att_block=cap, status=n)
    cols = {k: np.full(size[k] * 8, 0xAB, dtype=np.uint8) for k in wire.BLOCK_COLS}
    c = _lib.BlockColsOut(*[cols[k].ctypes.data for k in wire.BLOCK_COLS])
    got = ctypes.c_uint64(0)
    with pytest.raises(_lib.PzError) as e:
        _lib.lib.call("pz_unwire_blocks", data.ctypes.data, offs.ctypes.data, n, cap, ctypes.byref(c),
                      ctypes.byref(got))
    assert e.value.code == _lib.PZ_ERANGE and got.value == natt
    assert all((v == 0xAB).all() for v in cols.values())
