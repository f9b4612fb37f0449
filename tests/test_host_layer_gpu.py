"""The host layer under the column entry points (prysm_amd/csrc/att_cols.h, resident.h) on the GPU:
a host-pointer form stages the columns by one rule and must compute what the device-pointer form
computes over the same columns where they lie, also when the ranges do not start at 0; and a
host-pointer form on a resident handle waits for the handle's last stream, so it lands after a
device-pointer form enqueued before it on another stream.  Every result is integers and bytes:
every comparison is exact."""
import ctypes

import numpy as np
import pytest

from prysm_amd import _lib, pb, types, wire
from prysm_amd import blockchain as bc
from prysm_amd.pending import DevicePendingAttestations
from prysm_amd.votes import DeviceVoteCache

pytestmark = pytest.mark.gpu

U64 = np.uint64
PAD = 7  # bytes before the first range of every bytes column
_BYTES = ("justified_block_hash", "shard_block_hash", "attester_bitfield")


def five_records():
    """One with two oblique elements, one with an empty bitfield, one with a signature."""
    rng = np.random.default_rng(5)
    mk = lambda bf, elems, nsig: pb.AttestationRecord(  # noqa: E731
        slot=int(rng.integers(1, 200)), shard_id=int(rng.integers(0, 1024)), justified_slot=int(rng.integers(0, 100)),
        justified_block_hash=rng.bytes(32), shard_block_hash=rng.bytes(int(rng.integers(1, 40))), attester_bitfield=rng.bytes(bf),
        oblique_parent_hashes=[rng.bytes(e) for e in elems],
        aggregate_sig=[int(x) for x in rng.integers(0, 1 << 63, size=nsig, dtype=np.uint64)])
    return [mk(4, (32, 5), 0), mk(0, (), 0), mk(4, (), 1), mk(4, (32,), 2), mk(4, (), 0)]


def shifted(cols, elems=0, sigs=0):
    """The same records through columns whose ranges do not start at 0: PAD bytes lie before the
    first range of every bytes column (the elements' too), ``elems`` elements no row names before
    the first element and ``sigs`` values before the first signature value."""
    pad = np.full(PAD, 0xA5, np.uint8)
    out = dict(cols)
    for k in _BYTES:
        out[k] = np.concatenate([pad, cols[k]])
        out[k + "_offs"] = cols[k + "_offs"] + U64(PAD)
    out["oblique_parent_hashes"] = np.concatenate([pad, cols["oblique_parent_hashes"]])
    out["oblique_offs"] = np.concatenate([np.zeros(elems, U64), cols["oblique_offs"] + U64(PAD)])
    out["oblique_first"] = cols["oblique_first"] + U64(elems)
    out["aggregate_sig"] = np.concatenate([np.full(sigs, 0xA5A5, U64), cols["aggregate_sig"]])
    out["aggregate_sig_first"] = cols["aggregate_sig_first"] + U64(sigs)
    return out


def on_device(cols):
    """Host columns as device tensors, every one with 64 readable bytes after its last."""
    import torch

    def put(a):
        a = np.ascontiguousarray(a)
        raw = np.concatenate([a.view(np.uint8).ravel(), np.full(64, 0xA5, np.uint8)])
        t = torch.from_numpy(raw).to("cuda:0")[:a.nbytes]
        return t.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.dtype.itemsize])

    return {k: put(v) for k, v in cols.items()}


def dev_wire(cols, n):
    """pz_dev_wire_attestations (bare records) over device tensors: (bytes, offsets)."""
    import torch

    d = on_device(cols)
    c = _lib.AttestationCols(*[d[k].data_ptr() for k in wire.ATT_COLS])
    nbytes = sum(int(cols[k][-1]) for k in ("justified_block_hash_offs", "shard_block_hash_offs", "attester_bitfield_offs",
                                            "oblique_offs"))
    bound = int(_lib.lib.dll.pz_wire_attestations_bound(n, nbytes, int(cols["oblique_first"][-1]), int(cols["aggregate_sig_first"][-1])))
    out = torch.empty(bound, dtype=torch.uint8, device="cuda:0")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda:0")
    scr = torch.empty(int(_lib.lib.dll.pz_wire_attestations_scratch_bytes(n)), dtype=torch.uint8, device="cuda:0")
    _lib.lib.call("pz_dev_wire_attestations", ctypes.byref(c), n, 0, out.data_ptr(), offs.data_ptr(), scr.data_ptr(),
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    offs = offs.cpu().numpy().view(U64)
    return out[:int(offs[-1])].cpu().numpy().tobytes(), offs


# the checks' outputs the digests and the tallies take: every row PROCESSED
N_RECENT = 70
PARENTS_START = np.array([0, 1, 2, 3, 4], dtype=U64)
STATUS = np.zeros(5, dtype=np.int32)
COMMITTEE = np.array([0, 1, 0, 0, 0], dtype=np.uint32)  # (committee 1 is empty: the row with no bitfield)
MEMBERS, COFFS = np.arange(32, dtype=np.uint32), np.array([0, 32, 32], dtype=U64)
BALANCE = np.arange(1, 65, dtype=U64)


def run(entry, form, cols):
    """What ``entry`` computes from ``cols`` through its host or its device form, as comparable values."""
    import torch

    n = 5
    recent = np.random.default_rng(7).integers(0, 256, size=(N_RECENT, 32), dtype=np.uint8)
    d = on_device(cols) if form == "device" else None
    t = lambda a: on_device({"a": a})["a"]  # noqa: E731
    if entry == "pz_wire_attestations":
        out, offs = wire.attestations_device(cols, n) if form == "host" else dev_wire(cols, n)
        return out, offs.tolist()
    if entry == "pz_attestation_keys":
        if form == "host":
            return (types.attestation_keys_columns(cols, n, 64).tobytes(),)
        return (types.attestation_keys_device(d, n, out_bytes=64).cpu().numpy().tobytes(),)
    if entry == "pz_attestation_messages":
        if form == "host":
            dig, mlen = bc.attestation_messages(cols, n, STATUS, PARENTS_START, recent)
            return dig.tobytes(), mlen.tolist()
        dig, mlen = bc.attestation_messages_device(d, n, t(STATUS), t(PARENTS_START), t(recent))
        return dig.cpu().numpy().tobytes(), mlen.cpu().numpy().tolist()
    if entry == "pz_att_pool_append":
        pool = DevicePendingAttestations([8, 256, 256, 64, 8, 128, 8])
        if form == "host":
            pool.append_host(cols, n, STATUS, COMMITTEE)
        else:
            pool.append_columns(d, n, t(STATUS), t(COMMITTEE))
        return pool.counts().tolist(), pool.records(), pool.columns()["committee"].tolist()
    assert entry == "pz_vote_cache_tally"
    cache = DeviceVoteCache(64, 512)
    if form == "host":
        cache.tally_host(cols, n, STATUS, COMMITTEE, PARENTS_START, recent, MEMBERS, COFFS, BALANCE)
    else:
        cache.tally_columns(d, n, t(STATUS), t(COMMITTEE), t(PARENTS_START), t(recent), t(MEMBERS), t(COFFS), t(BALANCE))
        torch.cuda.synchronize()
    hashes, totals = cache.read()
    return hashes.tobytes(), totals.tolist()


ENTRIES = ["pz_wire_attestations", "pz_attestation_keys", "pz_attestation_messages", "pz_att_pool_append",
           "pz_vote_cache_tally"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_host_form_equals_device_form_at_a_nonzero_base(entry):
    """Five records through columns whose bytes ranges begin PAD bytes into their buffers: the host
    form (staged by the one rule) equals the device form over the same columns, and both equal the
    host form over the plain columns, whose ranges start at 0.  For the pool and the cache the
    oblique ranges also begin at a non-zero element (the pool's signature ranges at a non-zero
    value); the encoder refuses those two, as it always has."""
    recs = five_records()
    plain = wire.attestation_columns(recs)
    refuses = entry == "pz_wire_attestations"
    resident = entry in ("pz_att_pool_append", "pz_vote_cache_tally")
    cols = shifted(plain, elems=2 if resident else 0, sigs=3 if entry == "pz_att_pool_append" else 0)
    want = run(entry, "host", plain)
    if entry == "pz_att_pool_append":
        assert want[1] == recs
    if refuses:
        assert want[0] == b"".join(wire.attestation_record(r) for r in recs)
        for kw, text in (({"elems": 2}, "oblique ranges must start at 0"), ({"sigs": 3}, "signature ranges must start at 0")):
            with pytest.raises(_lib.PzError, match=text) as e:
                run(entry, "host", shifted(plain, **kw))
            assert e.value.code == _lib.PZ_EINVAL
    assert any(want[0]) if isinstance(want[0], bytes) else want[0][0] == 5
    assert run(entry, "host", cols) == want
    assert run(entry, "device", cols) == want


def test_pool_host_append_lands_after_a_device_append_on_another_stream():
    """A device-form append of 513 rows (two tiles and a row) on a side stream, then at once a
    host-form append of 3 rows: the pool holds the 516 rows in that order."""
    import torch

    rng = np.random.default_rng(513)
    mk = lambda: pb.AttestationRecord(  # noqa: E731
        slot=int(rng.integers(1, 200)), shard_id=int(rng.integers(0, 1024)), justified_slot=1,
        justified_block_hash=rng.bytes(32), shard_block_hash=rng.bytes(32), attester_bitfield=rng.bytes(4),
        oblique_parent_hashes=[rng.bytes(32)] * int(rng.integers(0, 2)), aggregate_sig=[])
    first, then = [mk() for _ in range(513)], [mk() for _ in range(3)]
    pool = DevicePendingAttestations([516, 516 * 32, 516 * 32, 516 * 4, 516, 516 * 32, 1])
    d = on_device(wire.attestation_columns(first))
    status = on_device({"s": np.zeros(513, np.int32), "c": np.arange(513, dtype=np.uint32)})
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pool.append_columns(d, 513, status["s"], status["c"])
    pool.append_host(wire.attestation_columns(then), 3, np.zeros(3, np.int32), np.arange(513, 516, dtype=np.uint32))
    assert pool.counts()[0] == 516
    assert pool.records() == first + then
    assert pool.columns()["committee"].tolist() == list(range(516))
    side.synchronize()


def test_cache_host_tally_lands_after_a_device_tally_on_another_stream():
    """A device-form tally of 64 rows naming hashes A on a side stream, then at once a host-form
    tally naming hashes B: slots are numbered in the order the calls land, so the read lists A's
    slots before B's."""
    import torch

    rng = np.random.default_rng(64)
    a_hashes = rng.integers(0, 256, size=(127, 32), dtype=np.uint8)  # row i signs A[i .. i + 64)
    b_hashes = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
    rows = lambda n: wire.attestation_columns([pb.AttestationRecord(  # noqa: E731
        slot=1, shard_id=0, justified_slot=0, justified_block_hash=b"", shard_block_hash=b"", attester_bitfield=b"\xff",
        oblique_parent_hashes=[], aggregate_sig=[]) for _ in range(n)])
    members, coffs, balance = np.arange(8, dtype=np.uint32), np.array([0, 8], dtype=U64), np.arange(1, 9, dtype=U64)
    cache = DeviceVoteCache(8, 256)
    d = on_device(rows(64))
    x = on_device({"status": np.zeros(64, np.int32), "committee": np.zeros(64, np.uint32), "ps": np.arange(64, dtype=U64),
                   "recent": a_hashes, "members": members, "coffs": coffs, "balance": balance})
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cache.tally_columns(d, 64, x["status"], x["committee"], x["ps"], x["recent"], x["members"], x["coffs"], x["balance"])
    cache.tally_host(rows(1), 1, np.zeros(1, np.int32), np.zeros(1, np.uint32), np.zeros(1, U64), b_hashes, members, coffs,
                     balance)
    hashes, totals = cache.read()
    assert hashes.tobytes() == a_hashes.tobytes() + b_hashes.tobytes()
    assert totals.tolist() == [int(balance.sum())] * 191
    side.synchronize()
