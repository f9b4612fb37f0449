"""Attestation.Key and the processAttestation message digest from columns
(prysm_amd/csrc/attdigest.hip: pz_[dev_]attestation_keys, pz_[dev_]attestation_messages, and
blockchain.digest_serialized_blocks over them).

The oracle is hashlib.blake2b over oracle.ref's byte strings (attestation_key_bytes,
types/attestation.go:61-77; process_attestation_message over get_signed_parent_hashes,
blockchain/core.go:277-290, :348-360): it shares nothing with the code under test."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

from oracle import ref
from oracle import replay as oreplay
from prysm_amd import _lib, pb, synth, types, wire
from prysm_amd import blockchain as bc
from test_attcheck_gpu import PROCESSED, oracle_code, random_batch, table
from test_wire import rand_att, rand_bytes

pytestmark = pytest.mark.gpu

U64 = np.uint64
KEY_COLS = ("slot", "shard_id", "shard_block_hash", "shard_block_hash_offs", "oblique_parent_hashes", "oblique_offs",
            "oblique_first")
BYTES_COLS = ("shard_block_hash", "oblique_parent_hashes")


def sum512(b):
    return hashlib.blake2b(bytes(b), digest_size=64).digest()


def want_keys(atts, out_bytes=32):
    return np.array([list(sum512(ref.attestation_key_bytes(a))[:out_bytes]) for a in atts],
                    dtype=np.uint8).reshape(len(atts), out_bytes)


def to_device(cols):
    """The key / message columns as torch tensors; every bytes column ends in the 4 readable
    bytes of the contract, filled with 0xA5 so a byte taken from them shows in a digest."""
    import torch

    dev = torch.device("cuda", 0)
    out = {}
    for k in KEY_COLS:
        a = np.ascontiguousarray(cols[k])
        if k in BYTES_COLS:
            used = int(cols[k + "_offs" if k == "shard_block_hash" else "oblique_offs"][-1])
            a = np.concatenate([a[:used], np.full(4, 0xA5, np.uint8)])
        out[k] = torch.from_numpy(a.view(np.int64) if a.dtype == U64 else a.copy()).to(dev)
    return out


def device_keys(atts, out_bytes=32, rec_status=None):
    import torch

    d = to_device(wire.attestation_columns(atts))
    st = None if rec_status is None else torch.from_numpy(np.asarray(rec_status, np.int32)).to("cuda:0")
    got = types.attestation_keys_device(d, len(atts), rec_status=st, out_bytes=out_bytes)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def key_att(rng):
    """test_wire.rand_att with the ranges closed: ShardBlockHash of 0-40 bytes, 0-3 elements of
    0-33 bytes."""
    a = rand_att(rng)
    a.shard_block_hash = rand_bytes(rng, 0, 41)
    a.oblique_parent_hashes = [rand_bytes(rng, 0, 34) for _ in range(int(rng.integers(0, 4)))]
    return a


# ---- Key ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 257, 2000])
def test_keys_random_records(n):
    rng = np.random.default_rng(500 + n)
    atts = [key_att(rng) for _ in range(n)]
    for ob in (32, 64):
        want = want_keys(atts, ob)
        dev = device_keys(atts, ob)
        np.testing.assert_array_equal(dev, want)
        host = types.attestation_keys_columns(wire.attestation_columns(atts), n, ob)
        np.testing.assert_array_equal(host, dev)


# varints of 1, 2, 9 and 10 bytes on both sides; a shard id shorter than the slot leaves slot bytes behind
VARINTS = [(0, 0), (127, 128), (1 << 62, 5), ((1 << 64) - 1, 300), (5, 1 << 63), (1 << 56, 1 << 62),
           (16383, 16384), ((1 << 63) + 77, 1 << 56), (300, 1)]


def test_keys_block_edges():
    """Message lengths 10 + sl + 32 m on and around 128 and 256 (sl 118, 119, 246), up to 19
    blocks (m = 65: past any fixed cap on the element count)."""
    rng = np.random.default_rng(7)
    atts = []
    for sl in (0, 1, 31, 32, 33, 118, 119, 246):
        for m in (0, 1, 3, 4, 64, 65):
            slot, shard = VARINTS[len(atts) % len(VARINTS)]
            elems = [rng.bytes(int(rng.choice([0, 31, 32, 32, 32, 33, 40]))) for _ in range(m)]
            atts.append(pb.AttestationRecord(slot=slot, shard_id=shard, shard_block_hash=rng.bytes(sl),
                                             oblique_parent_hashes=elems))
    lens = {len(ref.attestation_key_bytes(a)) for a in atts}
    assert {128, 129, 256} <= lens and max(lens) > 17 * 128
    for ob in (32, 64):
        np.testing.assert_array_equal(device_keys(atts, ob), want_keys(atts, ob))
    np.testing.assert_array_equal(types.attestation_keys_columns(wire.attestation_columns(atts), len(atts)),
                                  want_keys(atts))


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_keys_alignment(phase):
    """A first record of `phase` bytes in both bytes columns starts every later range at that
    byte phase of its (256-byte aligned) column."""
    rng = np.random.default_rng(40 + phase)
    atts = [pb.AttestationRecord(slot=1, shard_id=2, shard_block_hash=rng.bytes(phase),
                                 oblique_parent_hashes=[rng.bytes(phase)])]
    for el in (0, 31, 32, 33, 40):
        for sl in (0, 5, 32, 33):
            atts.append(pb.AttestationRecord(slot=int(rng.integers(0, 1 << 40)), shard_id=int(rng.integers(0, 1 << 20)),
                                             shard_block_hash=rng.bytes(sl),
                                             oblique_parent_hashes=[rng.bytes(el), rng.bytes(4 * ((el + 3) // 4))]))
    np.testing.assert_array_equal(device_keys(atts), want_keys(atts))
    np.testing.assert_array_equal(types.attestation_keys_columns(wire.attestation_columns(atts), len(atts)),
                                  want_keys(atts))


def test_keys_bad_rows_are_zero():
    rng = np.random.default_rng(11)
    atts = [key_att(rng) for _ in range(300)]
    st = np.zeros(300, np.int32)
    bad = rng.random(300) < 0.2
    st[bad] = _lib.PZ_EINVAL
    st[7] = 3  # any status but PZ_OK
    bad[7] = True
    want = want_keys(atts)
    want[bad] = 0
    np.testing.assert_array_equal(device_keys(atts, rec_status=st), want)


def test_keys_null_columns_follow_the_encoders_rules():
    """NULL scalars are 0 everywhere, NULL offsets empty ranges (pz_attestation_cols)."""
    atts = [pb.AttestationRecord() for _ in range(5)]
    got = types.attestation_keys_columns({}, 5)
    np.testing.assert_array_equal(got, want_keys(atts))


# ---- messages -------------------------------------------------------------------------------------
def message_batch(rng, cstate, n, lsr, n_recent):
    """test_attcheck_gpu.random_batch's rows (every failing check) plus as many rows built to pass:
    m from {0, 1, 63, 64} with elements shorter and longer than 32 bytes, ShardBlockHash of 0, 32
    or 40 bytes, parents_start at 0, at n_recent - 64 and in between."""
    atts, bslots = random_batch(rng, cstate, n // 2, lsr, n_recent)
    arrs = table(cstate)
    for _ in range(n - n // 2):
        start = int(rng.choice([0, n_recent - 64, int(rng.integers(0, n_recent - 63))]))
        s = lsr + int(rng.integers(0, len(arrs)))
        shard, comm = arrs[s - lsr][int(rng.integers(0, len(arrs[s - lsr])))]
        k = len(comm)
        bf = bytearray(rng.integers(0, 256, size=(k + 7) // 8, dtype=np.uint8).tobytes())
        if k % 8:
            bf[-1] &= (0xFF << (8 - k % 8)) & 0xFF
        m = int(rng.choice([0, 1, 63, 64]))
        elems = [rng.bytes(int(rng.choice([0, 5, 31, 32, 32, 33, 40]))) for _ in range(m)]
        atts.append(pb.AttestationRecord(slot=s, shard_id=shard, justified_slot=cstate.last_justified_slot,
                                         attester_bitfield=bytes(bf), shard_block_hash=rng.bytes(int(rng.choice([0, 32, 40]))),
                                         oblique_parent_hashes=elems))
        bslots.append(s + start)
    order = rng.permutation(len(atts))
    return [atts[i] for i in order], [bslots[i] for i in order]


@functools.lru_cache(None)
def message_case(lsr, ljs, n_recent):
    """(atts, block slots, recent hashes, oracle statuses, oracle digests, oracle lengths), once."""
    active, cstate = ref.new_genesis_states(1024)
    cstate.last_state_recalc, cstate.last_justified_slot = lsr, ljs
    rng = np.random.default_rng(900 + lsr + n_recent)
    del active.recent_block_hashes[:]
    active.recent_block_hashes.extend(rng.bytes(32 if i % 5 else i % 32) for i in range(n_recent))  # some short: BytesToHash
    atts, bslots = message_batch(rng, cstate, 1500, lsr, n_recent)
    o_atts = [oreplay.to_pb_block(pb.BeaconBlock(attestations=[a])).attestations[0] for a in atts]
    codes = np.array([oracle_code(cstate, active, bs, a) for a, bs in zip(o_atts, bslots)], dtype=np.int32)
    digests = np.zeros((len(atts), 64), np.uint8)
    lens = np.zeros(len(atts), np.uint32)
    for i, (a, bs) in enumerate(zip(o_atts, bslots)):
        if codes[i] == PROCESSED:
            msg = ref.process_attestation_message(a, ref.get_signed_parent_hashes(active, bs, a))
            digests[i] = list(sum512(msg))
            lens[i] = len(msg)
    return atts, bslots, [bytes(h) for h in active.recent_block_hashes], codes, digests, lens


@pytest.mark.parametrize("lsr,ljs,n_recent", [(0, 0, 128), (64, 60, 128), (64, 60, 100)])
def test_messages_match_oracle(lsr, ljs, n_recent):
    import torch

    atts, bslots, recent, codes, want, want_len = message_case(lsr, ljs, n_recent)
    n = len(atts)
    assert (codes == PROCESSED).sum() >= n // 4  # (a condition on the inputs)
    ms = {len(a.oblique_parent_hashes) for a, c in zip(atts, codes) if c == PROCESSED}
    starts = {bs - a.slot for a, bs, c in zip(atts, bslots, codes) if c == PROCESSED}
    assert {0, 1, 63, 64} <= ms and {0, n_recent - 64} <= starts
    pstart = np.array([(bs - a.slot) & ((1 << 64) - 1) for a, bs in zip(atts, bslots)], dtype=U64)
    cols = wire.attestation_columns(atts)
    host, host_len = bc.attestation_messages(cols, n, codes, pstart, recent)
    np.testing.assert_array_equal(host_len, want_len)
    np.testing.assert_array_equal(host, want)
    d = to_device(cols)
    dev = torch.device("cuda", 0)
    got, got_len = bc.attestation_messages_device(
        d, n, torch.from_numpy(codes).to(dev), torch.from_numpy(pstart.view(np.int64)).to(dev),
        torch.from_numpy(bc._recent_array(recent).copy()).to(dev))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got_len.cpu().numpy().view(np.uint32), want_len)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert not want[codes != PROCESSED].any() and not want_len[codes != PROCESSED].any()


# ---- against the engine -----------------------------------------------------------------------------
def test_digest_serialized_blocks_matches_the_engine():
    """130 blocks at 1,024 validators (two cycle transitions) through BeaconChain.process_serialized,
    and the same bytes through digest_serialized_blocks against the state each block meets.  That
    state is the oracle chain's just before the block: RecentBlockHashes moves with every block
    (computeNewActiveState, core.go:223-237), so the calls go block by block."""
    nval, nblocks = 1024, 130
    blocks = synth.chain_blocks(nval, nblocks, seed=4)
    data, offs = bc.serialize_blocks(blocks)
    br, ar = bc.BeaconChain(nval).process_serialized(data, offs)
    assert (ar["status"] == bc.ATT_PROCESSED).all() and len(ar) >= nblocks
    chain = oreplay.Chain(nval)
    tables = {}
    seen = 0
    for i, blk in enumerate(blocks):
        C, A = chain.C, chain.A.data
        if C.last_state_recalc not in tables:
            tables[C.last_state_recalc] = table(C)
        tab = tables[C.last_state_recalc]
        lo, hi = int(offs[i]), int(offs[i + 1])
        got = bc.digest_serialized_blocks(data[lo:hi], np.array([0, hi - lo], dtype=U64), C.last_justified_slot,
                                          C.last_state_recalc, len(A.recent_block_hashes), tab,
                                          [bytes(h) for h in A.recent_block_hashes])
        assert list(got["block_status"]) == [_lib.PZ_OK]
        assert got["block_hash"][0].tobytes() == br["hash"][i].tobytes()
        f, k = int(br["first_att"][i]), int(br["natt"][i])
        assert list(got["att_first"]) == [0, k]
        rows = ar[f:f + k]
        np.testing.assert_array_equal(got["att_status"], rows["status"])
        for name, col in (("key", "key"), ("hash", "hash"), ("msg", "msg"), ("msg_len", "msg_len")):
            np.testing.assert_array_equal(got[name], rows[col], err_msg="%s of block %d" % (name, i))
        seen += k
        chain.process_block(oreplay.to_pb_block(blk))
    assert seen == len(ar)


# ---- edge cases -------------------------------------------------------------------------------------
def call(name, *args):
    return getattr(_lib.lib.dll, name)(*args)


def test_empty_batches():
    assert types.attestation_keys_columns({}, 0).shape == (0, 32)
    out, ln = bc.attestation_messages({}, 0, np.zeros(0, np.int32), np.zeros(0, U64), [])
    assert out.shape == (0, 64) and ln.shape == (0,)
    assert call("pz_dev_attestation_keys", None, 0, None, None, 64, None) == _lib.PZ_OK
    b = _lib.AttMsgBatch()
    assert call("pz_dev_attestation_messages", ctypes.byref(b), None) == _lib.PZ_OK
    assert call("pz_attestation_messages", ctypes.byref(b)) == _lib.PZ_OK


def test_argument_errors_are_einval():
    """Each is refused on the host, before any launch: the pointers below are never followed."""
    import torch

    c = _lib.AttestationCols()
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    host = np.zeros(256, np.uint8)
    p, hp = buf.data_ptr(), host.ctypes.data
    for ob in (0, 16, 48, 65):
        assert call("pz_dev_attestation_keys", ctypes.byref(c), 1, None, p, ob, None) == _lib.PZ_EINVAL
        assert call("pz_attestation_keys", ctypes.byref(c), 1, hp, ob) == _lib.PZ_EINVAL
        assert call("pz_attestation_keys", ctypes.byref(c), 0, hp, ob) == _lib.PZ_EINVAL
    assert call("pz_dev_attestation_keys", None, 1, None, p, 32, None) == _lib.PZ_EINVAL
    assert call("pz_dev_attestation_keys", ctypes.byref(c), 1, None, None, 32, None) == _lib.PZ_EINVAL
    assert call("pz_attestation_keys", None, 1, hp, 32) == _lib.PZ_EINVAL
    assert call("pz_attestation_keys", ctypes.byref(c), 1, None, 32) == _lib.PZ_EINVAL
    assert call("pz_dev_attestation_keys", ctypes.byref(c), 1, None, p + 8, 32, None) == _lib.PZ_EINVAL  # alignment
    offs_only = _lib.AttestationCols(shard_block_hash_offs=p)
    assert call("pz_dev_attestation_keys", ctypes.byref(offs_only), 1, None, p, 32, None) == _lib.PZ_EINVAL

    status = np.zeros(4, np.int32)  # PROCESSED
    pstart = np.zeros(4, U64)
    recent = np.zeros((64, 32), np.uint8)
    out = np.zeros((4, 64), np.uint8)

    def host_batch(**kw):
        f = dict(natt=4, status=status.ctypes.data, parents_start=pstart.ctypes.data, recent=recent.ctypes.data,
                 n_recent=64, out=out.ctypes.data)
        f.update(kw)
        return _lib.AttMsgBatch(**f)

    assert call("pz_attestation_messages", None) == _lib.PZ_EINVAL
    for kw in (dict(status=None), dict(parents_start=None), dict(out=None), dict(recent=None), dict(n_recent=63),
               dict(oblique_first=hp)):
        assert call("pz_attestation_messages", ctypes.byref(host_batch(**kw))) == _lib.PZ_EINVAL, kw
    # n_recent < 64 is an error only while some row is PROCESSED
    status[:] = bc.ATT_NOT_PROCESSED
    out[:] = 1
    assert call("pz_attestation_messages", ctypes.byref(host_batch(n_recent=63))) == _lib.PZ_OK
    assert not out.any()
    status[:] = 0

    def dev_batch(**kw):
        f = dict(natt=1, status=p, parents_start=p, recent=p, n_recent=64, out=p + 64)
        f.update(kw)
        return _lib.AttMsgBatch(**f)

    assert call("pz_dev_attestation_messages", None, None) == _lib.PZ_EINVAL
    for kw in (dict(status=None), dict(parents_start=None), dict(out=None), dict(recent=None), dict(n_recent=63),
               dict(out=p + 8), dict(shard_block_hash_offs=p)):
        assert call("pz_dev_attestation_messages", ctypes.byref(dev_batch(**kw)), None) == _lib.PZ_EINVAL, kw
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()  # nothing was written
