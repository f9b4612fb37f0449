"""The stored CrystallizedState loaded on the device (prysm_amd/csrc/unwire_state.hip):
pz_dev_cstate_frame / pz_dev_cstate_decode through ``wire.unwire_crystallized_state``,
``ResidentRecalcState.from_state`` and ``ResidentChain.from_state``.  Ground truth is oracle.schema's
parse (Google's runtime) of the same bytes, and an input counts as canonical when that parse
serialises back to it; the non-canonical corpus is held against unwire_state_dev.h's sequential
verdict (the A/B library's host-only pz_debug_cstate_check) and against offsets worked out by hand."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import unwire_state_cases as uc
from oracle import ref
from oracle import replay as oreplay
from prysm_amd import _lib, pb, wire
from prysm_amd import blockchain as bc
from prysm_amd.pending import ResidentRecalcState

pytestmark = pytest.mark.gpu

U64 = np.uint64
SENTINEL = 0xA5
TILE, GROUP = _lib.CSTATE_TILE_BYTES, _lib.CSTATE_TILE_BYTES * _lib.CSTATE_GROUP_TILES  # the framing's units, in bytes
LIMIT = _lib.CSTATE_RECORD_LIMIT


def loaded(raw):
    """The device's columns of ``raw`` against the parse's; returns them."""
    assert uc.canonical(raw)
    got = wire.unwire_crystallized_state(raw)
    want = uc.truth(raw)
    uc.same_columns(got, want)
    f12 = b"".join(wire._msg(12, a.SerializeToString()) for a in uc.parse(raw).shard_and_committees_for_slots)
    r = got["result"]
    assert got["field12"] == f12
    assert (r[_lib.CSF_VAL_END], r[_lib.CSF_F12_END]) == (len(raw) - len(f12), len(raw))
    assert (r[_lib.CSF_NVAL], r[_lib.CSF_NARR]) == (want["nval"], want["narr"])
    assert all(max(n, 0) < LIMIT for n in uc.record_lengths(raw))  # every accepted input stays under the limit
    return got


SMALL_TAB = [[(3, [1, 2, 300])], [(0, [70000])]]


# ---- 1: framing edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nval", (0, 1, 2))
def test_a_handful_of_validators(nval):
    for arrays in ((), uc.arrays_of(SMALL_TAB)):
        loaded(uc.state(uc.mixed_validators(nval, seed=nval) if nval else None, arrays))
    if nval == 0:
        got = loaded(b"")  # nothing at all: zeros, nothing launched
        assert got["result"][:_lib.CSF_COUNT] == [0] * _lib.CSF_COUNT


def test_all_zero_validators_are_two_bytes_each():
    raw = uc.state(pb.Validators(3 * TILE), uc.arrays_of(SMALL_TAB))  # 2,048 records a tile, six tiles
    assert raw.count(b"\x5a\x00") >= 3 * TILE and set(uc.record_lengths(raw)) == {0}
    loaded(raw)


@pytest.mark.parametrize("framed", (5, 37, 113))
def test_records_of_one_length_put_a_header_on_every_offset_of_a_tile(framed):
    """An odd record length is coprime to the tile's 4,096 bytes: TILE + 100 records in a row start at
    every offset modulo the tile, and cross every tile edge at every split the length allows."""
    n = TILE + 100
    raw = uc.state(uc.fixed_validators(n, framed, seed=framed), uc.arrays_of(SMALL_TAB))
    lens = uc.record_lengths(raw)
    assert {x + 1 + len(wire.varint(x)) for x in lens} == {framed} and framed % 2 == 1
    body = wire.cstate_head(raw)["body_beg"]
    assert len({(body + i * framed) % TILE for i in range(n)}) == TILE
    loaded(raw)


def test_mixed_lengths():
    raw = uc.state(uc.mixed_validators(3000, seed=11), uc.arrays_of(SMALL_TAB), dynasty_seed=b"\x5a" * 32)
    lens = set(uc.record_lengths(raw))
    assert min(lens) == 0 and max(lens) == 111 and len(lens) > 60  # from 5a 00 to the full record
    loaded(raw)


def test_a_state_of_more_than_three_tile_groups():
    """The framing's largest unit is the group: 64 tiles of 4,096 bytes (PZ_CSTATE_GROUP_TILES x
    PZ_CSTATE_TILE_BYTES).  Full records over more than three of them: the chain kernel chains four
    groups, and every group's lane starts from an entry another launch computed."""
    n = 3 * GROUP // 113 + 300
    raw = uc.state(uc.full_validators(n, seed=3), uc.arrays_of(SMALL_TAB))
    assert len(raw) > 3 * GROUP + TILE
    loaded(raw)


# ---- 2: false chains ----------------------------------------------------------------------------------------
def test_bytes_fields_that_look_like_headers():
    vals = uc.mixed_validators(4000, seed=12, blobs=uc.decoy_blob)
    raw = uc.state(vals, uc.arrays_of(SMALL_TAB))
    decoys = sum(raw.count(d) for d in uc.DECOYS)
    assert decoys > 5 * (len(raw) // TILE + 1)  # several a tile
    loaded(raw)


# ---- 3: the length limit ------------------------------------------------------------------------------------
def abi_load(raw, v_sizes=None):
    """Frame and decode at the ABI, the outputs filled with a sentinel first and sized by ``v_sizes``
    (default: the frame's own numbers).  Returns (result record, decode status, outputs as numpy)."""
    import torch

    dev = torch.device("cuda", 0)
    buf = np.frombuffer(bytes(raw), np.uint8)
    head = wire.cstate_head(buf)
    d = torch.from_numpy(buf.copy()).to(dev)
    scr = torch.randint(0, 256, (int(_lib.lib.dll.pz_cstate_scratch_bytes(buf.size)),), dtype=torch.uint8, device=dev)
    result = torch.full((_lib.CSF_COUNT,), -99, dtype=torch.int64, device=dev)
    sh = _lib.stream_ptr(dev)
    _lib.lib.call("pz_dev_cstate_frame", d.data_ptr(), buf.size, head["body_beg"], scr.data_ptr(), result.data_ptr(), sh)
    r = [int(x) for x in result.cpu()]
    nval, narr, nent = v_sizes or (r[_lib.CSF_NVAL], r[_lib.CSF_NARR], r[_lib.CSF_NENTRIES])
    outs = {k: torch.full((4096,), SENTINEL, dtype=torch.uint8, device=dev) for k in wire.VALIDATOR_COLS + wire.TABLE_COLS}
    v = _lib.ValidatorColsOut(*[outs[k].data_ptr() for k in wire.VALIDATOR_COLS])
    t = _lib.CommitteeTableOut(narr=narr, ncomm=nent, **{k: outs[k].data_ptr() for k in wire.TABLE_COLS})
    status = torch.full((2,), -99, dtype=torch.int64, device=dev)
    _lib.lib.call("pz_dev_cstate_decode", d.data_ptr(), buf.size, scr.data_ptr(), ctypes.byref(v), ctypes.byref(t),
                  status.data_ptr(), sh)
    return r, [int(x) for x in status.cpu()], {k: o.cpu().numpy() for k, o in outs.items()}


def test_a_record_just_under_the_limit_decodes_and_one_at_it_is_erange():
    under = pb.Validators(3, balance=[1, 2, 3], withdrawal_address=[b"", bytes(range(256)) * 2, b""][:3])
    under.withdrawal_address[1] = under.withdrawal_address[1][:LIMIT - 6]  # 28 02 + 1a, a 2-byte length, the bytes: LIMIT - 1
    raw = uc.state(under)
    assert max(uc.record_lengths(raw)) == LIMIT - 1
    loaded(raw)
    at = pb.Validators(3, balance=[1, 2, 3], withdrawal_address=[b"", b"\x5a" * (LIMIT - 5), b""])
    raw = uc.state(at)
    assert uc.canonical(raw) and uc.record_lengths(raw) == [2, LIMIT, 2]
    with pytest.raises(_lib.PzError) as e:
        wire.unwire_crystallized_state(raw)
    first = wire.cstate_head(raw)["body_beg"] + 4
    assert (e.value.code, e.value.offset) == (_lib.PZ_ERANGE, first)  # the offset of the record's header
    r, status, outs = abi_load(raw, (3, 0, 0))
    assert r == [_lib.PZ_ERANGE, first] + [0] * (_lib.CSF_COUNT - 2)  # the record alone
    assert status == [_lib.PZ_ERANGE, first]
    assert all((o == SENTINEL).all() for o in outs.values())  # nothing else written


# ---- 4: committees -------------------------------------------------------------------------------------------
EDGES = [0, 1, 127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, (1 << 32) - 1]  # 1 to 5 bytes each
LONG = [int(x) for x in np.random.default_rng(8).integers(0, 1 << 32, size=3000, dtype=np.uint64)]   # ~14 KB of packed bytes
TABLES = {
    "member_edges": [[(5, EDGES)], [(1 << 40, EDGES[::-1])]],
    "shard_0_and_an_empty_committee": [[(0, [4, 5]), (9, []), (0, [])], [(2, [1])]],
    "an_empty_array": [[], [(1, [2])], [], []],
    "narr_1": [[(1, [2, 3])]],
    "narr_64": [[(a, [a, a + 1])] * (a % 3) for a in range(64)],
    "narr_65": [[(a % 7, list(range(a)))] for a in range(65)],
    "a_committee_longer_than_a_workgroups_round": [[(1, LONG), (2, [7])], [(3, LONG[:257])]],
    "more_arrays_than_one_framing_round": [[(1, [a])] if a % 2 else [] for a in range(1030)],
}


@pytest.mark.parametrize("name", list(TABLES))
def test_committees(name):
    tab = TABLES[name]
    raw = uc.state(uc.mixed_validators(5, seed=1), uc.arrays_of(tab))
    got = loaded(raw)
    parsed = [[(e.shard_id, list(e.committee)) for e in a.array_shard_and_committee] for a in uc.parse(raw).shard_and_committees_for_slots]
    assert parsed == [[(s, list(c)) for s, c in arr] for arr in tab]
    entries = sum(len(a) for a in tab)
    for k, want in zip(("arr_offs", "arr_shard", "arr_comm", "coffs"), bc._committee_table(parsed)):
        np.testing.assert_array_equal(got[k], want[:len(got[k])] if not entries else want, k)
    if got["members"].size:
        np.testing.assert_array_equal(got["members"], bc._members(parsed))
    loaded(uc.state(None, uc.arrays_of(tab)))  # and with no validator in front


# ---- 5: the non-canonical corpus --------------------------------------------------------------------------------
def cpu_verdict(raw):
    from ab_lib import ab_dll

    fn = ab_dll().pz_debug_cstate_check
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p], ctypes.c_int
    buf, out = np.frombuffer(bytes(raw), np.uint8).copy(), np.zeros(6, U64)
    assert fn(buf.ctypes.data, buf.size, out.ctypes.data) == _lib.PZ_OK
    return int(out.view(np.int64)[0]), int(out[1])


CORPUS = uc.corpus()


@pytest.mark.parametrize("name", [c[0] for c in CORPUS])
def test_what_is_not_canonical_is_einval_at_its_offset(name):
    _, raw, offset = next(c for c in CORPUS if c[0] == name)
    assert cpu_verdict(raw) == (_lib.PZ_EINVAL, offset)
    with pytest.raises(_lib.PzError) as e:
        wire.unwire_crystallized_state(raw)
    assert (e.value.code, e.value.offset) == (_lib.PZ_EINVAL, offset)
    # the same violation far from the start: behind validators that fill more than a tile
    filler = b"".join(uc.R(b"\x28" + wire.varint(1000 + i)) for i in range(1200))
    assert raw.startswith(uc.HEAD) and len(filler) > TILE
    moved = uc.HEAD + filler + raw[len(uc.HEAD):]
    assert cpu_verdict(moved) == (_lib.PZ_EINVAL, offset + len(filler))
    with pytest.raises(_lib.PzError) as e:
        wire.unwire_crystallized_state(moved)
    assert (e.value.code, e.value.offset) == (_lib.PZ_EINVAL, offset + len(filler))


# ---- 6: round trip ----------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def oracle_chain():
    """test_state_wire_gpu.test_the_states_of_the_oracle_chain's 130 blocks through the oracle: the blocks,
    the stored CrystallizedStates (genesis, after slots 64 and 128) and, for the reload, the chain's saved
    hashes and records as they stood when the state of slot 64 had become the chain's."""
    from test_attpool_gpu import late_chain

    blocks = late_chain(1024, 136, seed=4)
    chain = oreplay.Chain(1024)
    stored, at_reload = [ref.marshal(chain.C)], None
    for i, blk in enumerate(blocks[:130]):
        r = chain.process_block(oreplay.to_pb_block(blk))
        assert r["status"] == "processed"
        if r["transition"]:
            stored.append(ref.marshal(chain.candidate[2]))
        if i == 64:  # block 64 promoted the transition block's states
            assert ref.marshal(chain.C) == stored[1]
            at_reload = sorted(chain.saved)
    assert len(stored) == 3 and len(set(stored)) == 3
    return blocks, stored, at_reload


def round_trip(raw, hash_stride=32):
    state = ResidentRecalcState.from_state(raw, hash_stride=hash_stride)
    assert state.wire(state.field12, **state.rest) == raw
    assert state.root(state.field12, **state.rest) == hashlib.blake2b(raw).digest()[:32]
    return state


@pytest.mark.parametrize("which", (0, 1, 2))
def test_the_stored_states_of_the_oracle_chain_load_and_store_back(which):
    raw = oracle_chain()[1][which]
    state = round_trip(raw)
    cs = uc.parse(raw)
    assert state.nval == 1024 and state.nrec == len(cs.crosslink_records) and state.narr == len(cs.shard_and_committees_for_slots)
    assert tuple(getattr(state, k) for k in state._SCALARS) == tuple(getattr(cs, k) for k in state._SCALARS)


def test_a_state_whose_validators_carry_every_field_loads_and_stores_back():
    recs = [pb.CrosslinkRecord(i, bytes([i]) * (i % 49), 3 * i) for i in range(60)]
    tab = [[(a, list(range(a, 2000, 64)))] for a in range(64)]
    raw = uc.state(uc.mixed_validators(2000, seed=21), uc.arrays_of(tab), recs, crosslinking_start_shard=9, dynasty_seed=b"\x01" * 32,
                   dynasty_seed_last_reset=5, justified_streak=2)
    state = round_trip(raw, hash_stride=48)
    assert state.withdrawal_address.numel() > 10000 and state.randao_commitment.numel() > 10000
    loaded(raw)


# ---- 7: reload and go on ----------------------------------------------------------------------------------------
def test_a_reloaded_chain_goes_on_as_the_oracles():
    """The state stored after the first transition, reloaded into oracle.replay.Chain.reload and into
    ResidentChain.from_state with the hashes saved by then; the next 70 blocks, through the transition
    at slot 128, on both: statuses, digests, cache, pool, ring, saved set, scalars, records, balances
    and both roots (test_blockcycle_gpu's checks).  The engine reloads the same bytes to the same bytes."""
    from test_blockcycle_gpu import check_chain, check_outs

    blocks, stored, saved = oracle_chain()
    raw, nxt = stored[1], blocks[65:135]
    chain = oreplay.Chain.reload(raw, saved)
    rc = bc.ResidentChain.from_state(raw, saved)
    recs = [chain.process_block(oreplay.to_pb_block(b)) for b in nxt]
    assert [j for j, r in enumerate(recs) if r["transition"]] == [62] and {r["status"] for r in recs} == {"processed"}
    data, offs = bc.serialize_blocks(nxt)
    outs = rc.process_all(data, offs, want_digests=True)
    check_outs(outs, recs, nxt)
    check_chain(chain, rc)
    assert bc.BeaconChain.from_state(raw, saved).state_bytes("chain_crystallized") == raw


# ---- 8: argument checks -----------------------------------------------------------------------------------------
def test_argument_errors_are_einval_before_any_launch():
    import torch

    dev = torch.device("cuda", 0)
    raw = np.frombuffer(uc.state(uc.mixed_validators(4), uc.arrays_of(SMALL_TAB)), np.uint8)
    d = torch.from_numpy(raw.copy()).to(dev)
    dll, sh = _lib.lib.dll, _lib.stream_ptr(dev)
    scr = torch.zeros(int(dll.pz_cstate_scratch_bytes(raw.size)) + 16, dtype=torch.uint8, device=dev)
    result = torch.full((_lib.CSF_COUNT,), -99, dtype=torch.int64, device=dev)
    body = wire.cstate_head(raw)["body_beg"]
    frame = dll.pz_dev_cstate_frame
    assert frame(None, raw.size, body, scr.data_ptr(), result.data_ptr(), sh) == _lib.PZ_EINVAL
    assert frame(d.data_ptr(), raw.size, body, None, result.data_ptr(), sh) == _lib.PZ_EINVAL
    assert frame(d.data_ptr(), raw.size, body, scr.data_ptr() + 8, result.data_ptr(), sh) == _lib.PZ_EINVAL
    assert frame(d.data_ptr(), raw.size, body, scr.data_ptr(), None, sh) == _lib.PZ_EINVAL
    assert frame(d.data_ptr(), raw.size, raw.size + 1, scr.data_ptr(), result.data_ptr(), sh) == _lib.PZ_EINVAL
    outs = {k: torch.full((64,), SENTINEL, dtype=torch.uint8, device=dev) for k in wire.VALIDATOR_COLS + wire.TABLE_COLS}
    v = _lib.ValidatorColsOut(*[outs[k].data_ptr() for k in wire.VALIDATOR_COLS])
    t = _lib.CommitteeTableOut(narr=2, ncomm=2, **{k: outs[k].data_ptr() for k in wire.TABLE_COLS})
    status = torch.full((2,), -99, dtype=torch.int64, device=dev)
    decode = dll.pz_dev_cstate_decode
    good = [d.data_ptr(), raw.size, scr.data_ptr(), ctypes.byref(v), ctypes.byref(t), status.data_ptr(), sh]
    for k, bad in ((0, None), (2, None), (2, scr.data_ptr() + 8), (3, None), (4, None), (5, None)):
        assert decode(*[bad if j == k else a for j, a in enumerate(good)]) == _lib.PZ_EINVAL, k
    for k in wire.VALIDATOR_COLS:
        nul = _lib.ValidatorColsOut.from_buffer_copy(v)
        setattr(nul, k, None)
        assert decode(*[ctypes.byref(nul) if j == 3 else a for j, a in enumerate(good)]) == _lib.PZ_EINVAL, k
    for k in wire.TABLE_COLS:
        nul = _lib.CommitteeTableOut.from_buffer_copy(t)
        setattr(nul, k, None)
        assert decode(*[ctypes.byref(nul) if j == 4 else a for j, a in enumerate(good)]) == _lib.PZ_EINVAL, k
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [-99] * _lib.CSF_COUNT and status.cpu().tolist() == [-99, -99]  # no refused call launched anything
    assert all((o.cpu().numpy() == SENTINEL).all() for o in outs.values())
    # len == 0: zeros, nothing launched, the bytes may be NULL
    assert frame(None, 0, 0, scr.data_ptr(), result.data_ptr(), sh) == _lib.PZ_OK
    assert decode(None, 0, scr.data_ptr(), ctypes.byref(v), ctypes.byref(t), status.data_ptr(), sh) == _lib.PZ_OK
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [0] * _lib.CSF_COUNT and status.cpu().tolist() == [0, 0]
    assert all((o.cpu().numpy() == SENTINEL).all() for o in outs.values())
    # sizes that are not the frame's: refused on the device, nothing written
    assert frame(d.data_ptr(), raw.size, body, scr.data_ptr(), result.data_ptr(), sh) == _lib.PZ_OK
    wrong = _lib.CommitteeTableOut.from_buffer_copy(t)
    wrong.ncomm = 1
    assert decode(*[ctypes.byref(wrong) if j == 4 else a for j, a in enumerate(good)]) == _lib.PZ_OK
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [_lib.PZ_EINVAL, 0] and all((o.cpu().numpy() == SENTINEL).all() for o in outs.values())
