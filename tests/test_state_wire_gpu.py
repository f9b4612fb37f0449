"""The two states' proto3 bytes and roots from the device-resident objects (prysm_amd/csrc/wire_state.hip):
pz_dev_wire_committees / pz_wire_committees, pz_dev_crystallized_state_bytes / pz_crystallized_state_read
and pz_dev_active_state_bytes / pz_active_state_read against tests/state_wire_cases.py's expected bytes
(pinned to the protobuf runtime by tests/test_state_wire_cases.py), with the write extent checked byte by
byte round every output; the whole states on the 130-block oracle chain, a synthetic state with inactive
validators, the reload through the engine, the sticky errors and the refusals."""
import ctypes
import functools

import numpy as np
import pytest

import state_wire_cases as sc
from oracle import ref
from oracle import replay as oreplay
from prysm_amd import _lib, pb, synth, wire
from prysm_amd import blockchain as bc
from prysm_amd.pending import DevicePendingAttestations, ResidentRecalcState
from prysm_amd.votes import DeviceVoteCache
from test_attpool_gpu import as_pb, late_chain, pool_for, rec, table
from test_recalc_gpu import pools_for, states_for, synthetic
from test_votecache_gpu import put, rand_hashes

pytestmark = pytest.mark.gpu

U64 = np.uint64
GUARD = 0xA5
LEAD = 16        # guard bytes before the 16-byte aligned address the offsets count from
OFFSETS = (0, 1, 15)
TABLES = {c.name: c for c in sc.table_cases()}
HEADS = {c.name: c for c in sc.head_cases()}
RECENTS = {c.name: c for c in sc.recent_cases()}


def dll():
    return _lib.lib.dll


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(nbytes, offset):
    """A device buffer of guard bytes and the address ``offset`` bytes past a 16-byte aligned one."""
    import torch
    buf = torch.full((LEAD + offset + nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + LEAD + offset


def garbage(nbytes):
    """Scratch pre-filled with garbage, 16-byte aligned."""
    import torch
    t = torch.randint(0, 256, (max(int(nbytes), 16),), dtype=torch.uint8, device="cuda:0")
    assert t.data_ptr() % 16 == 0
    return t


def only(buf, offset, begin, length, want):
    """buf holds ``want`` at [begin, begin + length) past the output address and the guard everywhere else."""
    host = buf.cpu().numpy()
    at = LEAD + offset + begin
    assert length == len(want)
    assert host[at:at + length].tobytes() == want
    assert (host[:at] == GUARD).all() and (host[at + length:] == GUARD).all()


# ---- 1: ShardAndCommitteesForSlots ---------------------------------------------------------------------
def device_table(cols):
    d = {k: put(cols[k]) for k in wire.TABLE_COLS}
    return d, wire._table_struct(d, _lib.dptr)


def committees(case, offset, field=12, members_cap=None, nentries=None, cols=None):
    import torch

    cols = case.columns() if cols is None else cols
    nentries = case.nentries if nentries is None else nentries
    cap = case.members_total if members_cap is None else members_cap
    keep, t = device_table(cols)
    buf, d_out = guarded(dll().pz_wire_committees_bound(t.narr, nentries, cap), offset)
    scr = garbage(dll().pz_wire_committees_scratch_bytes(t.narr, nentries, cap))
    result = torch.full((2,), -99, dtype=torch.int64, device="cuda:0")
    rc = dll().pz_dev_wire_committees(ctypes.byref(t), nentries, cap, field, d_out, result.data_ptr(), scr.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, buf, [int(x) for x in result.cpu()]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", list(TABLES))
def test_committees_device_form(name, offset):
    case = TABLES[name]
    rc, buf, (length, status) = committees(case, offset)
    assert rc == _lib.PZ_OK and status == _lib.PZ_OK
    only(buf, offset, 0, length, case.expected)


@pytest.mark.parametrize("name", list(TABLES))
def test_committees_host_form(name):
    case = TABLES[name]
    assert wire.committees_device(case.columns()) == case.expected
    if name in ("shards", "genesis_1024"):
        assert wire.committees_device(case.pb()) == case.expected


@pytest.mark.parametrize("field", (0, 1, 16, (1 << 29) - 1))
def test_committees_follow_the_framing_rule_of_the_other_encoders(field):
    case = TABLES["member_edges"]
    bodies = [wire.shard_and_committee_array(a) for a in case.pb()]
    want = b"".join((wire.varint((field << 3) | 2) + wire.varint(len(b)) if field else b"") + b for b in bodies)
    rc, buf, (length, status) = committees(case, 1, field=field)
    assert (rc, status) == (_lib.PZ_OK, _lib.PZ_OK)
    only(buf, 1, 0, length, want)
    assert wire.committees_device(case.columns(), field_num=field) == want


def test_committees_with_a_slack_members_cap_and_the_python_device_face():
    case = TABLES["sizes"]
    rc, buf, (length, status) = committees(case, 15, members_cap=case.members_total + 1000)
    assert (rc, status) == (_lib.PZ_OK, _lib.PZ_OK)
    only(buf, 15, 0, length, case.expected)
    keep, _ = device_table(case.columns())
    out, result = wire.committees_device(keep)
    length, status = (int(x) for x in result.cpu())
    assert status == 0 and out[:length].cpu().numpy().tobytes() == case.expected
    shared = TABLES["shared"]  # entries share committees: the member sum exceeds the number of members
    keep, _ = device_table(shared.columns())
    assert int(wire.committees_device(keep)[1].cpu()[1]) == _lib.PZ_ERANGE
    out, result = wire.committees_device(keep, members_cap=shared.members_total)
    length, status = (int(x) for x in result.cpu())
    assert status == 0 and out[:length].cpu().numpy().tobytes() == shared.expected


def test_committees_table_errors_leave_the_output_alone():
    case = TABLES["shared"]
    for kw, code in ((dict(members_cap=case.members_total - 1), _lib.PZ_ERANGE), (dict(nentries=case.nentries - 1), _lib.PZ_ERANGE)):
        rc, buf, (length, status) = committees(case, 1, **kw)
        assert (rc, length, status) == (_lib.PZ_OK, 0, code), kw
        assert (buf.cpu().numpy() == GUARD).all(), kw
    cols = case.columns()
    cols["arr_comm"][2] = len(cols["coffs"]) - 1  # == ncomm
    rc, buf, (length, status) = committees(case, 1, cols=cols)
    assert (rc, length, status) == (_lib.PZ_OK, 0, _lib.PZ_EINDEX)
    assert (buf.cpu().numpy() == GUARD).all()
    # the host form returns the table's status
    t = wire._table_struct(cols, _lib.ptr)
    out, n = np.full(4096, GUARD, np.uint8), ctypes.c_uint64(7)
    assert dll().pz_wire_committees(ctypes.byref(t), case.nentries, 12, out.ctypes.data, out.size, ctypes.byref(n)) == _lib.PZ_EINDEX
    good = case.columns()  # (kept: the struct holds addresses only)
    t = wire._table_struct(good, _lib.ptr)
    assert dll().pz_wire_committees(ctypes.byref(t), case.nentries - 1, 12, out.ctypes.data, out.size, ctypes.byref(n)) == _lib.PZ_ERANGE
    assert (out == GUARD).all()
    # cap too small by one: PZ_ERANGE, *len set, out untouched
    want = case.expected
    assert dll().pz_wire_committees(ctypes.byref(t), case.nentries, 12, out.ctypes.data, len(want) - 1, ctypes.byref(n)) == _lib.PZ_ERANGE
    assert n.value == len(want) and (out == GUARD).all()
    assert dll().pz_wire_committees(ctypes.byref(t), case.nentries, 12, out.ctypes.data, len(want), ctypes.byref(n)) == _lib.PZ_OK
    assert out[:len(want)].tobytes() == want and (out[len(want):] == GUARD).all()


def test_a_decreasing_offset_is_found_without_any_entry():
    """No entries and 200 arrays, the one decreasing offset in the plan's second wave: the only barrier
    between the error word's initialisation and that lane's bit is the one that follows the initialisation."""
    import torch

    offs = np.zeros(201, U64)
    offs[100] = 1
    cols = {"arr_offs": offs, "arr_shard": np.zeros(0, U64), "arr_comm": np.zeros(0, np.uint32), "coffs": np.zeros(1, U64),
            "members": np.zeros(0, np.uint32)}
    keep, t = device_table(cols)
    for _ in range(4):
        buf, d_out = guarded(dll().pz_wire_committees_bound(200, 0, 0), 1)
        scr = garbage(dll().pz_wire_committees_scratch_bytes(200, 0, 0))
        result = torch.full((2,), -99, dtype=torch.int64, device="cuda:0")
        assert dll().pz_dev_wire_committees(ctypes.byref(t), 0, 0, 12, d_out, result.data_ptr(), scr.data_ptr(), stream()) == _lib.PZ_OK
        torch.cuda.synchronize()
        assert result.cpu().tolist() == [0, _lib.PZ_ERANGE] and (buf.cpu().numpy() == GUARD).all()


def test_committees_argument_errors_are_einval():
    import torch

    case = TABLES["shared"]
    keep, t = device_table(case.columns())
    n, cap = case.nentries, case.members_total
    buf, d_out = guarded(dll().pz_wire_committees_bound(t.narr, n, cap), 0)
    scr = garbage(dll().pz_wire_committees_scratch_bytes(t.narr, n, cap) + 16)
    result = torch.full((2,), -99, dtype=torch.int64, device="cuda:0")
    call, sh, r, s = dll().pz_dev_wire_committees, stream(), result.data_ptr(), scr.data_ptr()
    assert call(None, n, cap, 12, d_out, r, s, sh) == _lib.PZ_EINVAL
    assert call(ctypes.byref(t), n, cap, 12, d_out, None, s, sh) == _lib.PZ_EINVAL
    assert call(ctypes.byref(t), n, cap, 12, None, r, s, sh) == _lib.PZ_EINVAL
    assert call(ctypes.byref(t), n, cap, 12, d_out, r, None, sh) == _lib.PZ_EINVAL
    assert call(ctypes.byref(t), n, cap, 12, d_out, r, s + 8, sh) == _lib.PZ_EINVAL
    assert call(ctypes.byref(t), n, cap, 1 << 29, d_out, r, s, sh) == _lib.PZ_EINVAL
    assert call(ctypes.byref(t), n, 1 << 39, 12, d_out, r, s, sh) == _lib.PZ_EINVAL  # more chunks than the write grid covers
    assert call(ctypes.byref(t), (1 << 31) - 1, cap, 12, d_out, r, s, sh) == _lib.PZ_EINVAL
    for k in wire.TABLE_COLS:
        bad = _lib.CommitteeTable.from_buffer_copy(t)
        setattr(bad, k, None)
        assert call(ctypes.byref(bad), n, cap, 12, d_out, r, s, sh) == _lib.PZ_EINVAL, k
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all() and result.cpu().tolist() == [-99, -99]  # no refused call launched anything
    empty = _lib.CommitteeTable()  # narr == 0: length 0, d_out untouched and NULL
    assert call(ctypes.byref(empty), 0, 0, 12, None, r, None, sh) == _lib.PZ_OK
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [0, 0]


# ---- 2: the CrystallizedState ---------------------------------------------------------------------------
def resident_head(case, nval=0, seed=0):
    rng = np.random.default_rng(seed)
    bal = rng.integers(0, 1 << 40, size=nval, dtype=U64)
    start = rng.integers(0, 3, size=nval, dtype=U64)
    end = np.where(rng.random(nval) < 0.5, U64(ref.DEFAULT_END_DYNASTY), U64(0)).astype(U64)
    kw = dict(zip(sc.HEAD_SCALARS, case.values[:6]))
    state = ResidentRecalcState(bal, start, end, np.zeros(0, np.uint32), np.zeros(1, U64), case.records, hash_stride=case.stride, **kw)
    vals = pb.Validators(nval, balance=bal, start_dynasty=start, end_dynasty=end)
    return state, vals


def rest_of(case):
    r = _lib.CstateRest(crosslinking_start_shard=case.values[6], dynasty_seed_len=len(case.seed), dynasty_seed_last_reset=case.values[7])
    ctypes.memmove(r.dynasty_seed, case.seed, len(case.seed))
    return r


def cstate_device(state, rest, f12, offset):
    import torch

    n12 = int(f12.numel()) if f12 is not None else 0
    bound = dll().pz_crystallized_state_bound(state.nrec, state.hash_stride, state.nval, 0, n12)
    buf, d_out = guarded(bound, offset)
    scr = garbage(dll().pz_crystallized_state_scratch_bytes(state.nval))
    span = torch.full((2,), -99, dtype=torch.int64, device="cuda:0")
    cols = state.validator_cols()
    rc = dll().pz_dev_crystallized_state_bytes(state._h, ctypes.byref(rest), ctypes.byref(cols), state.nval, _lib.dptr(f12), n12,
                                               d_out, span.data_ptr(), scr.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, buf, [int(x) for x in span.cpu()]


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", list(HEADS))
def test_head_device_and_host_forms(name, offset):
    case = HEADS[name]
    state, _ = resident_head(case)
    rc, buf, (begin, length) = cstate_device(state, rest_of(case), None, offset)
    assert rc == _lib.PZ_OK
    only(buf, offset, begin, length, case.expected)
    if offset == 0:
        assert state.wire(b"", case.values[6], case.seed, case.values[7]) == case.expected
        assert state.root(b"", case.values[6], case.seed, case.values[7]) == ref.hash32(case.expected)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("n12", (0, 1, 15, 16, 17, 33, 4097))
def test_head_validators_and_tail_meet(n12, offset):
    """300 validators between a head and a field 12 of every tail shape: under one 16-byte piece, one
    piece, a piece and an overlapping one, many."""
    case = HEADS["hash_lengths_48"]
    state, vals = resident_head(case, nval=300, seed=n12)
    f12 = np.random.default_rng(n12).integers(0, 256, size=n12, dtype=np.uint8)
    want = case.expected + wire.validators(vals) + f12.tobytes()
    d12 = put(f12) if n12 else None
    rc, buf, (begin, length) = cstate_device(state, rest_of(case), d12, offset)
    assert rc == _lib.PZ_OK
    only(buf, offset, begin, length, want)
    if offset == 1 and n12:
        shifted = put(np.concatenate([np.zeros(3, np.uint8), f12]))[3:]  # a field 12 at an odd address
        assert state.wire(shifted, case.values[6], case.seed, case.values[7]) == want


def test_crystallized_state_refusals():
    import torch

    case = HEADS["one_record"]
    state, vals = resident_head(case, nval=10)
    rest, cols = rest_of(case), state.validator_cols()
    want = case.expected + wire.validators(vals)
    out, n, root = np.full(len(want) + 8, GUARD, np.uint8), ctypes.c_uint64(0), np.zeros(32, np.uint8)
    read = dll().pz_crystallized_state_read
    rc = read(state._h, ctypes.byref(rest), ctypes.byref(cols), 10, None, 0, out.ctypes.data, len(want) - 1, ctypes.byref(n), root.ctypes.data)
    assert rc == _lib.PZ_ERANGE and n.value == len(want) and (out == GUARD).all()  # cap too small by one
    rc = read(state._h, ctypes.byref(rest), ctypes.byref(cols), 10, None, 0, out.ctypes.data, len(want), ctypes.byref(n), root.ctypes.data)
    assert rc == _lib.PZ_OK and out[:len(want)].tobytes() == want and (out[len(want):] == GUARD).all()
    assert root.tobytes() == ref.hash32(want)
    assert read(None, ctypes.byref(rest), ctypes.byref(cols), 10, None, 0, out.ctypes.data, out.size, ctypes.byref(n), None) == _lib.PZ_EINVAL
    assert read(state._h, None, ctypes.byref(cols), 10, None, 0, out.ctypes.data, out.size, ctypes.byref(n), None) == _lib.PZ_EINVAL
    assert read(state._h, ctypes.byref(rest), None, 10, None, 0, out.ctypes.data, out.size, ctypes.byref(n), None) == _lib.PZ_EINVAL
    assert read(state._h, ctypes.byref(rest), ctypes.byref(cols), 10, None, 5, out.ctypes.data, out.size, ctypes.byref(n), None) == _lib.PZ_EINVAL
    assert read(state._h, ctypes.byref(rest), ctypes.byref(cols), 10, None, 0, out.ctypes.data, out.size, None, None) == _lib.PZ_EINVAL
    long_seed = _lib.CstateRest(dynasty_seed_len=65)
    assert read(state._h, ctypes.byref(long_seed), ctypes.byref(cols), 10, None, 0, out.ctypes.data, out.size, ctypes.byref(n), None) == _lib.PZ_EINVAL
    buf, d_out = guarded(dll().pz_crystallized_state_bound(1, 32, 10, 0, 0), 0)
    scr = garbage(dll().pz_crystallized_state_scratch_bytes(10) + 16)
    span = torch.full((2,), -99, dtype=torch.int64, device="cuda:0")
    call, sh = dll().pz_dev_crystallized_state_bytes, stream()
    args = lambda **o: [o.get(k, v) for k, v in (("st", state._h), ("rest", ctypes.byref(rest)), ("v", ctypes.byref(cols)), ("n", 10),  # noqa: E731
                                                 ("f12", None), ("n12", 0), ("out", d_out), ("span", span.data_ptr()),
                                                 ("scr", scr.data_ptr()), ("sh", sh))]
    for bad in (dict(st=None), dict(rest=None), dict(v=None), dict(out=None), dict(span=None), dict(scr=None),
                dict(scr=scr.data_ptr() + 8), dict(n12=4), dict(rest=ctypes.byref(long_seed))):
        assert call(*args(**bad)) == _lib.PZ_EINVAL, list(bad)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GUARD).all() and span.cpu().tolist() == [-99, -99]


# ---- 3: the ActiveState ---------------------------------------------------------------------------------
@functools.lru_cache(None)
def pending():
    rng = np.random.default_rng(31)
    recs = [rec(rng, elems=(32,) * (i % 3), nsig=i % 2, bf=1 + i % 5) for i in range(37)]
    pool = pool_for(recs, slack=8)
    pool.append_host(wire.attestation_columns(recs), len(recs), np.zeros(len(recs), np.int32), np.arange(len(recs), dtype=np.uint32))
    return pool, recs


def active_device(pool, case, offset, short=0):
    import torch

    counts = pool.counts()
    cap = dll().pz_active_state_bound(counts.ctypes.data, len(case.rows)) - short
    buf, d_out = guarded(cap, offset)
    d_rows = put(case.rows) if len(case.rows) else None
    d_lens = put(np.ascontiguousarray(case.lens, np.uint8)) if case.lens is not None else None
    total = torch.full((1,), -99, dtype=torch.int64, device="cuda:0")
    rc = dll().pz_dev_active_state_bytes(pool._h, _lib.dptr(d_rows), _lib.dptr(d_lens), len(case.rows), d_out, cap, total.data_ptr(),
                                         stream())
    torch.cuda.synchronize()
    return rc, buf, int(total.cpu()[0])


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("filled", (False, True))
@pytest.mark.parametrize("name", list(RECENTS))
def test_active_state_device_and_host_forms(name, filled, offset):
    case = RECENTS[name]
    pool, recs = pending() if filled else (DevicePendingAttestations([4, 64, 64, 64, 4, 64, 4]), [])
    want = wire.active_state(pb.ActiveState(pending_attestations=recs, recent_block_hashes=case.hashes()))
    rc, buf, total = active_device(pool, case, offset)
    assert rc == _lib.PZ_OK
    only(buf, offset, 0, total, want)
    if offset == 0:
        assert pool.active_state(case.rows, case.lens) == want
        assert pool.active_state_root(case.rows, case.lens) == ref.hash32(want)


def test_active_state_refusals():
    import torch

    pool, recs = pending()
    case = RECENTS["mixed"]
    rc, buf, total = active_device(pool, case, 1, short=1)  # cap below the bound by one: nothing written
    assert rc == _lib.PZ_ERANGE and total == -99 and (buf.cpu().numpy() == GUARD).all()
    want = wire.active_state(pb.ActiveState(pending_attestations=recs, recent_block_hashes=case.hashes()))
    out, n = np.full(len(want) + 8, GUARD, np.uint8), ctypes.c_uint64(0)
    lens = np.ascontiguousarray(case.lens, np.uint8)
    read = dll().pz_active_state_read
    assert read(pool._h, case.rows.ctypes.data, lens.ctypes.data, 8, out.ctypes.data, len(want) - 1, ctypes.byref(n), None) == _lib.PZ_ERANGE
    assert n.value == len(want) and (out == GUARD).all()
    assert read(pool._h, case.rows.ctypes.data, lens.ctypes.data, 8, out.ctypes.data, len(want), ctypes.byref(n), None) == _lib.PZ_OK
    assert out[:len(want)].tobytes() == want and (out[len(want):] == GUARD).all()
    assert read(None, case.rows.ctypes.data, None, 8, out.ctypes.data, out.size, ctypes.byref(n), None) == _lib.PZ_EINVAL
    assert read(pool._h, None, None, 8, out.ctypes.data, out.size, ctypes.byref(n), None) == _lib.PZ_EINVAL
    assert read(pool._h, case.rows.ctypes.data, None, 8, out.ctypes.data, out.size, None, None) == _lib.PZ_EINVAL
    total = torch.full((1,), -99, dtype=torch.int64, device="cuda:0")
    call = dll().pz_dev_active_state_bytes
    assert call(None, None, None, 0, None, 0, total.data_ptr(), stream()) == _lib.PZ_EINVAL
    assert call(pool._h, None, None, 0, None, 0, None, stream()) == _lib.PZ_EINVAL
    assert call(pool._h, None, None, 8, None, 0, total.data_ptr(), stream()) == _lib.PZ_EINVAL


def test_a_pool_with_its_sticky_capacity_error_reports_it():
    rng = np.random.default_rng(32)
    recs = [rec(rng) for _ in range(3)]
    pool = pool_for(recs[:2])
    cols = lambda r: (wire.attestation_columns(r), len(r), np.zeros(len(r), np.int32), np.zeros(len(r), np.uint32))  # noqa: E731
    pool.append_host(*cols(recs[:2]))
    pool.append_host(*cols(recs[2:]))  # one row more than the pool holds: dropped whole, sticky
    case = RECENTS["one"]
    with pytest.raises(_lib.PzError) as e:
        pool.active_state(case.rows)
    assert e.value.code == _lib.PZ_ERANGE
    want = wire.active_state(pb.ActiveState(pending_attestations=recs[:2], recent_block_hashes=case.hashes()))
    assert pool.active_state(case.rows, strict=False) == want  # the output is written all the same
    rc, buf, total = active_device_lenient(pool, case)
    assert rc == _lib.PZ_ERANGE
    only(buf, 0, 0, total, want)


def active_device_lenient(pool, case):
    import torch

    counts = pool.counts(strict=False)
    cap = dll().pz_active_state_bound(counts.ctypes.data, len(case.rows))
    buf, d_out = guarded(cap, 0)
    total = torch.full((1,), -99, dtype=torch.int64, device="cuda:0")
    d_rows = put(case.rows)
    rc = dll().pz_dev_active_state_bytes(pool._h, d_rows.data_ptr(), None, len(case.rows), d_out, cap, total.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, buf, int(total.cpu()[0])


# ---- 4: the whole states ---------------------------------------------------------------------------------
def pb_cstate(C):
    """An oracle CrystallizedState as prysm_amd.pb's (the validators as columns)."""
    vs = C.validators
    for v in vs:
        assert not (v.public_key or v.withdrawal_shard or v.withdrawal_address or v.randao_commitment)
    vals = pb.Validators(len(vs), balance=[v.balance for v in vs], start_dynasty=[v.start_dynasty for v in vs],
                         end_dynasty=[v.end_dynasty for v in vs])
    arrs = [pb.ShardAndCommitteeArray([pb.ShardAndCommittee(e.shard_id, np.array(list(e.committee), np.uint32))
                                       for e in a.array_shard_and_committee]) for a in C.shard_and_committees_for_slots]
    return pb.CrystallizedState(C.last_state_recalc, C.justified_streak, C.last_justified_slot, C.last_finalized_slot,
                                C.current_dynasty, C.crosslinking_start_shard, C.total_deposits, bytes(C.dynasty_seed),
                                C.dynasty_seed_last_reset,
                                [pb.CrosslinkRecord(r.dynasty, bytes(r.blockhash), r.slot) for r in C.crosslink_records], vals, arrs)


def check_states(pool, state, A, C, device_table_too=False):
    """The resident objects' bytes and roots against the oracle's states A (active) and C."""
    rest = (C.crosslinking_start_shard, bytes(C.dynasty_seed), C.dynasty_seed_last_reset)
    f12 = wire.committees_device(table(C))
    got = state.wire(f12, *rest)
    assert got == wire.crystallized_state(pb_cstate(C)) == ref.marshal(C)
    assert state.root(f12, *rest) == ref.crystallized_state_hash(C)
    if device_table_too:  # field 12 straight from device columns, never on the host
        d = {k: put(v) for k, v in wire.committee_table(table(C)).items()}
        assert state.wire(wire.committees_device(d), *rest) == got
    raw = [bytes(h) for h in A.recent_block_hashes]
    lens = np.array([len(h) for h in raw], np.uint8)
    a_pb = pb.ActiveState([as_pb(a) for a in A.pending_attestations], raw)
    assert pool.active_state(raw, lens) == wire.active_state(a_pb) == ref.marshal(A)
    assert pool.active_state_root(raw, lens) == ref.active_state_hash(A)
    assert bc.resident_state_roots(pool, state, raw, f12, lens, *rest) == (ref.active_state_hash(A), ref.crystallized_state_hash(C))
    return got


def genesis_resident(cs0):
    tab0 = table(cs0)
    args = ([v.balance for v in cs0.validators], [v.start_dynasty for v in cs0.validators],
            [v.end_dynasty for v in cs0.validators], [v for arr in tab0 for e in arr for v in e[1]],
            bc._committee_table(tab0)[3], cs0.crosslink_records)
    kw = dict(last_state_recalc=cs0.last_state_recalc, justified_streak=cs0.justified_streak,
              last_justified_slot=cs0.last_justified_slot, last_finalized_slot=cs0.last_finalized_slot,
              current_dynasty=cs0.current_dynasty, total_deposits=cs0.total_deposits)
    return ResidentRecalcState(*args, **kw), tab0


CAPS = [256, 256 * 32, 256 * 32, 256 * 8, 256, 256 * 32, 512]


def test_the_states_of_the_oracle_chain():
    """test_recalc_gpu.test_the_chain_through_the_resident_call's 130 blocks at 1,024 validators: at
    genesis, after the transition at slot 64 and after the one at slot 128 the resident objects' bytes
    and roots are the oracle's; the engine reloads the stored CrystallizedState and gives it back."""
    nval, nblocks = 1024, 130
    blocks = late_chain(nval, nblocks, seed=4)
    data, offs = bc.serialize_blocks(blocks)
    chain = oreplay.Chain(nval)
    state, _ = genesis_resident(chain.C)
    pool, cache = DevicePendingAttestations(CAPS), DeviceVoteCache(nval, 512)
    A0 = chain.A.data
    assert {len(h) for h in A0.recent_block_hashes} == {0}  # recent_len all 0 at genesis
    stored = [check_states(pool, state, A0, chain.C, device_table_too=True)]
    tables = {}
    lsr = chain.C.last_state_recalc
    for i, blk in enumerate(blocks):
        C, A = chain.C, chain.A.data
        if C.last_state_recalc not in tables:
            tables[C.last_state_recalc] = table(C)
        transition = blk.slot_number >= lsr + 64
        if transition:
            recent = [bytes(h) for h in chain.candidate[1].data.recent_block_hashes]
            bc.state_recalc_resident(pool, cache, state, recent, blk.slot_number)
            lsr += 64
        lo, hi = int(offs[i]), int(offs[i + 1])
        report, _, status = bc.tally_serialized_blocks(
            cache, data[lo:hi], np.array([0, hi - lo], dtype=U64), C.last_justified_slot, C.last_state_recalc,
            len(A.recent_block_hashes), tables[C.last_state_recalc], [bytes(h) for h in A.recent_block_hashes],
            np.array([v.balance for v in C.validators], U64), pending=pool, candidate=[1])
        assert list(report) == [bc.BLOCK_TALLIED] and (status == 0).all(), i
        r = chain.process_block(oreplay.to_pb_block(blk))
        assert r["status"] == "processed" and r["transition"] == transition, i
        if transition:
            _, A1, C1 = chain.candidate
            stored.append(check_states(pool, state, A1.data, C1))
    assert len(stored) == 3 and len(set(stored)) == 3
    for raw in (stored[0], stored[2]):
        assert bc.BeaconChain.from_state(raw).state_bytes("chain_crystallized") == raw


def test_a_synthetic_state_with_inactive_validators():
    """5,000 validators, some not active, records of several hash lengths under stride 48: after one
    state_recalc_resident the bytes are the encoding of state_recalc_device's twin."""
    inst, recs = synthetic(5000, True, (32, 48, 33, 1))
    model, state = states_for(inst, hash_stride=48, last_state_recalc=31)
    pool_m, pool = pools_for(inst, recs)
    recent = rand_hashes(np.random.default_rng(3), 64)
    bc.state_recalc_device(pool_m, None, model, recent, 1234)
    bc.state_recalc_resident(pool, None, state, recent, 1234)
    coffs = inst["coffs"].astype(np.int64)
    ncomm = len(coffs) - 1
    arrs = [pb.ShardAndCommitteeArray([pb.ShardAndCommittee(c % 1024, inst["committee"][coffs[c]:coffs[c + 1]].astype(np.uint32))
                                       for c in range(a, ncomm, 64)]) for a in range(64)]
    f12 = wire.committees_device(arrs)
    vals = pb.Validators(5000, balance=model.balances(), start_dynasty=inst["start"][0], end_dynasty=inst["end"][0])
    twin = pb.CrystallizedState(model.last_state_recalc, model.justified_streak, model.last_justified_slot, model.last_finalized_slot,
                                model.current_dynasty, 5, model.total_deposits, b"\x01" * 32, 9, model.crosslink_records, vals, arrs)
    want = wire.crystallized_state(twin)
    assert len({len(r.blockhash) for r in model.crosslink_records}) > 3 and (inst["start"][0] == 7).any()
    assert state.wire(f12, 5, b"\x01" * 32, 9) == want
    assert state.root(f12, 5, b"\x01" * 32, 9) == ref.hash32(want)
    rows = [r for r in recs if r.slot > 31]
    assert pool.active_state(recent) == wire.active_state(pb.ActiveState(rows, recent))


def test_after_the_rewards_panic_the_bytes_are_the_state_before_it():
    """test_recalc_gpu's small chain at full participation: stateRecalc panics at the block of slot 64;
    the read form returns PZ_EINDEX and the bytes it filled are the pre-panic state's."""
    nval = 1024
    blocks = synth.chain_blocks(nval, 64, seed=2, participation=(1.0, 0.5))
    chain = oreplay.Chain(nval)
    cs0 = chain.C
    state, tab0 = genesis_resident(cs0)
    data, offs = bc.serialize_blocks(blocks[:63])
    pool = DevicePendingAttestations(CAPS)
    bc.pend_serialized_blocks(pool, data, offs, cs0.last_justified_slot, cs0.last_state_recalc, len(chain.A.data.recent_block_hashes), tab0)
    f12 = wire.committees_device(tab0)
    before = state.wire(f12)
    assert before == ref.marshal(cs0)
    with pytest.raises(bc.ChainPanic):
        bc.state_recalc_resident(pool, None, state, rand_hashes(np.random.default_rng(1), 64), 64)
    with pytest.raises(_lib.PzError) as e:
        state.wire(f12)
    assert e.value.code == _lib.PZ_EINDEX
    assert state.wire(f12, strict=False) == before
    assert state.root(f12, strict=False) == ref.crystallized_state_hash(cs0)
