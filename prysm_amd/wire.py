"""proto3 wire encoder for the hashed messages (host side; what ``proto.Marshal`` produces).

Restates the golang/protobuf v1.1 table marshaller's proto3 rules as used at
types/block.go:69, types/attestation.go:51 and (via gogo, same generated code)
types/state.go:141,240:
  * fields in ascending field-number order;
  * zero scalars and empty ``bytes`` scalars are omitted;
  * every element of a ``repeated bytes`` is emitted, empty ones as ``tag 00``;
  * a non-nil message field is emitted even when empty (``Timestamp{0,0}`` -> ``3a 00``);
  * ``repeated uint32/uint64`` are packed and omitted when empty;
  * negative int32/int64 are 10-byte varints (sign-extended to 64 bits).
Validators and committees are encoded with numpy (one vectorised pass per field) so a
1M-validator CrystallizedState serialises in well under a second.
"""
import numpy as np

from prysm_amd import pb

_U64 = np.uint64
M64 = (1 << 64) - 1


def varint(x):
    x &= M64
    out = bytearray()
    while x >= 0x80:
        out.append((x & 0x7F) | 0x80)
        x >>= 7
    out.append(x)
    return bytes(out)


def _tag(num, wt):
    return varint((num << 3) | wt)


def _u(num, v):
    return _tag(num, 0) + varint(v) if v else b""


def _b(num, v):
    return _tag(num, 2) + varint(len(v)) + bytes(v) if v else b""


def _msg(num, body):
    return _tag(num, 2) + varint(len(body)) + body


def _packed(num, values):
    if len(values) == 0:
        return b""
    if len(values) <= 64 and not isinstance(values, np.ndarray):  # short lists: scalar path
        body = b"".join(varint(int(v)) for v in values)
    else:
        body = packed_varints(np.asarray(values, dtype=_U64))
    return _tag(num, 2) + varint(len(body)) + body


# ---- vectorised varints ---------------------------------------------------------------------
def varint_len(x):
    """Per-element varint byte length of a uint64 array (0 -> 1)."""
    x = np.asarray(x, dtype=_U64)
    n = np.ones(x.shape, dtype=np.int64)
    for k in range(1, 10):
        n += (x >= _U64(1 << (7 * k))).astype(np.int64)
    return n


def _scatter_varints(out, pos, x, nbytes):
    """Write varint(x[i]) at out[pos[i]:pos[i]+nbytes[i]] (vectorised over bytes)."""
    x = x.astype(_U64).copy()
    for k in range(int(nbytes.max()) if nbytes.size else 0):
        live = nbytes > k
        more = nbytes > k + 1
        b = (x & _U64(0x7F)).astype(np.uint8) | np.where(more, 0x80, 0).astype(np.uint8)
        out[(pos + k)[live]] = b[live]
        x >>= _U64(7)


def packed_varints(values):
    values = np.asarray(values, dtype=_U64)
    nb = varint_len(values)
    pos = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int64)
    out = np.zeros(int(nb.sum()), dtype=np.uint8)
    _scatter_varints(out, pos, values, nb)
    return out.tobytes()


# ---- messages ------------------------------------------------------------------------------
def timestamp(t):
    return _u(1, t.seconds & M64) + _u(2, t.nanos & M64)


def attestation_record(a):
    """messages.proto:110-119."""
    out = [_u(1, a.slot), _u(2, a.shard_id), _u(3, a.justified_slot), _b(4, a.justified_block_hash),
           _b(5, a.shard_block_hash), _b(6, a.attester_bitfield)]
    out += [_msg(7, bytes(h)) for h in a.oblique_parent_hashes]  # repeated bytes: every element
    out.append(_packed(8, a.aggregate_sig))
    return b"".join(out)


def beacon_block(b):
    """messages.proto:37-46."""
    out = [_b(1, b.parent_hash), _u(2, b.slot_number), _b(3, b.randao_reveal), _b(4, b.pow_chain_ref),
           _b(5, b.active_state_hash), _b(6, b.crystallized_state_hash)]
    if b.timestamp is not None:
        out.append(_msg(7, timestamp(b.timestamp)))
    out += [_msg(8, attestation_record(a)) for a in b.attestations]
    return b"".join(out)


def active_state(s):
    """messages.proto:94-97."""
    out = [_msg(1, attestation_record(a)) for a in s.pending_attestations]
    out += [_msg(2, bytes(h)) for h in s.recent_block_hashes]
    return b"".join(out)


def crosslink_record(r):
    return _u(1, r.dynasty) + _b(2, r.blockhash) + _u(3, r.slot)


def shard_and_committee(sc):
    return _u(1, sc.shard_id) + _packed(2, sc.committee)


def shard_and_committee_array(arr):
    return b"".join(_msg(1, shard_and_committee(sc)) for sc in arr.array_shard_and_committee)


def validators(v, field_num=11):
    """Every ValidatorRecord of a ``pb.Validators`` block, each framed as repeated message
    ``field_num`` (CrystallizedState.validators = 11), vectorised over records."""
    n = len(v)
    if n == 0:
        return b""
    if v.withdrawal_address is not None or v.randao_commitment is not None:
        return b"".join(_msg(field_num, _validator_scalar(v, i)) for i in range(n))
    fields = [(1, v.public_key), (2, v.withdrawal_shard), (5, v.balance), (6, v.start_dynasty),
              (7, v.end_dynasty)]
    lens = []
    body = np.zeros(n, dtype=np.int64)
    for num, x in fields:
        nb = np.where(x != 0, varint_len(x), 0)
        lens.append(nb)
        body += np.where(x != 0, 1 + nb, 0)  # single-byte tags (fields 1..15)
    frame = 1 + varint_len(body.astype(_U64))  # tag 0x5a + length varint
    total = frame + body
    start = np.concatenate([[0], np.cumsum(total)[:-1]]).astype(np.int64)
    out = np.zeros(int(total.sum()), dtype=np.uint8)
    out[start] = (field_num << 3) | 2
    _scatter_varints(out, start + 1, body.astype(_U64), frame - 1)
    pos = start + frame
    for (num, x), nb in zip(fields, lens):
        present = x != 0
        out[pos[present]] = (num << 3) | 0
        _scatter_varints(out, (pos + 1)[present], x[present], nb[present])
        pos = pos + np.where(present, 1 + nb, 0)
    return out.tobytes()


def _validator_scalar(v, i):
    wa = v.withdrawal_address[i] if v.withdrawal_address is not None else b""
    rc = v.randao_commitment[i] if v.randao_commitment is not None else b""
    return (_u(1, int(v.public_key[i])) + _u(2, int(v.withdrawal_shard[i])) + _b(3, wa) + _b(4, rc) +
            _u(5, int(v.balance[i])) + _u(6, int(v.start_dynasty[i])) + _u(7, int(v.end_dynasty[i])))


def crystallized_state(s):
    """messages.proto:59-72."""
    out = [_u(1, s.last_state_recalc), _u(2, s.justified_streak), _u(3, s.last_justified_slot),
           _u(4, s.last_finalized_slot), _u(5, s.current_dynasty), _u(6, s.crosslinking_start_shard),
           _u(7, s.total_deposits), _b(8, s.dynasty_seed), _u(9, s.dynasty_seed_last_reset)]
    out += [_msg(10, crosslink_record(r)) for r in s.crosslink_records]
    out.append(validators(s.validators))
    out += [_msg(12, shard_and_committee_array(a)) for a in s.shard_and_committees_for_slots]
    return b"".join(out)


# ---- device encoder (prysm_amd/csrc/wire.hip) ------------------------------------------------
def _csr(blobs, n):
    if blobs is None:
        return None, None
    offs = np.zeros(n + 1, dtype=_U64)
    offs[1:] = np.cumsum([len(b) for b in blobs], dtype=_U64)
    data = np.frombuffer(b"".join(bytes(b) for b in blobs) + b"\0", dtype=np.uint8)
    return data, offs


def validators_device(v, field_num=11, with_offsets=False):
    """The same bytes as :func:`validators`, encoded on the GPU by ``pz_wire_validators``
    (size / scan / write kernels over the SoA columns).  ``field_num=0`` gives
    bare records; ``with_offsets`` also returns each record's start (n+1 offsets)."""
    from prysm_amd import _lib

    n = len(v)
    wa, wa_offs = _csr(v.withdrawal_address, n)
    rc, rc_offs = _csr(v.randao_commitment, n)
    cols = _lib.ValidatorCols(
        _lib.ptr(v.public_key), _lib.ptr(v.withdrawal_shard), _lib.ptr(wa), _lib.ptr(wa_offs),
        _lib.ptr(rc), _lib.ptr(rc_offs), _lib.ptr(v.balance), _lib.ptr(v.start_dynasty),
        _lib.ptr(v.end_dynasty))
    nbytes = (int(wa_offs[-1]) if wa_offs is not None else 0) + (int(rc_offs[-1]) if rc_offs is not None else 0)
    cap = int(_lib.lib.dll.pz_wire_validators_bound(n, nbytes))
    out = np.empty(max(cap, 1), dtype=np.uint8)
    offs = np.empty(n + 1, dtype=_U64) if with_offsets else None
    length = _lib.ctypes.c_uint64(0)
    _lib.lib.call("pz_wire_validators", _lib.ctypes.byref(cols), n, field_num, _lib.ptr(out), cap,
                  _lib.ptr(offs), _lib.ctypes.byref(length))
    raw = out[:length.value].tobytes()
    return (raw, offs) if with_offsets else raw


ATT_COLS = ("slot", "shard_id", "justified_slot", "justified_block_hash", "justified_block_hash_offs",
            "shard_block_hash", "shard_block_hash_offs", "attester_bitfield", "attester_bitfield_offs",
            "oblique_parent_hashes", "oblique_offs", "oblique_first", "aggregate_sig", "aggregate_sig_first")


def attestation_columns(atts):
    """pb.AttestationRecord list -> the SoA / CSR columns of ``pz_attestation_cols``."""
    n = len(atts)
    cols = {k: np.ascontiguousarray([getattr(a, k) for a in atts], dtype=_U64)
            for k in ("slot", "shard_id", "justified_slot")}
    for k in ("justified_block_hash", "shard_block_hash", "attester_bitfield"):
        cols[k], cols[k + "_offs"] = _csr([bytes(getattr(a, k)) for a in atts], n)
    elems = [bytes(h) for a in atts for h in a.oblique_parent_hashes]
    cols["oblique_parent_hashes"], cols["oblique_offs"] = _csr(elems, len(elems))
    cols["oblique_first"] = np.zeros(n + 1, dtype=_U64)
    cols["oblique_first"][1:] = np.cumsum([len(a.oblique_parent_hashes) for a in atts])
    cols["aggregate_sig"] = np.ascontiguousarray([v & M64 for a in atts for v in a.aggregate_sig] or [0], dtype=_U64)
    cols["aggregate_sig_first"] = np.zeros(n + 1, dtype=_U64)
    cols["aggregate_sig_first"][1:] = np.cumsum([len(a.aggregate_sig) for a in atts])
    return cols


def attestations_device(cols, n, field_num=0):
    """AttestationRecords encoded on the GPU by ``pz_wire_attestations`` from columns (see
    :func:`attestation_columns`).  Returns (bytes, offsets[n+1]); with ``field_num=0`` the
    records are bare, as Attestation.Hash() hashes them."""
    from prysm_amd import _lib

    c = _lib.att_cols(cols)
    nbytes = sum(int(cols[k][-1]) for k in ("justified_block_hash_offs", "shard_block_hash_offs",
                                            "attester_bitfield_offs", "oblique_offs")) if n else 0
    ne = int(cols["oblique_first"][-1]) if n else 0
    ns = int(cols["aggregate_sig_first"][-1]) if n else 0
    cap = int(_lib.lib.dll.pz_wire_attestations_bound(n, nbytes, ne, ns))
    out = np.empty(max(cap, 1), dtype=np.uint8)
    offs = np.empty(n + 1, dtype=_U64)
    length = _lib.ctypes.c_uint64(0)
    _lib.lib.call("pz_wire_attestations", _lib.ctypes.byref(c), n, field_num, _lib.ptr(out), cap, _lib.ptr(offs),
                  _lib.ctypes.byref(length))
    return out[:length.value].tobytes(), offs


# ---- device decoder (prysm_amd/csrc/unwire.hip) ----------------------------------------------
ATT_OUT_COLS = ATT_COLS + ("n_oblique", "last_byte", "status")
BLOCK_COLS = ("slot_number", "ts_seconds", "ts_nanos", "has_timestamp", "bytes_beg", "bytes_len", "att_first",
              "att_beg", "att_end", "att_block_slot", "att_block", "status")
_BYTES_COLS = ("justified_block_hash", "shard_block_hash", "attester_bitfield", "oblique_parent_hashes")
_ATT_DTYPES = {"last_byte": np.uint8, "status": np.int32}
_BLOCK_DTYPES = {"ts_seconds": np.int64, "ts_nanos": np.int64, "has_timestamp": np.uint8, "bytes_len": np.uint32,
                 "att_block": np.uint32, "status": np.int32}


def att_sizes(n, totals):
    """Entries of every ``ATT_COLS`` column for n rows and the six totals in the header's order
    (three bytes columns, elements, element bytes, sig values)."""
    jb, sb, bf, ne, eb, ns = (int(x) for x in totals[:6])
    size = {k: n + 1 if k.endswith(("_offs", "_first")) else n for k in ATT_COLS}
    size.update(justified_block_hash=jb, shard_block_hash=sb, attester_bitfield=bf, oblique_parent_hashes=eb,
                oblique_offs=ne + 1, aggregate_sig=ns)
    return size


def _att_out_sizes(n, nbytes):
    """Entries of every pz_attestation_cols_out column at its bound (include/prysm_hip.h)."""
    return {**{k: n for k in ATT_OUT_COLS}, **att_sizes(n, [nbytes, nbytes, nbytes, nbytes // 2, nbytes, nbytes])}


def _att_trim(cols, n, totals):
    """Views of the bound-sized columns at their decoded lengths (``totals`` on the host)."""
    used = att_sizes(n, totals)
    return {k: v[:used[k]] if k in used else v for k, v in cols.items()}


def unwire_attestations(data, offsets, field_num=0):
    """The inverse of :func:`attestations_device`: record i is ``data[offsets[i]:offsets[i+1]]``
    (bare, or framed as field ``field_num``), decoded on the GPU by ``pz_unwire_attestations``.
    Returns the columns of ``ATT_COLS`` plus ``n_oblique``, ``last_byte``, ``status`` (PZ_OK, or
    PZ_EINVAL for a record that is not the canonical encoding of its decoding: such a record
    has zero scalars and empty ranges) and ``totals`` (the seven totals of the header)."""
    from prysm_amd import _lib

    data = np.ascontiguousarray(_lib.as_u8(data), dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=_U64)
    n = len(offsets) - 1
    nbytes = int(offsets[-1] - offsets[0])
    size = _att_out_sizes(n, nbytes)
    cols = {k: np.zeros(max(size[k], 1), dtype=_ATT_DTYPES.get(k, np.uint8 if k in _BYTES_COLS else _U64))
            for k in ATT_OUT_COLS}
    c = _lib.AttestationColsOut(*[cols[k].ctypes.data for k in ATT_OUT_COLS])
    caps = np.array([nbytes, nbytes, nbytes, nbytes // 2, nbytes, nbytes], dtype=_U64)
    totals = np.zeros(7, dtype=_U64)
    _lib.lib.call("pz_unwire_attestations", data.ctypes.data, offsets.ctypes.data, n, field_num,
                  _lib.ctypes.byref(c), caps.ctypes.data, totals.ctypes.data)
    out = _att_trim({k: v[:size[k]] for k, v in cols.items()}, n, totals)
    out["totals"] = totals
    return out


def unwire_blocks(data, offsets):
    """The top level of serialized BeaconBlocks (block i is ``data[offsets[i]:offsets[i+1]]``),
    split on the GPU by ``pz_unwire_blocks``: the columns of ``BLOCK_COLS`` (``bytes_beg`` /
    ``bytes_len`` as (n, 5): fields 1, 3, 4, 5, 6) with the span of every attestation.  A
    block's ``status`` covers its top level only; :func:`folded_block_status` adds the verdicts
    of its attestations' bodies."""
    from prysm_amd import _lib

    data = np.ascontiguousarray(_lib.as_u8(data), dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=_U64)
    n = len(offsets) - 1
    cap = int(offsets[-1] - offsets[0]) // 2  # a framed record takes two bytes at least
    size = {k: n for k in BLOCK_COLS}
    size.update(bytes_beg=5 * n, bytes_len=5 * n, att_first=n + 1, att_beg=cap, att_end=cap, att_block_slot=cap,
                att_block=cap)
    cols = {k: np.zeros(max(size[k], 1), dtype=_BLOCK_DTYPES.get(k, _U64)) for k in BLOCK_COLS}
    c = _lib.BlockColsOut(*[cols[k].ctypes.data for k in BLOCK_COLS])
    natt = _lib.ctypes.c_uint64(0)
    _lib.lib.call("pz_unwire_blocks", data.ctypes.data, offsets.ctypes.data, n, cap, _lib.ctypes.byref(c),
                  _lib.ctypes.byref(natt))
    out = {k: v[:natt.value if k in ("att_beg", "att_end", "att_block_slot", "att_block") else size[k]]
           for k, v in cols.items()}
    out["bytes_beg"] = out["bytes_beg"].reshape(n, 5)
    out["bytes_len"] = out["bytes_len"].reshape(n, 5)
    out["natt"] = natt.value
    return out


def folded_block_status(block_status, att_block, att_status):
    """The engine's verdict on each block: bad (PZ_EINVAL) if its top level is bad or any of its
    attestations' records is.  numpy arrays or torch tensors (then nothing leaves the device)."""
    from prysm_amd import _lib

    bad = att_block[att_status != 0]
    if hasattr(block_status, "clone"):
        out = block_status.clone()
        out[bad.long()] = _lib.PZ_EINVAL
    else:
        out = block_status.copy()
        out[bad.astype(np.int64)] = _lib.PZ_EINVAL
    return out


def _torch_empty(torch, dev, count, np_dtype):
    """torch has no unsigned 32/64-bit arithmetic: those columns travel as int32 / int64."""
    dt = {np.uint8: torch.uint8, np.int32: torch.int32, np.uint32: torch.int32, np.int64: torch.int64,
          _U64: torch.int64}[np_dtype]
    return torch.empty(max(count, 1), dtype=dt, device=dev)


def unwire_attestations_device(d_bytes, d_begs, d_ends, n, field_num=0, nbytes=None):
    """``pz_dev_unwire_attestations`` on torch tensors, on the current stream: record i is
    ``d_bytes[d_begs[i]:d_ends[i]]`` (int64 tensors; a CSR batch passes ``offs[:-1]`` and
    ``offs[1:]``).  ``nbytes`` bounds the sum of the spans (default: all of ``d_bytes``, right
    for spans that do not overlap).  Returns the columns of ``ATT_OUT_COLS`` as tensors at their
    bounds and ``totals`` (7, on the device); :func:`_att_trim` cuts them once the totals are
    on the host."""
    import torch

    from prysm_amd import _lib

    dev = d_bytes.device
    nbytes = int(d_bytes.numel()) if nbytes is None else int(nbytes)
    size = _att_out_sizes(n, nbytes)
    cols = {k: _torch_empty(torch, dev, size[k], _ATT_DTYPES.get(k, np.uint8 if k in _BYTES_COLS else _U64))
            for k in ATT_OUT_COLS}
    c = _lib.AttestationColsOut(*[cols[k].data_ptr() for k in ATT_OUT_COLS])
    totals = torch.empty(7, dtype=torch.int64, device=dev)
    scr = torch.empty(int(_lib.lib.dll.pz_unwire_attestations_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    sh = _lib.stream_ptr(dev)
    _lib.lib.call("pz_dev_unwire_attestations", d_bytes.data_ptr(), d_begs.data_ptr(), d_ends.data_ptr(), n,
                  field_num, _lib.ctypes.byref(c), totals.data_ptr(), scr.data_ptr(), sh)
    out = {k: v[:size[k]] for k, v in cols.items()}
    out["totals"] = totals
    return out


def unwire_blocks_device(d_blocks, d_offsets, n, att_cap=None):
    """``pz_dev_unwire_blocks`` on torch tensors, on the current stream.  ``att_cap`` rows are
    allocated for the attestations (default: half the byte count, which always suffices).
    Returns the columns of ``BLOCK_COLS`` as tensors and ``natt`` (1, on the device)."""
    import torch

    from prysm_amd import _lib

    dev = d_blocks.device
    cap = int(d_blocks.numel()) // 2 if att_cap is None else int(att_cap)
    size = {k: n for k in BLOCK_COLS}
    size.update(bytes_beg=5 * n, bytes_len=5 * n, att_first=n + 1, att_beg=cap, att_end=cap, att_block_slot=cap,
                att_block=cap)
    cols = {k: _torch_empty(torch, dev, size[k], _BLOCK_DTYPES.get(k, _U64)) for k in BLOCK_COLS}
    c = _lib.BlockColsOut(*[cols[k].data_ptr() for k in BLOCK_COLS])
    natt = torch.empty(1, dtype=torch.int64, device=dev)
    scr = torch.empty(int(_lib.lib.dll.pz_unwire_blocks_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    sh = _lib.stream_ptr(dev)
    _lib.lib.call("pz_dev_unwire_blocks", d_blocks.data_ptr(), d_offsets.data_ptr(), n, cap, _lib.ctypes.byref(c),
                  natt.data_ptr(), scr.data_ptr(), sh)
    out = {k: v[:size[k]] for k, v in cols.items()}
    out["bytes_beg"] = out["bytes_beg"].view(n, 5)
    out["bytes_len"] = out["bytes_len"].view(n, 5)
    out["natt"] = natt
    return out


# ---- ShardAndCommitteesForSlots on the device (prysm_amd/csrc/wire_state.hip) ------------------
TABLE_COLS = ("arr_offs", "arr_shard", "arr_comm", "coffs", "members")


def committee_table(shard_and_committees):
    """ShardAndCommitteesForSlots -- a list (one per slot) of lists of ``(shard_id, committee)``
    pairs, or of ``pb.ShardAndCommitteeArray`` -- as the columns of ``pz_committee_table``: one
    committee per entry."""
    arrays = [[(sc.shard_id, sc.committee) for sc in a.array_shard_and_committee]
              if hasattr(a, "array_shard_and_committee") else list(a) for a in shard_and_committees]
    entries = [e for arr in arrays for e in arr]
    arr_offs = np.zeros(len(arrays) + 1, dtype=_U64)
    arr_offs[1:] = np.cumsum([len(arr) for arr in arrays], dtype=_U64)
    coffs = np.zeros(len(entries) + 1, dtype=_U64)
    coffs[1:] = np.cumsum([len(e[1]) for e in entries], dtype=_U64)
    members = np.concatenate([np.asarray(e[1], dtype=np.uint32) for e in entries] + [np.zeros(0, np.uint32)])
    return {"arr_offs": arr_offs, "arr_shard": np.array([e[0] & M64 for e in entries], dtype=_U64),
            "arr_comm": np.arange(len(entries), dtype=np.uint32), "coffs": coffs,
            "members": np.ascontiguousarray(members, dtype=np.uint32)}


def _table_struct(table, address):
    from prysm_amd import _lib

    t = _lib.CommitteeTable(narr=len(table["arr_offs"]) - 1, ncomm=len(table["coffs"]) - 1)
    for k in TABLE_COLS:
        setattr(t, k, address(table[k]))
    return t


def committees_device(table, field_num=12, members_cap=None):
    """ShardAndCommitteesForSlots encoded on the GPU, each array framed as repeated message
    ``field_num`` (CrystallizedState.shard_and_committees_for_slots = 12): the bytes
    :func:`crystallized_state` emits for that field.

    ``table``: ShardAndCommitteesForSlots itself (see :func:`committee_table`) or the table's
    columns as a dict keyed as ``TABLE_COLS``.  Host columns (numpy) go through
    ``pz_wire_committees`` and the result is ``bytes``.  Device columns (torch; int64 / int32
    carrying the unsigned values) go through ``pz_dev_wire_committees`` on the current stream: the
    result is ``(out, result)``, a uint8 tensor at its bound and an int64 tensor ``[length, status]``.
    ``members_cap`` bounds the sum of the entries' committee sizes (None: the number of members,
    right when no two entries share a committee); the call makes no wait."""
    from prysm_amd import _lib

    if not isinstance(table, dict):
        table = committee_table(table)
    nentries = len(table["arr_comm"])
    if not hasattr(table["arr_offs"], "data_ptr"):
        table = {k: np.ascontiguousarray(table[k]) for k in TABLE_COLS}
        t = _table_struct(table, _lib.ptr)
        coffs, comm = table["coffs"], table["arr_comm"].astype(np.int64)
        ok = comm[comm < len(coffs) - 1]
        cap = int(_lib.lib.dll.pz_wire_committees_bound(t.narr, nentries, int((coffs[ok + 1] - coffs[ok]).sum())))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        length = _lib.ctypes.c_uint64(0)
        _lib.lib.call("pz_wire_committees", _lib.ctypes.byref(t), nentries, field_num, _lib.ptr(out), cap,
                      _lib.ctypes.byref(length))
        return out[:length.value].tobytes()
    import torch

    dev = table["arr_offs"].device
    t = _table_struct(table, _lib.dptr)
    members_cap = int(table["members"].numel()) if members_cap is None else int(members_cap)
    dll = _lib.lib.dll
    out = torch.empty(max(int(dll.pz_wire_committees_bound(t.narr, nentries, members_cap)), 1), dtype=torch.uint8, device=dev)
    scr = torch.empty(max(int(dll.pz_wire_committees_scratch_bytes(t.narr, nentries, members_cap)), 16), dtype=torch.uint8,
                      device=dev)
    result = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.lib.call("pz_dev_wire_committees", _lib.ctypes.byref(t), nentries, members_cap, field_num, out.data_ptr(),
                  result.data_ptr(), scr.data_ptr(), _lib.stream_ptr(dev))
    return out, result


# ---- the stored CrystallizedState read back on the device (prysm_amd/csrc/unwire_state.hip) -------
VALIDATOR_COLS = ("public_key", "withdrawal_shard", "withdrawal_address", "withdrawal_address_offs", "randao_commitment",
                  "randao_commitment_offs", "balance", "start_dynasty", "end_dynasty")


def cstate_head(raw):
    """``pz_cstate_head`` (host only): fields 1-10 of a stored CrystallizedState.  Returns
    ``{"scalars": uint64[8], "rest": _lib.CstateRest, "rec_dynasty", "rec_slot", "rec_hash" (uint8),
    "rec_hash_offs" (nrec + 1), "body_beg"}``; a head that is not canonical raises ``PzError``
    (PZ_EINVAL) with the violation's offset as ``.offset``."""
    from prysm_amd import _lib

    ct = _lib.ctypes
    buf = np.ascontiguousarray(_lib.as_u8(raw), dtype=np.uint8)
    scalars, rest = np.zeros(_lib.RS_COUNT, _U64), _lib.CstateRest()
    nrec, body = ct.c_uint64(0), ct.c_uint64(0)
    cap = 0
    while True:
        dyn, slot = np.zeros(max(cap, 1), _U64), np.zeros(max(cap, 1), _U64)
        hashes, offs = np.zeros(max(buf.size, 1), np.uint8), np.zeros(cap + 1, _U64)
        rc = _lib.lib.dll.pz_cstate_head(_lib.ptr(buf), buf.size, scalars.ctypes.data, ct.byref(rest), dyn.ctypes.data,
                                         slot.ctypes.data, hashes.ctypes.data, offs.ctypes.data, cap, ct.byref(nrec),
                                         ct.byref(body))
        if rc == _lib.PZ_ERANGE and nrec.value > cap:
            cap = nrec.value
            continue
        if rc != _lib.PZ_OK:
            err = _lib.PzError(rc, _lib.lib.dll.pz_last_error().decode())
            err.offset = body.value
            raise err
        n = nrec.value
        return {"scalars": scalars, "rest": rest, "rec_dynasty": dyn[:n], "rec_slot": slot[:n], "rec_hash": hashes[:int(offs[n])],
                "rec_hash_offs": offs, "body_beg": body.value}


def _upload(buf, dev):
    import warnings

    import torch

    with warnings.catch_warnings():  # (a read-only source, e.g. np.frombuffer: it is only copied from)
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(buf).to(dev)


def unwire_crystallized_state_device(raw, device=0):
    """A stored CrystallizedState (``PersistCrystallizedState``'s bytes, blockchain/core.go:170-177)
    loaded on the device, on the current stream: one upload of the bytes, ``pz_cstate_head`` on the
    host, ``pz_dev_cstate_frame``, the read of its result record (the load's wait for sizes),
    exact-size tensors, ``pz_dev_cstate_decode`` and the read of its status word.  Exactly the
    canonical encoding is accepted: anything else raises ``PzError`` (PZ_EINVAL, or PZ_ERANGE for a
    record over ``_lib.CSTATE_RECORD_LIMIT``) with the violation's offset as ``.offset``.

    Returns the head (:func:`cstate_head`'s dict) as ``head``, ``nval``, the columns of
    ``VALIDATOR_COLS`` and of ``TABLE_COLS`` as device tensors (int64 / int32 carrying the unsigned
    values), ``narr`` and ``field12``: the received span of field 12, a uint8 device tensor."""
    import torch

    from prysm_amd import _lib

    buf = np.ascontiguousarray(_lib.as_u8(raw), dtype=np.uint8)
    head = cstate_head(buf)
    dev = torch.device("cuda", device)
    n = int(buf.size)
    d_bytes = _upload(buf, dev) if n else torch.empty(0, dtype=torch.uint8, device=dev)  # the one upload
    dll, sh = _lib.lib.dll, _lib.stream_ptr(dev)
    scr = torch.empty(int(dll.pz_cstate_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    result = torch.empty(_lib.CSF_COUNT, dtype=torch.int64, device=dev)
    _lib.lib.call("pz_dev_cstate_frame", _lib.dptr(d_bytes), n, head["body_beg"], scr.data_ptr(), result.data_ptr(), sh)
    r = [int(x) for x in result.cpu()]  # the wait

    def refuse(status, offset):
        err = _lib.PzError(status, "stored CrystallizedState: %s at offset %d" % (
            "a ValidatorRecord over the framing's limit" if status == _lib.PZ_ERANGE else "not the canonical encoding", offset))
        err.offset = offset
        return err

    if r[_lib.CSF_STATUS]:
        raise refuse(r[_lib.CSF_STATUS], r[_lib.CSF_OFFSET])
    nval, narr, nent, nmem = r[_lib.CSF_NVAL], r[_lib.CSF_NARR], r[_lib.CSF_NENTRIES], r[_lib.CSF_NMEMBERS]
    size = {k: nval for k in VALIDATOR_COLS}
    size.update(withdrawal_address=r[_lib.CSF_ADDRESS_BYTES], randao_commitment=r[_lib.CSF_COMMITMENT_BYTES],
                withdrawal_address_offs=nval + 1, randao_commitment_offs=nval + 1, arr_offs=narr + 1, arr_shard=nent,
                arr_comm=nent, coffs=nent + 1, members=nmem)
    kind = {"withdrawal_address": np.uint8, "randao_commitment": np.uint8, "arr_comm": np.uint32, "members": np.uint32}
    cols = {k: _torch_empty(torch, dev, size[k], kind.get(k, _U64)) for k in VALIDATOR_COLS + TABLE_COLS}
    for k in ("withdrawal_address_offs", "randao_commitment_offs", "arr_offs", "coffs"):
        cols[k][:1] = 0  # (what an empty message leaves as it is)
    v = _lib.ValidatorColsOut(*[cols[k].data_ptr() for k in VALIDATOR_COLS])
    t = _lib.CommitteeTableOut(narr=narr, ncomm=nent, **{k: cols[k].data_ptr() for k in TABLE_COLS})
    status = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.lib.call("pz_dev_cstate_decode", _lib.dptr(d_bytes), n, scr.data_ptr(), _lib.ctypes.byref(v), _lib.ctypes.byref(t),
                  status.data_ptr(), sh)
    st = [int(x) for x in status.cpu()]
    if st[0]:
        raise refuse(st[0], st[1])
    out = {k: c[:size[k]] for k, c in cols.items()}
    out.update(head=head, nval=nval, narr=narr, field12=d_bytes[r[_lib.CSF_VAL_END]:r[_lib.CSF_F12_END]], result=r)
    return out


def unwire_crystallized_state(raw, device=0):
    """:func:`unwire_crystallized_state_device` as a host-side view, for tests and tools: the same
    dict with numpy columns (the unsigned dtypes restored) and ``field12`` as bytes."""
    d = unwire_crystallized_state_device(raw, device)
    out = dict(d)
    for k in VALIDATOR_COLS + TABLE_COLS:
        a = d[k].cpu().numpy()
        out[k] = a.view(_U64) if a.dtype == np.int64 else a.view(np.uint32) if a.dtype == np.int32 else a
    out["field12"] = d["field12"].cpu().numpy().tobytes()
    return out
