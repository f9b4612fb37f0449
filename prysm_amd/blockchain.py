"""Block pipeline of the reference's beacon chain (blockchain/service.go:229-363 over
blockchain/core.go) — Python face of the native engine in ``prysm_amd/csrc/chain.hip``.

``BeaconChain.process_serialized(data, offsets)`` feeds canonical BeaconBlock encodings (as
the sync service receives them, sync/service.go:147-164) through ``pz_chain_process_blocks``:
a C++ walk with the control flow of ``ChainService.blockProcessing`` (parent check,
processAttestation, calculateBlockVoteCache, updateHead, saveBlock, IsCycleTransition ->
stateRecalc, computeNewActiveState), keeping the reference's object-sharing and ordering
semantics (restated by the oracle in oracle/replay.py).  The device does the
heavy work, batched per call:

* H  block digests, attestation ``Hash``/``Key`` (one CSR BLAKE2b launch before the walk),
     the 64-byte processAttestation message digests (``core.go:277-290``, one launch after
     it) and the Active/Crystallized state roots;
* T  the block vote cache (``core.go:300-345``) lives in HBM — a dedup bitmap and a u64
     total per signed parent hash — fed by the vote-tally kernel once per stretch of blocks
     between balance changes;
* R  stateRecalc's processCrosslinks + CalculateRewards + next-cycle balance run as one epoch
     instance on the HBM-resident validator arrays.

Where the reference panics, ``ChainPanic`` is raised and the chain object is spent.

The ``*_serialized_blocks`` functions and ``ResidentChain`` are the same pipeline composed from the
device-resident objects of ``prysm_amd.votes`` and ``prysm_amd.pending`` instead of the engine:
``ResidentChain.process_serialized`` takes a run of received blocks, its cycle transition included,
with one upload and one host read (``pz_dev_block_cycle``, prysm_amd/csrc/blockcycle.hip).
"""
import ctypes
import warnings

import numpy as np

from prysm_amd import _lib, wire
from prysm_amd._lib import PzError, lib

BLOCK_RESULT = np.dtype([("hash", "u1", 32), ("status", "<i4"), ("transition", "<i4"),
                         ("first_att", "<u4"), ("natt", "<u4")])
ATT_RESULT = np.dtype([("status", "<i4"), ("msg_len", "<u4"), ("key", "u1", 32), ("hash", "u1", 32),
                       ("msg", "u1", 64)])
BLOCK_STATUS = {0: "processed", 1: "no_parent", 2: "attestations_rejected", 3: "saved_not_candidate"}
ATT_PROCESSED, ATT_NOT_PROCESSED = 0, 1
ATT_ERRORS = {2: "slot too high", 3: "slot too low", 4: "justified slot mismatch", 5: "no committee",
              6: "bitfield length", 7: "non-zero trailing bits"}


def _committee_table(shard_and_committees):
    """ShardAndCommitteesForSlots (a list per slot of ``(shard_id, committee)`` pairs) as the
    pz_att_check_batch table: arr_offs, arr_shard, arr_comm, coffs."""
    u64 = np.uint64
    arr_offs = np.zeros(len(shard_and_committees) + 1, dtype=u64)
    arr_offs[1:] = np.cumsum([len(arr) for arr in shard_and_committees], dtype=u64)
    entries = [e for arr in shard_and_committees for e in arr]
    arr_shard = np.ascontiguousarray([e[0] for e in entries] or [0], dtype=u64)
    arr_comm = np.arange(max(len(entries), 1), dtype=np.uint32)
    coffs = np.zeros(len(entries) + 1, dtype=u64)
    coffs[1:] = np.cumsum([len(e[1]) for e in entries], dtype=u64)
    return arr_offs, arr_shard, arr_comm, coffs


def check_attestations(atts, block_slots, last_justified_slot, last_state_recalc, n_recent,
                       shard_and_committees):
    """processAttestation's checks (blockchain/core.go:240-297, :348-394) for a batch of
    attestations on the GPU (``pz_check_attestations``, one lane each).

    ``atts``: AttestationRecord-like objects; ``block_slots[i]``: the slot of the block that
    carries ``atts[i]``; the chain state: ``last_justified_slot``, ``last_state_recalc``,
    ``n_recent`` = len(RecentBlockHashes) and ``shard_and_committees`` = ShardAndCommitteesForSlots
    as a list (one per slot) of lists of ``(shard_id, committee)`` pairs.  Returns
    ``(status, committee_index, parents_start)``: status PZ_ATT_PROCESSED, the first failed
    check (PZ_ATT_*), or PZ_ERANGE / PZ_EINDEX where Go panics; committee_index counts the
    table's (shard, committee) entries in order (-1 if not reached)."""
    n = len(atts)
    u64 = np.uint64
    cols = {k: np.ascontiguousarray([getattr(a, k) for a in atts], dtype=u64)
            for k in ("slot", "justified_slot", "shard_id")}
    n_obl = np.ascontiguousarray([len(a.oblique_parent_hashes) for a in atts], dtype=u64)
    bslot = np.ascontiguousarray(block_slots, dtype=u64)
    bf = [bytes(a.attester_bitfield) for a in atts]
    boffs = np.zeros(n + 1, dtype=u64)
    boffs[1:] = np.cumsum([len(x) for x in bf], dtype=u64)
    bits = np.frombuffer(b"".join(bf) + b"\0", dtype=np.uint8)
    arr_offs, arr_shard, arr_comm, coffs = _committee_table(shard_and_committees)
    status = np.zeros(max(n, 1), dtype=np.int32)
    comm = np.zeros(max(n, 1), dtype=np.uint32)
    pstart = np.zeros(max(n, 1), dtype=u64)
    b = _lib.AttCheckBatch(
        n, _lib.ptr(cols["slot"]), _lib.ptr(cols["justified_slot"]), _lib.ptr(cols["shard_id"]), _lib.ptr(n_obl),
        _lib.ptr(bits), _lib.ptr(boffs), _lib.ptr(bslot), last_justified_slot, last_state_recalc, n_recent,
        len(shard_and_committees), _lib.ptr(arr_offs), _lib.ptr(arr_shard), _lib.ptr(arr_comm), _lib.ptr(coffs),
        _lib.ptr(status), _lib.ptr(comm), _lib.ptr(pstart))
    lib.call("pz_check_attestations", ctypes.byref(b))
    ci = comm[:n].astype(np.int64)
    ci[comm[:n] == 0xFFFFFFFF] = -1
    return status[:n], ci, pstart[:n]


def _to_device(a, dev):
    """A numpy array as a device tensor (torch has no unsigned 32/64-bit types: they travel as
    int32 / int64)."""
    import torch

    a = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
    with warnings.catch_warnings():  # (a read-only source, e.g. np.frombuffer: it is only copied from)
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(a).to(dev)


def _split_decode_check(payload, offsets, last_justified_slot, last_state_recalc, n_recent, shard_and_committees,
                        device, want_committee):
    """The steps the ``*_serialized_blocks`` functions share, on the current stream: ``payload``
    (the blocks' bytes, with whatever slack the caller's later kernels want) goes to the device
    once, is split (``pz_dev_unwire_blocks``), decoded (``pz_dev_unwire_attestations``) and checked
    (``pz_dev_check_attestations``).  Only the attestation count visits the host.  Returns the
    device tensors: ``d_bytes``, ``d_offs``, ``blk``, ``att``, ``natt`` (an int), ``rec`` (the
    records' decode statuses), ``status`` (the checks' statuses with ``rec`` folded in, natt rows),
    ``committee`` (or None), ``parents_start`` and ``block_status`` (folded) -- and, for the block
    gate, ``chk`` (the checks' batch) and ``table`` (the committee table's device tensors)."""
    import torch

    dev = torch.device("cuda", device)
    table = [_to_device(a, dev) for a in _committee_table(shard_and_committees)]
    return _decode_check(_to_device(payload, dev), _to_device(offsets, dev), len(offsets) - 1, last_justified_slot,
                         last_state_recalc, n_recent, len(shard_and_committees), table, dev, want_committee)


def _decode_check(d_bytes, d_offs, n, last_justified_slot, last_state_recalc, n_recent, narr, table, dev, want_committee):
    """:func:`_split_decode_check` from the device on: ``d_bytes`` / ``d_offs`` are the uploaded bytes
    and offsets, ``table`` the committee table's four device tensors (``_committee_table``'s order)
    over ``narr`` slots."""
    import torch

    blk = wire.unwire_blocks_device(d_bytes, d_offs, n)
    natt = int(blk["natt"].item())
    att = wire.unwire_attestations_device(d_bytes, blk["att_beg"], blk["att_end"], natt, 0)
    status = torch.zeros(max(natt, 1), dtype=torch.int32, device=dev)
    comm = torch.zeros(max(natt, 1), dtype=torch.int32, device=dev) if want_committee else None
    pstart = torch.zeros(max(natt, 1), dtype=torch.int64, device=dev)
    b = _lib.AttCheckBatch(
        natt, att["slot"].data_ptr(), att["justified_slot"].data_ptr(), att["shard_id"].data_ptr(),
        att["n_oblique"].data_ptr(), att["attester_bitfield"].data_ptr(), att["attester_bitfield_offs"].data_ptr(),
        blk["att_block_slot"].data_ptr(), last_justified_slot, last_state_recalc, n_recent,
        narr, *[t.data_ptr() for t in table], status.data_ptr(),
        comm.data_ptr() if want_committee else None, pstart.data_ptr(), att["last_byte"].data_ptr())
    lib.call("pz_dev_check_attestations", ctypes.byref(b), _lib.stream_ptr(dev))
    rec = att["status"][:natt]
    status = torch.where(rec != 0, rec, status[:natt])
    block_status = wire.folded_block_status(blk["status"], blk["att_block"][:natt], rec)
    return {"dev": dev, "n": n, "d_bytes": d_bytes, "d_offs": d_offs, "blk": blk, "att": att, "natt": natt, "rec": rec,
            "status": status, "committee": comm, "parents_start": pstart, "block_status": block_status,
            "chk": b, "table": table}


def check_serialized_blocks(data, offsets, last_justified_slot, last_state_recalc, n_recent, shard_and_committees,
                            device=0):
    """:func:`check_attestations` for a batch of received blocks held as bytes (block i is
    ``data[offsets[i]:offsets[i+1]]``, as the sync service receives them, sync/service.go:147-164):
    the bytes go to the device once and are split (``pz_dev_unwire_blocks``), decoded
    (``pz_dev_unwire_attestations`` over the attestations' spans) and checked
    (``pz_dev_check_attestations``) there, on the current stream; no column visits the host in
    between (only the attestation count does, to size the launches).

    Returns ``(block_status, att_first, att_status, committee_index, parents_start)``:
    block_status[i] is PZ_OK, or PZ_EINVAL where the engine rejects the block's bytes (its top
    level or one of its attestations is not canonical); block i's attestations are rows
    att_first[i] .. att_first[i+1] of the other three, which are what check_attestations returns,
    except that an attestation whose record is not canonical reports PZ_EINVAL."""
    data = np.ascontiguousarray(_lib.as_u8(data), dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    d = _split_decode_check(data if data.size else np.zeros(1, np.uint8), offsets, last_justified_slot,
                            last_state_recalc, n_recent, shard_and_committees, device, want_committee=True)
    natt = d["natt"]
    ci = d["committee"][:natt].cpu().numpy().view(np.uint32).astype(np.int64)
    ci[ci == 0xFFFFFFFF] = -1
    return (d["block_status"].cpu().numpy(), d["blk"]["att_first"].cpu().numpy().view(np.uint64),
            d["status"].cpu().numpy(), ci, d["parents_start"][:natt].cpu().numpy().view(np.uint64))


_MSG_COLS = ("slot", "shard_id", "shard_block_hash", "shard_block_hash_offs", "oblique_parent_hashes", "oblique_offs",
             "oblique_first")


def _recent_array(recent_hashes):
    """RecentBlockHashes() (types/state.go:189-195: every entry under BytesToHash) as (k, 32) uint8."""
    if isinstance(recent_hashes, np.ndarray):
        return np.ascontiguousarray(recent_hashes, dtype=np.uint8).reshape(-1, 32)
    from prysm_amd.types import bytes_to_hash
    return np.frombuffer(b"".join(bytes_to_hash(h) for h in recent_hashes), dtype=np.uint8).reshape(-1, 32)


def attestation_messages(cols, n, status, parents_start, recent_hashes):
    """The processAttestation message digests (blockchain/core.go:277-290) of n records held as
    host columns (numpy arrays keyed as ``wire.ATT_COLS``), with ``status`` / ``parents_start`` as
    :func:`check_attestations` returns them and ``recent_hashes`` = RecentBlockHashes() (a list
    of byte strings, normalised here, or a (k, 32) uint8 array): ``pz_attestation_messages``.
    Returns ``(digests (n, 64) uint8, msg_len (n) uint32)``; a row that is not PROCESSED has a
    zero digest and length 0."""
    c = _lib.att_cols(cols, _MSG_COLS)
    status = np.ascontiguousarray(status, dtype=np.int32)
    pstart = np.ascontiguousarray(parents_start, dtype=np.uint64)
    recent = _recent_array(recent_hashes)
    out = np.zeros((n, 64), dtype=np.uint8)
    mlen = np.zeros(n, dtype=np.uint32)
    b = _lib.AttMsgBatch(natt=n, status=_lib.ptr(status), parents_start=_lib.ptr(pstart), recent=_lib.ptr(recent),
                         n_recent=len(recent), out=_lib.ptr(out), msg_len=_lib.ptr(mlen),
                         **{k: getattr(c, k) for k in _MSG_COLS})
    lib.call("pz_attestation_messages", ctypes.byref(b))
    return out, mlen


def attestation_messages_device(cols, n, status, parents_start, recent, n_recent=None):
    """:func:`attestation_messages` on device columns (torch tensors keyed as ``wire.ATT_COLS``,
    e.g. from ``wire.unwire_attestations_device``; ``status`` int32, ``parents_start`` int64 and
    ``recent`` ((k, 32) uint8, already BytesToHash-normalised) tensors too), on the current
    stream: ``pz_dev_attestation_messages``.  Returns ``(digests (n, 64) uint8, msg_len (n)
    int32)`` tensors; nothing visits the host."""
    import torch

    dev = status.device
    out = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    mlen = torch.empty(n, dtype=torch.int32, device=dev)
    c = _lib.att_cols(cols, _MSG_COLS)
    b = _lib.AttMsgBatch(natt=n, status=status.data_ptr(), parents_start=parents_start.data_ptr(),
                         recent=recent.data_ptr() if recent.numel() else None,
                         n_recent=recent.numel() // 32 if n_recent is None else n_recent,
                         out=out.data_ptr() if n else None, msg_len=mlen.data_ptr() if n else None,
                         **{k: getattr(c, k) for k in _MSG_COLS})
    lib.call("pz_dev_attestation_messages", ctypes.byref(b), _lib.stream_ptr(dev))
    return out, mlen


def digest_serialized_blocks(data, offsets, last_justified_slot, last_state_recalc, n_recent, shard_and_committees,
                             recent_hashes, device=0):
    """The H side of blockProcessing (blockchain/service.go:229-363) for a batch of received
    blocks held as bytes, against one chain state: after one upload the bytes are split
    (``pz_dev_unwire_blocks``), decoded (``pz_dev_unwire_attestations``) and checked
    (``pz_dev_check_attestations``) as in :func:`check_serialized_blocks`, then hashed where they
    lie (``pz_dev_blake2b512_spans``: Block.Hash over the blocks, Attestation.Hash over the
    records' spans) and ``Key`` and the processAttestation message digest are made from the
    decoded columns (``pz_dev_attestation_keys``, ``pz_dev_attestation_messages``).  No column
    visits the host in between (only the attestation count does, to size the launches).

    ``recent_hashes``: RecentBlockHashes() (``n_recent`` entries: byte strings, normalised here,
    or a (n_recent, 32) uint8 array).  Returns a dict of numpy arrays: ``block_status`` (PZ_OK /
    PZ_EINVAL as check_serialized_blocks folds it), ``block_hash`` (n, 32), ``att_first`` (n+1),
    ``att_status`` and, per attestation, ``hash`` (32), ``key`` (32; zero where the record is not
    canonical), ``msg`` (64) and ``msg_len`` (zero where the attestation is not PROCESSED)."""
    import torch

    from prysm_amd import types

    dev = torch.device("cuda", device)
    data = np.ascontiguousarray(_lib.as_u8(data), dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    recent = _recent_array(recent_hashes)
    if len(recent) != n_recent:
        raise PzError(_lib.PZ_EINVAL, "recent_hashes holds %d hashes, n_recent is %d" % (len(recent), n_recent))

    # (the span hash reads whole dwords: 4 bytes of slack after the last block)
    d = _split_decode_check(np.concatenate([data[:int(offsets[-1])] if n else data[:0], np.zeros(4, np.uint8)]), offsets,
                            last_justified_slot, last_state_recalc, n_recent, shard_and_committees, device,
                            want_committee=False)
    d_bytes, d_offs, blk, att, natt = d["d_bytes"], d["d_offs"], d["blk"], d["att"], d["natt"]
    rec, status, pstart, block_status = d["rec"], d["status"], d["parents_start"], d["block_status"]
    sh = _lib.stream_ptr(dev)

    block_hash = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    att_hash = torch.empty((natt, 32), dtype=torch.uint8, device=dev)
    lib.call("pz_dev_blake2b512_spans", d_bytes.data_ptr(), d_offs[:-1].data_ptr(), d_offs[1:].data_ptr(), n,
             block_hash.data_ptr() if n else None, 32, sh)
    lib.call("pz_dev_blake2b512_spans", d_bytes.data_ptr(), blk["att_beg"].data_ptr(), blk["att_end"].data_ptr(), natt,
             att_hash.data_ptr() if natt else None, 32, sh)
    key = types.attestation_keys_device(att, natt, rec_status=rec if natt else None)
    if natt and n_recent < 64 and (status == ATT_PROCESSED).any().item():  # (an m > 0 row can pass with fewer)
        raise PzError(_lib.PZ_EINVAL, "n_recent %d < 64 with a PROCESSED attestation" % n_recent)
    if natt and n_recent >= 64:
        msg, msg_len = attestation_messages_device(att, natt, status.contiguous(), pstart, _to_device(recent, dev),
                                                   n_recent)
    else:
        msg = torch.zeros((natt, 64), dtype=torch.uint8, device=dev)
        msg_len = torch.zeros(natt, dtype=torch.int32, device=dev)
    return {"block_status": block_status.cpu().numpy(), "block_hash": block_hash.cpu().numpy(),
            "att_first": blk["att_first"].cpu().numpy().view(np.uint64), "att_status": status.cpu().numpy(),
            "hash": att_hash.cpu().numpy(), "key": key.cpu().numpy(), "msg": msg.cpu().numpy(),
            "msg_len": msg_len.cpu().numpy().view(np.uint32)}


BLOCK_REJECTED, BLOCK_TALLIED, BLOCK_MIXED = 0, 1, 2  # tally_serialized_blocks' per-block report


def _open_blocks(d, candidate=None):
    """service.go:304-306 on the device, from :func:`_split_decode_check`'s tensors: a block is open
    iff its folded status is PZ_OK, it has an attestation and its last attestation is PROCESSED --
    and, when ``candidate`` (a per-block 0/1 sequence) is given, ``candidate[i]`` too.  Returns
    ``(open, att_block, count, nproc)``: the block of every attestation row, and per block its rows
    and how many of them are PROCESSED.  Needs ``natt > 0``."""
    import torch

    dev, n, natt, blk = d["dev"], d["n"], d["natt"], d["blk"]
    first = blk["att_first"]
    count = first[1:] - first[:-1]
    att_block = blk["att_block"][:natt].long()
    proc = (d["status"] == ATT_PROCESSED).long()
    nproc = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, att_block, proc)
    last_ok = proc[(first[1:] - 1).clamp(min=0)] == 1
    open_ = (d["block_status"] == _lib.PZ_OK) & (count > 0) & last_ok
    if candidate is not None:
        open_ = open_ & _to_device(np.ascontiguousarray(candidate, dtype=np.uint8), dev).bool()
    return open_, att_block, count, nproc


def _pend(pool, d, candidate):
    """Appends the PROCESSED rows of the open blocks of ``d`` to ``pool``; returns ``open``."""
    import torch

    if not d["natt"]:
        return torch.zeros(d["n"], dtype=torch.bool, device=d["dev"])
    open_, att_block, _, _ = _open_blocks(d, candidate)
    pool.append_columns(d["att"], d["natt"], d["status"].contiguous(), d["committee"], take=open_[att_block].to(torch.uint8))
    return open_


def pend_serialized_blocks(pool, data, offsets, last_justified_slot, last_state_recalc, n_recent, shard_and_committees,
                           candidate=None, device=0):
    """processedAttestations (blockchain/service.go:280-301) of a batch of received blocks held as
    bytes, against one chain state, into ``pool`` (a ``prysm_amd.pending.DevicePendingAttestations``):
    the same upload, split, decode and checks as :func:`check_serialized_blocks`, then
    ``pz_dev_att_pool_append`` over the decoded columns and the checks' outputs -- what
    computeNewActiveState (core.go:223-237) appends to PendingAttestations.  Which rows it takes is
    formed on the device; no column visits the host in between.

    A block is open iff its bytes are accepted (folded status PZ_OK), it has at least one
    attestation and its LAST attestation is PROCESSED (service.go:304-306); with ``candidate`` (one
    0/1 per block) it must also have ``candidate[i]``: the walk's decision that this block reaches
    computeNewActiveState (its parent is saved and no candidate was already chosen,
    service.go:261-269, :331-333), which is sequential and stays the caller's.  The PROCESSED rows
    of open blocks are appended, those of mixed blocks included: processedAttestations holds only
    the attestations that passed.  Returns ``(block_open, att_first, att_status)``."""
    data = np.ascontiguousarray(_lib.as_u8(data), dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    d = _split_decode_check(data if data.size else np.zeros(1, np.uint8), offsets, last_justified_slot,
                            last_state_recalc, n_recent, shard_and_committees, device, want_committee=True)
    open_ = _pend(pool, d, candidate)
    return (open_.cpu().numpy(), d["blk"]["att_first"].cpu().numpy().view(np.uint64), d["status"].cpu().numpy())


def _gate(d, candidate=None, block_status=None, head=0, tail=0):
    """``pz_dev_block_gate`` over :func:`_split_decode_check`'s tensors, on the current stream.
    Returns ``(word, report, vote_status, pend_take, flags)``: ``word`` is the one uint8 buffer
    ``flags`` (four bytes) and ``report`` (the n after them) are views of, so that one copy
    brings both to the host; ``head`` / ``tail`` bytes before and after them are the caller's, to
    come along in that copy.  ``block_status`` (int32 per block) replaces the decoder's."""
    import torch

    dev, n, natt, blk, att = d["dev"], d["n"], d["natt"], d["blk"], d["att"]
    if d["committee"] is None:
        raise PzError(_lib.PZ_EINVAL, "the block gate completes the committee column: decode with want_committee")
    word = torch.zeros(head + 4 + n + tail, dtype=torch.uint8, device=dev)
    flags, report = word[head:head + 4].view(torch.int32), word[head + 4:head + 4 + n]
    status = d["status"].contiguous()
    vote_status = torch.empty(max(natt, 1), dtype=torch.int32, device=dev)
    pend_take = torch.empty(max(natt, 1), dtype=torch.uint8, device=dev)
    cand = None if candidate is None else _to_device(np.ascontiguousarray(candidate, dtype=np.uint8), dev)
    if cand is not None and cand.numel() != n:
        raise PzError(_lib.PZ_EINVAL, "candidate holds %d entries for %d blocks" % (cand.numel(), n))
    chk, p = d["chk"], _lib.dptr
    chk = _lib.AttCheckBatch(
        natt=natt, slot=p(att["slot"]), shard_id=p(att["shard_id"]), n_oblique=p(att["n_oblique"]),
        block_slot=p(blk["att_block_slot"]), last_state_recalc=chk.last_state_recalc, n_recent=chk.n_recent,
        narr=chk.narr, arr_offs=chk.arr_offs, arr_shard=chk.arr_shard, arr_comm=chk.arr_comm, coffs=chk.coffs,
        status=p(status), committee=p(d["committee"]), parents_start=p(d["parents_start"]))
    b = _lib.BlockGateBatch(nblocks=n, att_first=p(blk["att_first"]),
                            block_status=p(blk["status"] if block_status is None else block_status),
                            rec_status=p(d["rec"]), candidate=p(cand), chk=chk, report=p(report),
                            vote_status=p(vote_status), pend_take=p(pend_take), flags=p(flags))
    lib.call("pz_dev_block_gate", ctypes.byref(b), _lib.stream_ptr(dev))
    return word, report, vote_status[:natt], pend_take[:natt], flags


def gate_blocks(d, candidate=None):
    """The block gate (``pz_dev_block_gate``, prysm_amd/csrc/blockgate.hip) over
    :func:`_split_decode_check`'s tensors ``d``, on the current stream: which blocks are open
    (service.go:281-306), which rows calculateBlockVoteCache tallies (service.go:313-318 runs over
    every attestation of an open block, the refused ones included) and which reach
    processedAttestations.  Returns the device tensors ``(report, vote_status, pend_take, flags)``:
    ``report`` uint8 per block (BLOCK_REJECTED / BLOCK_TALLIED / BLOCK_MIXED), ``vote_status`` int32
    per row (PZ_ATT_PROCESSED exactly where the reference tallies the row: the tally's ``status``),
    ``pend_take`` uint8 per row (the pool's ``take``; ``candidate`` as in
    :func:`pend_serialized_blocks`) and ``flags`` (one int32; bit 0: the reference panics).
    ``d["committee"]`` and ``d["parents_start"]`` are completed in place for the re-derived rows.
    Nothing visits the host."""
    return _gate(d, candidate)[1:]


def tally_serialized_blocks(cache, data, offsets, last_justified_slot, last_state_recalc, n_recent,
                            shard_and_committees, recent_hashes, balance, device=0, pending=None, candidate=None,
                            tally_mixed=False):
    """The T side of blockProcessing (blockchain/service.go:313-318: calculateBlockVoteCache over
    a block's attestations, core.go:300-345) for a batch of received blocks held as bytes, against
    one chain state, into ``cache`` (a ``prysm_amd.votes.DeviceVoteCache``): the same upload, split,
    decode and checks as :func:`check_serialized_blocks`, then ``pz_dev_vote_cache_tally`` over the
    decoded columns and the checks' outputs.  Which rows it takes is formed on the device; no
    column visits the host in between (only the attestation count does, to size the launches).

    A block is tallied iff its bytes are accepted (folded status PZ_OK), it has at least one
    attestation, and every one of them -- so the last one too -- is PROCESSED.  The reference
    goes on when only the LAST attestation passed (service.go:304-306) and then tallies the
    failed ones as well, re-deriving their parents and committee: such a mixed block is left to
    the engine, none of its rows is tallied, and it is reported.  Returns ``(block, att_first,
    att_status)``: block[i] is BLOCK_TALLIED (1), BLOCK_REJECTED (0: bad bytes, no attestation or
    the last one failed, as service.go:304-306) or BLOCK_MIXED (2); block i's attestations are
    rows att_first[i] .. att_first[i+1] of att_status.  ``recent_hashes`` as in
    :func:`digest_serialized_blocks`; ``balance``: the validators' balances (nval).

    With ``pending`` (a ``prysm_amd.pending.DevicePendingAttestations``) the same decode also feeds
    the pool, as :func:`pend_serialized_blocks` does (``candidate`` as there; it bears on the pool
    alone): one upload then serves both.  With ``pending=None`` nothing about this function changes.

    With ``tally_mixed=True`` the decision is the block gate's (:func:`gate_blocks`): a mixed block is
    tallied as the reference tallies it, its refused attestations included (their parents and
    committee re-derived on the device), so the cache is exact on every block the reference
    tallies; the report still says 0 / 1 / 2.  Where the reference would panic on some row of the
    batch (a slice bound or committee index of the re-derivation, or processAttestation's own),
    ``ChainPanic`` is raised and neither the cache nor the pool sees any of the batch: it lands whole
    or panics.  The price is one more host read -- the gate's flag word and report, in one copy --
    between the gate and the tally.  (A panic only the tally can find, CheckBit past a short
    bitfield, stays the cache's sticky PZ_EINDEX, as without the gate.)"""
    import torch

    data = np.ascontiguousarray(_lib.as_u8(data), dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    recent = _recent_array(recent_hashes)
    if len(recent) != n_recent:
        raise PzError(_lib.PZ_EINVAL, "recent_hashes holds %d hashes, n_recent is %d" % (len(recent), n_recent))
    d = _split_decode_check(data if data.size else np.zeros(1, np.uint8), offsets, last_justified_slot,
                            last_state_recalc, n_recent, shard_and_committees, device, want_committee=True)
    dev, n, natt, blk, status = d["dev"], d["n"], d["natt"], d["blk"], d["status"]
    first = blk["att_first"]
    report = torch.zeros(n, dtype=torch.int64, device=dev)
    if tally_mixed:
        word, report, vote_status, pend_take, _ = _gate(d, candidate if pending is not None else None)
        host = word.cpu().numpy()  # the one extra read: flags, then the report
        if host[:4].view(np.uint32)[0] & 1:
            raise ChainPanic("a block of the batch makes the reference panic (processAttestation or "
                             "calculateBlockVoteCache: slice bounds, core.go:353, or committee index, core.go:367)")
        if natt:
            cache.tally_columns(d["att"], natt, vote_status, d["committee"], d["parents_start"], _to_device(recent, dev),
                                _to_device(_members(shard_and_committees), dev), d["table"][3],
                                _to_device(np.ascontiguousarray(balance, dtype=np.uint64), dev))
            if pending is not None:
                pending.append_columns(d["att"], natt, status.contiguous(), d["committee"], take=pend_take)
        return (host[4:].astype(np.int64), first.cpu().numpy().view(np.uint64), status.cpu().numpy())
    if natt:
        open_, att_block, count, nproc = _open_blocks(d)
        report = open_.long() * (BLOCK_TALLIED + (BLOCK_MIXED - BLOCK_TALLIED) * (nproc != count).long())
        take = (report == BLOCK_TALLIED)[att_block].to(torch.uint8)
        coffs = _committee_table(shard_and_committees)[3]
        cache.tally_columns(d["att"], natt, status.contiguous(), d["committee"], d["parents_start"],
                            _to_device(recent, dev), _to_device(_members(shard_and_committees), dev), _to_device(coffs, dev),
                            _to_device(np.ascontiguousarray(balance, dtype=np.uint64), dev), take=take)
        if pending is not None:
            _pend(pending, d, candidate)
    return (report.cpu().numpy(), first.cpu().numpy().view(np.uint64), status.cpu().numpy())


class ChainPanic(RuntimeError):
    """The reference would panic here (index out of range / nil map / nil state)."""


WALK_OFF, WALK_SAVED, WALK_CANDIDATE, WALK_DEFERRED = 0, 1, 2, 3  # walk_serialized_blocks' per-block code
_INELIGIBLE = 1  # a block status that is not PZ_OK: the parent is not saved or CanProcessBlock fails


def walk_serialized_blocks(cache, pool, ring, data, offsets, last_justified_slot, last_state_recalc,
                           shard_and_committees, balance, eligible=None, has_candidate=False, candidate_slot=0, lag=0,
                           want_digests=False, device=0):
    """blockProcessing (blockchain/service.go:229-363) for a RUN of consecutive received blocks held
    as bytes, each against its own RecentBlockHashes, in one call: into ``cache`` (a
    ``prysm_amd.votes.DeviceVoteCache``), ``pool`` (a ``prysm_amd.pending.DevicePendingAttestations``)
    and ``ring`` (a ``prysm_amd.pending.DeviceRecentHashes``).  The reference appends every candidate
    block's hash to RecentBlockHashes in place (computeNewActiveState, core.go:223-237, on the pointer
    of service.go:346), so block k reads a window shifted by the candidates before it
    (getSignedParentHashes, core.go:348-360): the other ``*_serialized_blocks`` functions work against
    ONE chain state and are exact for one block at a time only.

    After one upload: split, decode and checks with ``n_recent = 128`` (the statuses read only the
    ring's length, which a chain from genesis never changes); the block gate, with ``eligible`` (one
    0/1 per block, None: all; the caller's parent check, service.go:261-269, and CanProcessBlock,
    :272, :308) folded into its block status on the device; Block.Hash over the blocks
    (``pz_dev_blake2b512_spans``); the walk (``pz_dev_block_walk``: the candidate rule of
    service.go:320-333 as scans, the rows' ``parents_start`` made absolute in the log ``[ring | this
    run's candidate hashes]``, the ring rolled); ONE host read -- the gate's flag word and report with
    the walk's result record and codes; then ``cache.tally_columns`` and ``pool.append_columns`` over
    the log, and with ``want_digests`` the processAttestation message digests over it.  No hash list
    comes from the host.

    ``has_candidate`` / ``candidate_slot``: the candidate block pending before the run (carry the
    returned pair into the next call).  The run stops before the first candidate that is a cycle
    transition (``slot >= last_state_recalc + 64``, core.go:181-183), which the caller handles with
    ``state_recalc_resident``; the call right after a transition block takes ``lag=1`` with the
    pre-transition scalars, table and balances, and stops one past its first candidate.  Blocks at or
    past ``stop`` are untouched (walk code 3): submit them again.

    Where the reference would panic on some row of the run ``ChainPanic`` is raised and nothing lands:
    neither cache, pool nor ring.  Returns a dict: ``walk`` (uint8 per block, WALK_*), ``report`` (the
    gate's), ``stop``, ``ncand``, ``has_candidate``, ``candidate_slot``, ``att_first``, ``att_status``
    (the checks' statuses), ``parents_start`` (absolute: positions in the log), ``block_hash`` (n, 32)
    and, with ``want_digests``, ``msg`` (natt, 64) / ``msg_len``: zero for a row that is not PROCESSED
    or whose block is ineligible or deferred."""
    return _walk(cache, pool, ring, None, data, offsets, last_justified_slot, last_state_recalc, shard_and_committees, balance,
                 eligible, has_candidate, candidate_slot, lag, want_digests, device)


def walk_serialized_blocks_saved(cache, pool, ring, saved, data, offsets, last_justified_slot, last_state_recalc,
                                 shard_and_committees, balance, eligible=None, has_candidate=False, candidate_slot=0, lag=0,
                                 want_digests=False, device=0):
    """:func:`walk_serialized_blocks` with the parent check (``hasBlock(block.ParentHash())``,
    service.go:261-269) taken on the device too, from ``saved`` (a
    ``prysm_amd.pending.DeviceSavedBlocks``: the hashes of the blocks the DB holds,
    ``pz_dev_block_parents``): a block's parent may be a block of the same run, which is itself saved
    only if ITS parent was -- the device resolves that chain by pointer jumping -- and ``eligible``
    then means CanProcessBlock alone (service.go:272, :308).  The set is first given room for its
    count plus the run (from the count last read); the device then queues hash -> parents -> gate ->
    walk -> insert: the hashes of the run's saved and candidate blocks before ``stop`` go into the set
    (``pz_dev_block_set_insert_walked``; service.go:324).  Still one upload and one host read: the
    read also brings ``parent_ok`` (uint8 per block: 0 where the reference answers "parent does not
    exist"), which the returned dict gains, and the set's new count.  A ``ChainPanic`` leaves the set
    as it was.  (A function of its own rather than a ``saved=`` argument: the parameter list of
    :func:`walk_serialized_blocks` is pinned.)"""
    if saved is None:
        raise PzError(_lib.PZ_EINVAL, "saved is None: walk_serialized_blocks is the form without a set")
    return _walk(cache, pool, ring, saved, data, offsets, last_justified_slot, last_state_recalc, shard_and_committees, balance,
                 eligible, has_candidate, candidate_slot, lag, want_digests, device)


def _walk(cache, pool, ring, saved, data, offsets, last_justified_slot, last_state_recalc, shard_and_committees, balance,
          eligible, has_candidate, candidate_slot, lag, want_digests, device):
    """The body of :func:`walk_serialized_blocks` (``saved`` None) and :func:`walk_serialized_blocks_saved`."""
    import torch

    data = np.ascontiguousarray(_lib.as_u8(data), dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    if lag not in (0, 1):
        raise PzError(_lib.PZ_EINVAL, "lag %r: 0 or 1" % (lag,))
    # (the span hash reads whole dwords: 4 bytes of slack after the last block)
    payload = np.concatenate([data[:int(offsets[-1])] if n else data[:0], np.zeros(4, np.uint8)])
    d = _split_decode_check(payload, offsets, last_justified_slot, last_state_recalc, 128, shard_and_committees, device,
                            want_committee=True)
    dev, natt, blk = d["dev"], d["natt"], d["blk"]
    el = None
    if eligible is not None:
        el = _to_device(np.ascontiguousarray(eligible, dtype=np.uint8), dev)
        if el.numel() != n:
            raise PzError(_lib.PZ_EINVAL, "eligible holds %d entries for %d blocks" % (el.numel(), n))
    q = _queue_run(d, int(offsets[-1]) if n else 0, _fold_eligible(blk["status"], el), saved, 4)
    p = _lib.dptr
    base = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    log = torch.empty(int(lib.dll.pz_block_walk_scratch_bytes(n, natt)), dtype=torch.uint8, device=dev)
    # IsCycleTransition reads the chain's CrystallizedState AFTER updateHead (service.go:320-321, :345):
    # right after a transition block that is the new one, a cycle on, while the checks above read the old
    walk_lsr = (int(last_state_recalc) + (64 if lag else 0)) & ((1 << 64) - 1)
    b = _lib.BlockWalkBatch(nblocks=n, slot_number=p(blk["slot_number"]), report=p(q["report"]), block_hash=p(q["block_hash"]),
                            has_candidate=int(bool(has_candidate)), candidate_slot=int(candidate_slot),
                            last_state_recalc=walk_lsr, lag=int(lag), natt=natt, att_block=p(blk["att_block"]),
                            vote_status=p(q["vote_status"]), pend_take=p(q["pend_take"]), parents_start=p(d["parents_start"]),
                            walk=p(q["walk"]), base=p(base), result=p(q["result"]), log=p(log), flags=p(q["flags"]))
    lib.call("pz_dev_block_walk", ring._h, ctypes.byref(b), q["sh"])
    _, panic, out = _read_run(q, d, saved, (0, 0, int(bool(has_candidate)), int(candidate_slot) if has_candidate else 0))
    if panic:
        raise ChainPanic(_RUN_PANIC)
    if natt:
        cache.tally_columns(d["att"], natt, q["vote_status"], d["committee"], d["parents_start"], log,
                            _to_device(_members(shard_and_committees), dev), d["table"][3],
                            _to_device(np.ascontiguousarray(balance, dtype=np.uint64), dev))
        pool.append_columns(d["att"], natt, d["status"].contiguous(), d["committee"], take=q["pend_take"])
    return _run_outputs(out, d, q["walk"], q["block_status"], q["block_hash"], log, want_digests)


_RUN_PANIC = ("a block of the run makes the reference panic (processAttestation or "
              "calculateBlockVoteCache: slice bounds, core.go:353, or committee index, core.go:367)")


def _fold_eligible(block_status, el):
    """The gate's block status with ``el`` (a uint8 device tensor, one 0/1 per block; None: all)
    folded in: an ineligible block gets a status that is not PZ_OK, which closes it."""
    import torch

    return block_status if el is None else torch.where(el != 0, block_status, torch.full_like(block_status, _INELIGIBLE))


def _queue_run(d, nbytes, block_status, saved, result_words, extra=0):
    """What a walked run queues before its scan, on the current stream, over :func:`_decode_check`'s
    tensors ``d`` (``nbytes`` of block bytes) and the folded ``block_status``: with ``saved`` (a
    ``DeviceSavedBlocks``, else None) Block.Hash, the parent check, which hands the gate a status
    that closes a block whose parent is not saved, and the gate; without it the gate, then
    Block.Hash.  It allocates the one read-back buffer, ``result | set count | flags | report | walk |
    parent_ok | extra`` (``result_words``: the scan's result record; the count and ``parent_ok`` only with a
    set; ``extra`` bytes of the caller's, to come along in the read).  Returns a dict of device
    tensors: ``word`` (the buffer) with its views ``result``,
    ``flags``, ``report`` and ``walk``, ``block_hash``, the ``block_status`` the gate took,
    ``parent_ok`` (None without a set), ``vote_status`` and ``pend_take``; ``at``, the byte offset
    each part of the buffer starts at; and ``sh``, the stream."""
    import torch

    dev, n = d["dev"], d["n"]
    sh = _lib.stream_ptr(dev)
    block_hash = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    hash_blocks = lambda: lib.call(  # noqa: E731
        "pz_dev_blake2b512_spans", d["d_bytes"].data_ptr(), d["d_offs"][:-1].data_ptr(), d["d_offs"][1:].data_ptr(), n,
        block_hash.data_ptr() if n else None, 32, sh)
    parent_ok = None
    if saved is not None:
        hash_blocks()
        block_status, parent_ok = _parents(saved, d, nbytes, block_status, block_hash)
    at = {"count": 8 * result_words}
    at["flags"] = at["count"] + (8 if saved is not None else 0)
    at["report"] = at["flags"] + 4
    at["walk"] = at["report"] + n
    at["parent_ok"] = at["walk"] + n
    at["extra"] = at["parent_ok"] + (0 if saved is None else n)
    word, report, vote_status, pend_take, flags = _gate(d, None, block_status, head=at["flags"],
                                                        tail=(n if saved is None else 2 * n) + extra)
    if saved is None:
        hash_blocks()
    return {"at": at, "sh": sh, "word": word, "result": word[:at["count"]].view(torch.int64), "flags": flags, "report": report,
            "walk": word[at["walk"]:at["parent_ok"]], "block_hash": block_hash, "block_status": block_status,
            "parent_ok": parent_ok, "vote_status": vote_status, "pend_take": pend_take}


def _read_run(q, d, saved, empty):
    """Behind the scan of :func:`_queue_run`'s ``q``: with ``saved``, ``parent_ok`` into the buffer
    (device to device: it comes along) and the walked hashes into the set, which leaves its new
    count there (``pz_dev_block_set_insert_walked``; service.go:324); then the ONE host read.
    The caller's ``extra`` bytes come back as ``q["extra_host"]``.
    Returns ``(record, panic, out)``: the scan's result record as ints (``empty`` for a run of no
    block, which launches nothing), the gate's panic bit -- with it nothing rolled and nothing was
    inserted -- and the dict a walked run returns, so far."""
    n, at, word = d["n"], q["at"], q["word"]
    if saved is not None and n:
        word[at["parent_ok"]:at["extra"]].copy_(q["parent_ok"][:n])
        lib.call("pz_dev_block_set_insert_walked", saved._h, _lib.dptr(q["block_hash"]), _lib.dptr(q["walk"]), _lib.dptr(q["flags"]),
                 n, word[at["count"]:].data_ptr(), q["sh"])
    host = word.cpu().numpy()  # the one read
    panic = bool(host[at["flags"]:at["report"]].view(np.uint32)[0] & 1)
    record = tuple(int(x) for x in host[:at["count"]].view(np.uint64)) if n else tuple(empty)
    if saved is not None and n and not panic:
        saved._count = int(host[at["count"]:at["flags"]].view(np.uint64)[0])
    out = {"walk": host[at["walk"]:at["parent_ok"]].copy(), "report": host[at["report"]:at["walk"]].copy(), "stop": record[0],
           "ncand": record[1], "has_candidate": bool(record[2]), "candidate_slot": record[3]}
    if saved is not None:
        out["parent_ok"] = host[at["parent_ok"]:at["extra"]].copy()
    q["extra_host"] = host[at["extra"]:].copy()
    return record, panic, out


def _members(shard_and_committees):
    """Every committee's members in table order: the tally's ``members`` beside ``_committee_table``'s coffs."""
    return np.ascontiguousarray([v for arr in shard_and_committees for e in arr for v in e[1]] or [0], dtype=np.uint32)


def _parents(saved, d, nbytes, block_status, block_hash):
    """The parent check of a run on the current stream, behind Block.Hash: room in ``saved`` for its
    count plus the run, then ``pz_dev_block_parents`` over :func:`_decode_check`'s tensors ``d``.
    Returns ``(block_status_out, parent_ok)`` device tensors: the gate's ``block_status``, which
    closes a block whose parent is not saved, and one byte per block."""
    import torch

    dev, n, natt, blk = d["dev"], d["n"], d["natt"], d["blk"]
    p = _lib.dptr
    saved.reserve((saved.count() if saved._count is None else saved._count) + n, device_form=True)
    saved0 = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    status_out = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    parent_ok = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    scratch = torch.empty(int(lib.dll.pz_block_parents_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    b = _lib.BlockParentsBatch(
        nblocks=n, bytes=p(d["d_bytes"]), nbytes=nbytes, bytes_beg=p(blk["bytes_beg"]),
        bytes_len=p(blk["bytes_len"]), slot_number=p(blk["slot_number"]), block_hash=p(block_hash),
        att_first=p(blk["att_first"]), block_status=p(block_status.contiguous()), rec_status=p(d["rec"]),
        att_status=p(d["status"].contiguous()), natt=natt, parent_ok=p(parent_ok), saved0=p(saved0),
        block_status_out=p(status_out))
    lib.call("pz_dev_block_parents", saved._h, ctypes.byref(b), p(scratch), _lib.stream_ptr(dev))
    return status_out[:n], parent_ok


def _store_select(d, q):
    """``pz_dev_block_store_select`` behind the scan of :func:`_queue_run`'s ``q`` (with a set), on its
    stream, over :func:`_decode_check`'s tensors ``d`` (``natt > 0``): ``stop`` is word 0 of the scan's
    result record, read on the device.  Returns the device tensors ``rows``, ``span`` (room for every
    row), ``first`` (n + 1) and ``count`` (one word: the saved rows)."""
    import torch

    dev, n, natt, blk = d["dev"], d["n"], d["natt"], d["blk"]
    p = _lib.dptr
    rows = torch.empty(natt, dtype=torch.int32, device=dev)
    span = torch.empty((natt, 2), dtype=torch.int64, device=dev)
    first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = torch.empty(int(lib.dll.pz_block_store_scratch_bytes(n, natt)), dtype=torch.uint8, device=dev)
    status = d["status"].contiguous()
    b = _lib.BlockStoreBatch(nblocks=n, att_first=p(blk["att_first"]), block_status=p(d["block_status"]), parent_ok=p(q["parent_ok"]),
                             stop=p(q["result"]), natt=natt, att_block=p(blk["att_block"]), att_status=p(status), rec_status=p(d["rec"]),
                             att_beg=p(blk["att_beg"]), att_end=p(blk["att_end"]), rows=p(rows), span=p(span), first=p(first),
                             count=p(count))
    lib.call("pz_dev_block_store_select", ctypes.byref(b), p(scratch), q["sh"])
    return {"rows": rows, "span": span, "first": first, "count": count}


def store_writes(out, data):
    """The database writes of a ``ResidentChain`` dict ``out`` (a call with ``store`` on) over the
    call's ``data``, in the reference's order, as ``(key, value, append)`` triples with the prefixes
    of blockchain/schema.go:31-34: per block, in block order, for each of its saved rows
    ``(b"attestation-" + key, the record's bytes, False)`` -- db.Put, a key written twice keeps the
    later value (core.go:650-658) -- and then, if it saved any, ``(b"attestationHashes-" + block_hash,
    the block's segment of ``lists``, True)``: saveAttestationHash appends to whatever list the
    database holds under the key (core.go:745-760), so a block received twice grows its list."""
    st = out["store"]
    data = _lib.as_u8(data)
    first, lists = st["first"], st["lists"].tobytes()
    for j in range(len(first) - 1):
        lo, hi = int(first[j]), int(first[j + 1])
        for i in range(lo, hi):
            yield b"attestation-" + st["key"][i].tobytes(), data[int(st["span"][i, 0]):int(st["span"][i, 1])].tobytes(), False
        if hi > lo:
            yield b"attestationHashes-" + out["block_hash"][j].tobytes(), lists[34 * lo:34 * hi], True


def _run_outputs(out, d, walk, block_status, block_hash, log, want_digests):
    """What a walked run returns per row and per block, added to ``out``: with ``want_digests`` the
    message digests over the log (zero for a row that is not PROCESSED or whose block is ineligible
    or deferred), then ``att_first``, ``att_status``, ``parents_start`` and ``block_hash``."""
    import torch

    n, natt, blk, status = d["n"], d["natt"], d["blk"], d["status"]
    if want_digests:
        if natt:
            att_block = blk["att_block"][:natt].long()
            ran = (walk[att_block] != WALK_DEFERRED) & (block_status[att_block] == _lib.PZ_OK)
            msg_status = torch.where(ran, status, torch.full_like(status, ATT_NOT_PROCESSED)).contiguous()
            msg, msg_len = attestation_messages_device(d["att"], natt, msg_status, d["parents_start"], log, 129 + n)
            out["msg"], out["msg_len"] = msg.cpu().numpy(), msg_len.cpu().numpy().view(np.uint32)
        else:
            out["msg"], out["msg_len"] = np.zeros((0, 64), np.uint8), np.zeros(0, np.uint32)
    out["att_first"] = blk["att_first"].cpu().numpy().view(np.uint64)
    out["att_status"] = status.cpu().numpy()
    out["parents_start"] = d["parents_start"][:natt].cpu().numpy().view(np.uint64)
    out["block_hash"] = block_hash.cpu().numpy()
    return out


def state_recalc_device(pool, cache, state, recent_hashes, block_slot):
    """stateRecalc (blockchain/core.go:398-497) composed from what lives on the device: ``pool`` (a
    ``prysm_amd.pending.DevicePendingAttestations``: ActiveState.PendingAttestations), ``cache`` (a
    ``prysm_amd.votes.DeviceVoteCache`` or anything with ``items()``; None: no entry), ``state`` (a
    ``prysm_amd.pending.RecalcState``, advanced in place), ``recent_hashes`` = RecentBlockHashes()
    and ``block_slot`` = the transition block's SlotNumber.

    1. the 64-iteration justification loop (core.go:411-431) on the host, over ``cache.items()``
       and ``recent_hashes[:64]``;
    2. ``pz_dev_epoch_count`` then ``pz_dev_epoch_finish`` with one instance over the pool's view,
       on the current stream: processCrosslinks' tallies on the pre-reward balances, the winners,
       CalculateRewards in place and the next-cycle total (core.go:433-464);
    3. ``scal`` and ``winner`` come back; where the reference panics ``ChainPanic`` is raised and, by
       the kernels' contract, the balances are untouched;
    4. the records of the shards with a winner get {dynasty, block_slot, the winner's ShardBlockHash}
       (core.go:549-555);
    5. the pool is pruned to ``slot > last_state_recalc`` (core.go:444-450);
    6. the new scalars (core.go:467-478): last_state_recalc + 64, justified / streak / finalized,
       total_deposits = the next-cycle balance -- and current_dynasty 0, which the reference's new
       state leaves unset.
    Returns the winners (one attestation row per record, 0xFFFFFFFF: none)."""
    import torch

    from prysm_amd import pb

    M64 = (1 << 64) - 1
    from prysm_amd.pending import recent_of

    lsr = state.last_state_recalc
    recent = _recent_array(recent_of(recent_hashes)[0])
    if len(recent) < 64:
        raise ChainPanic("stateRecalc: RecentBlockHashes()[i], index out of range (core.go:413)")
    totals = cache.items() if cache is not None else {}
    streak, justified, finalized = state.justified_streak, state.last_justified_slot, state.last_finalized_slot
    for i in range(64):
        slot = (lsr - 64 + i) & M64
        bal = totals.get(recent[i].tobytes(), 0)
        if (3 * bal) & M64 >= (2 * state.total_deposits) & M64:
            justified = max(justified, slot)
            streak = (streak + 1) & M64
        else:
            streak = 0
        if streak >= 65 and ((slot - 64) & M64) > finalized:
            finalized = (slot - 64) & M64

    dev = state.balance.device
    n, nrec = state.nval, len(state.crosslink_records)
    b = pool.epoch_batch()
    natt = int(b.natt)
    i64 = lambda v: _to_device(np.array(v, dtype=np.uint64), dev)  # noqa: E731
    dynasty, tdep = i64([state.current_dynasty]), i64([state.total_deposits])
    rec_dynasty = i64([r.dynasty for r in state.crosslink_records] or [0])
    winner = torch.full((max(nrec, 1),), -1, dtype=torch.int32, device=dev)
    red = torch.zeros(_lib.SCAL_COUNT + 2 * max(natt, 1), dtype=torch.int64, device=dev)
    act_mask = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    blk_cnt = torch.zeros((n + 2047) // 2048 + 1, dtype=torch.int32, device=dev)
    act_list = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    b.nval, b.val_offset, b.nval_global, b.kind = n, 0, n, _lib.KIND_ACTIVE
    b.balance, b.start, b.end = state.balance.data_ptr(), state.start.data_ptr(), state.end.data_ptr()
    b.dynasty, b.total_deposit = dynasty.data_ptr(), tdep.data_ptr()
    b.pop_rank, b.pop_world = 0, 1
    b.committee, b.coffs = state.members.data_ptr(), state.coffs.data_ptr()
    b.nrec, b.rec_dynasty, b.winner = nrec, rec_dynasty.data_ptr(), winner.data_ptr()
    b.scal = red.data_ptr()
    b.vote, b.total = red[_lib.SCAL_COUNT:].data_ptr(), red[_lib.SCAL_COUNT + max(natt, 1):].data_ptr()
    b.act_mask, b.blk_cnt, b.act_list = act_mask.data_ptr(), blk_cnt.data_ptr(), act_list.data_ptr()
    sh = _lib.stream_ptr(dev)
    lib.call("pz_dev_epoch_count", ctypes.byref(b), sh)
    lib.call("pz_dev_epoch_finish", ctypes.byref(b), sh)
    scal = red[:_lib.SCAL_COUNT].cpu().numpy().view(np.uint64)
    win = winner.cpu().numpy().view(np.uint32)[:nrec]
    if scal[_lib.SCAL_ERR_XL]:
        raise ChainPanic("processCrosslinks: index out of range (committee member, bitfield or shard)")
    thr = (int(scal[_lib.SCAL_POP]) * 32 * 3) & M64 >= (state.total_deposits * 2) & M64
    if thr and scal[_lib.SCAL_NACT] > 0 and scal[_lib.SCAL_ERR_RWD]:
        raise ChainPanic("CalculateRewards: CheckBit index out of range (incentives.go:23)")
    shards = np.nonzero(win != 0xFFFFFFFF)[0]
    for s, h in zip(shards, pool.shard_block_hashes(win[shards])):
        state.crosslink_records[int(s)] = pb.CrosslinkRecord(state.current_dynasty, h, int(block_slot))
    pool.prune(lsr)
    state.last_state_recalc = (lsr + 64) & M64
    state.justified_streak, state.last_justified_slot, state.last_finalized_slot = streak, justified, finalized
    state.total_deposits = int(scal[_lib.SCAL_NEXT_BAL])
    state.current_dynasty = 0
    return win


def state_recalc_resident(pool, cache, state, recent_hashes, block_slot):
    """stateRecalc (blockchain/core.go:398-497) as ONE ABI call, ``pz_dev_state_recalc``, over what
    lives on the device: ``pool`` (a ``prysm_amd.pending.DevicePendingAttestations``), ``cache`` (a
    ``prysm_amd.votes.DeviceVoteCache``, looked up on the device -- the map is not downloaded; None:
    no entry) and ``state`` (a ``prysm_amd.pending.ResidentRecalcState``, advanced in place).
    ``recent_hashes`` = RecentBlockHashes() (a list, an array, or a
    ``prysm_amd.pending.DeviceRecentHashes``, read where it lies) and ``block_slot`` = the transition
    block's SlotNumber.  Computes what ``state_recalc_device`` computes and raises ``ChainPanic`` where it does; a
    pending ShardBlockHash longer than the state's ``hash_stride`` is refused whole (PZ_ERANGE).
    Returns the winners (one attestation row per record, 0xFFFFFFFF: none)."""
    from prysm_amd.pending import DeviceRecentHashes

    dev = state.balance.device
    if isinstance(recent_hashes, DeviceRecentHashes):  # read where it lies: nothing is uploaded
        d_recent, n_recent = recent_hashes.view()[0], recent_hashes.WINDOW
    else:
        recent = _recent_array(recent_hashes)
        d_recent, n_recent = _to_device(recent if len(recent) else np.zeros((1, 32), np.uint8), dev), len(recent)
    return _recalc_resident(pool, cache, state, d_recent, n_recent, block_slot)["winner"]


def _recalc_resident(pool, cache, state, d_recent, n_recent, block_slot):
    """``pz_dev_state_recalc`` with ``d_recent`` (a uint8 device tensor, read where it lies) as
    RecentBlockHashes(), then the handle's one read: ``ResidentRecalcState.read()``'s dict."""
    import torch

    dev = state.balance.device
    b = _lib.RecalcBatch(nval=state.nval, balance=state.balance.data_ptr(), start=state.start.data_ptr(),
                         end=state.end.data_ptr(), members=state.members.data_ptr(), coffs=state.coffs.data_ptr(),
                         recent=d_recent.data_ptr(), n_recent=n_recent, block_slot=int(block_slot))
    nbytes = int(lib.dll.pz_state_recalc_scratch_bytes(state.nval, int(pool.caps[0]), state.nrec))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.dll.pz_dev_state_recalc(state._h, pool._h, cache._h if cache is not None else None, ctypes.byref(b),
                                     scratch.data_ptr(), _lib.stream_ptr(dev))
    msg = lib.dll.pz_last_error().decode() if rc != _lib.PZ_OK else ""
    if rc == _lib.PZ_EINDEX:
        raise ChainPanic(msg)
    if rc != _lib.PZ_OK:
        raise _lib.PzError(rc, msg)
    try:
        return state.read()
    except _lib.PzError as e:
        if e.code == _lib.PZ_EINDEX:
            raise ChainPanic(str(e)) from None
        raise


def resident_state_roots(pool, state, recent_hashes, field12, recent_len=None, crosslinking_start_shard=0, dynasty_seed=b"",
                         dynasty_seed_last_reset=0):
    """``(ActiveState.Hash(), CrystallizedState.Hash())`` (types/state.go:138-149, 237-248) -- the two
    digests a proposer writes into a block -- of the states held in ``pool`` (a
    ``prysm_amd.pending.DevicePendingAttestations``) and ``state`` (a
    ``prysm_amd.pending.ResidentRecalcState``), encoded on the device where they lie.
    ``recent_hashes`` / ``recent_len``: as ``DevicePendingAttestations.active_state``; ``field12`` and
    the remaining arguments: as ``ResidentRecalcState.wire``."""
    return (pool.active_state_root(recent_hashes, recent_len),
            state.root(field12, crosslinking_start_shard, dynasty_seed, dynasty_seed_last_reset))


_NO_T = (1 << 64) - 1  # pz_block_cycle_batch.result's t_index without a transition block


class _CacheRoom:
    """``ResidentChain``'s ``cache_policy`` (its text has the rules) over ``cache``, a
    ``DeviceVoteCache``: the bounds, the counters and every step that is the policy's own.  Under
    ``"fixed"`` it asks for no byte of the read, queues nothing and never calls ``cache``."""

    def __init__(self, cache, policy):
        self.cache, self.policy = cache, policy
        self.extra_bytes = 0 if policy == "fixed" else 16  # of the run's one read: the two landings' oblique sums
        self.retains = 0  # retains queued ("retire")
        self.grows = 0    # reserves that raised the capacity ("grow", "retire")
        # host-side upper bounds, never read back: the slots in use, and whether the ring's 129 hashes
        # are counted in it already (the landing of a run counts the run's whole log, which holds the next ring)
        self.slots_ub = len(cache.read(strict=False)[1]) if self.extra_bytes else 0
        self.ring_counted = False
        self._run_counted = False  # the run's log is counted in slots_ub: at most once across its two landings

    def queue(self, dst, n_oblique, vote):
        """Queues into ``dst``, its bytes of the read-back buffer, the oblique elements of the rows
        each landing tallies (``vote``: the two landings' vote statuses of the run's rows)."""
        if self.extra_bytes:
            import torch

            dst.copy_(torch.stack([(n_oblique * (vote[k] == ATT_PROCESSED)).sum() for k in (0, 1)]).view(torch.uint8))

    def parse(self, got):
        """The two landings' oblique sums from its bytes of the read."""
        return [int(x) for x in np.frombuffer(got.tobytes(), dtype=np.uint64)] if self.extra_bytes else [0, 0]

    def begin(self):
        """Before the first landing of a run that lands."""
        self._run_counted = False

    def fit(self, oblique, nlog, log):
        """Before a landing's tally, which adds ``oblique`` slots at most beside the first ``nlog``
        hashes of ``log``: the bounds fit, or the policy makes them."""
        if not self.extra_bytes:
            return
        cache = self.cache
        need = oblique + (0 if self._run_counted else nlog - (129 if self.ring_counted else 0))
        if self.slots_ub + need > cache.slot_cap:
            if self.policy == "retire":  # the kept entries and the log's new ones are the log's hashes
                cache.retain(log[:32 * nlog])
                self.retains += 1
                self.slots_ub, need = nlog, oblique
            if self.slots_ub + need > cache.slot_cap:
                cache.reserve(max(self.slots_ub + need, min(2 * cache.slot_cap, 1 << 30)), device_form=True)
                self.grows += 1
        self.slots_ub += need
        self._run_counted = True

    def end(self, ncand):
        """Behind a run that landed: the next ring is log entries [ncand, ncand + 129), counted iff
        this run's log was, or nothing rolled."""
        self.ring_counted = self._run_counted or (self.ring_counted and ncand == 0)


class _PoolRoom:
    """``ResidentChain``'s ``pool_policy`` (its text has the rules) over ``pool``, a
    ``DevicePendingAttestations``, as :class:`_CacheRoom` is the cache's."""

    def __init__(self, pool, policy):
        self.pool = pool
        self.extra_bytes = 0 if policy == "fixed" else 112  # of the run's one read: the two landings' seven needs
        self.grows = 0  # reserves that raised a capacity
        # host-side upper bounds of the pool's seven counts (exact here, stale upward behind a prune)
        self.counts_ub = [int(x) for x in pool.counts(strict=False)] if self.extra_bytes else None

    def queue(self, dst, cols, n, status, take):
        """Queues into ``dst``, its bytes of the read-back buffer, what each landing's append of the
        run's rows would add to the seven counts (``take``: the two landings' take columns)."""
        if self.extra_bytes:
            import torch

            dst.copy_(self.pool.need_columns(cols, n, status, take[0], take[1]).view(torch.uint8).reshape(-1))

    def parse(self, got):
        """The two landings' seven needs from its bytes of the read."""
        return np.frombuffer(got.tobytes(), dtype=np.uint64).reshape(2, 7).tolist() if self.extra_bytes else [None, None]

    def fit(self, need):
        """Before a landing's append, which adds ``need`` (seven ints) to the counts: the bounds fit
        the capacities, or a reserve makes them."""
        if not self.extra_bytes:
            return
        pool = self.pool
        cap = [int(x) for x in pool.caps]
        if any(u + a > c for u, a, c in zip(self.counts_ub, need, cap)):
            self.counts_ub = [int(x) for x in pool.counts(strict=False)]  # the one wait of this path
            want = [u + a for u, a in zip(self.counts_ub, need)]
            if any(w > c for w, c in zip(want, cap)):
                pool.reserve([min(max(w, 2 * c), (1 << 40) - 1) if w > c else c for w, c in zip(want, cap)], device_form=True)
                self.grows += 1
        self.counts_ub = [u + a for u, a in zip(self.counts_ub, need)]


class ResidentChain:
    """blockProcessing (blockchain/service.go:229-363) over the resident objects, transition blocks
    included: ``cache`` (a ``prysm_amd.votes.DeviceVoteCache``), ``pool`` (a
    ``prysm_amd.pending.DevicePendingAttestations``), ``ring`` (a ``DeviceRecentHashes``), ``saved`` (a
    ``DeviceSavedBlocks``) and ``state`` (a ``ResidentRecalcState``), with ``shard_and_committees`` =
    ShardAndCommitteesForSlots, which stateRecalc hands on unchanged (core.go:469): its device form is
    built here, once.  The balances are ``state.balance``, read where they lie by both tallies.

    The object keeps the host side of the carry between calls: ``has_candidate`` /
    ``candidate_slot`` (candidateBlock), ``lag`` (1: the pending candidate is a transition block, so
    its states are not the chain's yet) and, while ``lag`` is set, the chain's own
    ``(last_justified_slot, last_state_recalc)`` beside the candidate's, which are the state
    handle's.  That pair and the ring's history entry are all that tells the two pairs of states
    apart: CalculateRewards writes the balances in place (casper/incentives.go:22-28) on the slice
    stateRecalc hands to the new state (core.go:468), so the chain's old CrystallizedState tallies
    with the rewarded balances from the transition block on.

    The two policies are keyword-only arguments, checked before any other argument is touched.
    Each one's bounds, counters and steps are one object's (``_CacheRoom``, ``_PoolRoom``), which a
    landing asks for room (``fit``) before its tally and before its append.

    ``cache_policy``: the reference's map only grows, and a tally that needs more slots than the
    cache has left lands nothing and sets the sticky PZ_ERANGE.  ``"fixed"`` (the default) leaves it
    at that: the cache's ``slot_cap`` bounds the chain.  With the other two a tally never meets that
    error.  The driver keeps an upper bound of the slots in use and, per landing, of the slots it can
    add -- the run's hash log (the ring's 129 entries, where no earlier landing counted them, and the
    run's candidates) plus the oblique elements of the rows that land, two sums formed on the device
    that come along in the run's one read.  Where the bounds do not fit, ``"grow"`` reserves at least
    the need, doubling (``DeviceVoteCache.reserve``): the map as the reference keeps it.  ``"retire"``
    first retains the run's hash log, which already lies on the device (``DeviceVoteCache.retain``):
    every window this call's stateRecalc and any later one can read (votecache_dev.h holds the
    argument and what it leaves out), and reserves only if the log and the need still do not fit.
    ``cache_retains`` and ``cache_grows`` count them.

    ``pool_policy``: the reference's PendingAttestations is a slice that append grows
    (core.go:223-237), and an append that would exceed one of the pool's seven capacities lands
    nothing and sets the sticky PZ_ERANGE.  ``"fixed"`` (the default) leaves it at that and queues
    nothing.  With ``"grow"`` an append never meets that error: the driver keeps upper bounds of the
    seven counts (one ``pool.counts()`` when the object is made), and per submission
    ``pz_dev_att_pool_need`` forms on the device what each landing's append would add; its 112 bytes
    come along in the run's one read, beside the cache policy's.  Where bound + need exceeds a
    capacity the bounds are first replaced by ``pool.counts()`` (they go stale upward behind a
    stateRecalc's prune; one wait, on this path only), and if they still do not fit each short
    column is reserved to ``max(bound + need, 2 * capacity)`` (``DevicePendingAttestations.reserve``
    on the stream).  ``pool_grows`` counts the reserves that raised a capacity.  Nothing bounds the
    pool's memory here: the reference's own prune does.

    ``store`` (a plain attribute, False by default, read at each call): with it on every returned
    dict carries ``out["store"]``, the call's attestation store batch -- exactly the attestation
    writes blockProcessing makes for the blocks the call processed (saveAttestation and
    saveAttestationHash, service.go:288-297), selected, hashed and encoded on the device
    (``pz_dev_block_store_select`` behind ``pz_dev_block_cycle``, its count in the run's one read;
    ``pz_dev_block_store_digests`` behind the read; one further read brings the batch).  A dict of
    numpy arrays over the ``m`` saved rows: ``rows`` (m, ascending row indices), ``first`` (n + 1:
    block j's saved rows are ``[first[j], first[j + 1])``), ``span`` (m, 2: the records' byte ranges in
    the caller's ``data``, the value saveAttestation writes), ``key`` (m, 32: Attestation.Key()),
    ``hash`` (m, 32: Attestation.Hash()) and ``lists`` (34 m bytes: entry i is ``0a 20 | hash[i]``,
    so block j's appended bytes are ``lists[34 * first[j]:34 * first[j + 1]]``).  Which rows are saved
    is prysm_amd/csrc/blockstore_dev.h's rule: it reads neither ``eligible`` nor the outcome of a
    block's last attestation.  When a call is submitted twice the store is the second submission's,
    the one that landed; on ``ChainPanic`` nothing is returned.  :func:`store_writes` turns a dict
    into database writes.  With ``store`` off no byte and no launch is added."""

    CACHE_POLICIES = ("fixed", "grow", "retire")
    POOL_POLICIES = ("fixed", "grow")
    store = False  # with it on, every returned dict carries the call's attestation store batch

    def __init__(self, cache, pool, ring, saved, state, shard_and_committees, device=0, *, cache_policy="fixed", pool_policy="fixed"):
        for what, value, known in (("cache_policy", cache_policy, self.CACHE_POLICIES), ("pool_policy", pool_policy, self.POOL_POLICIES)):
            if value not in known:  # before any argument is touched
                raise PzError(_lib.PZ_EINVAL, "%s %r: one of %s" % (what, value, ", ".join(known)))
        import torch

        self.cache, self.pool, self.ring, self.saved, self.state = cache, pool, ring, saved, state
        self.cache_policy, self.pool_policy = cache_policy, pool_policy
        self.device = device
        dev = torch.device("cuda", device)
        if shard_and_committees is None:  # (from_state: the table as the loader left it on the device)
            self._narr, self._table, self._members = state.narr, list(state.table), state.members
        else:
            self._narr = len(shard_and_committees)
            self._table = [_to_device(a, dev) for a in _committee_table(shard_and_committees)]
            self._members = _to_device(_members(shard_and_committees), dev)
        self.has_candidate, self.candidate_slot, self.lag = False, 0, 0
        scal = state.read()["scalars"]
        self._cand = (int(scal[2]), int(scal[0]))  # (last_justified_slot, last_state_recalc) of the state handle
        self._chain = None                         # the chain's own pair while lag is set
        self.calls = 0      # submissions so far: one upload and one read each
        self.resubmits = 0  # of them, runs submitted again without the blocks past their stop
        self.spent = False  # a call failed after its host read: the objects no longer match the carry
        self._cache_room, self._pool_room = _CacheRoom(cache, cache_policy), _PoolRoom(pool, pool_policy)

    cache_retains = property(lambda self: self._cache_room.retains)
    cache_grows = property(lambda self: self._cache_room.grows)
    pool_grows = property(lambda self: self._pool_room.grows)

    RUN_BLOCKS = 1024  # process_all's submission: the scan's tile, and far more than a cycle's blocks of one chain
    CAPS = (256, 256 * 32, 256 * 32, 256 * 8, 256, 256 * 32, 512)  # from_state's pool: rows and bytes of four cycles' blocks

    @classmethod
    def from_state(cls, crystallized_bytes, saved_hashes=(), device=0, slot_cap=512, caps=CAPS, hash_stride=32,
                   cache_policy="fixed", pool_policy="fixed"):
        """NewBeaconChain over a database that holds a CrystallizedState (blockchain/core.go:86-95):
        the state decoded on the device from its stored bytes (``ResidentRecalcState.from_state``;
        exactly the canonical encoding is accepted), a fresh vote cache of ``slot_cap`` slots over
        its validators, an empty pending pool of ``caps`` (``pending.CAPS``'s order), the genesis
        ring of 128 empty entries -- the reference reloads no ActiveState (core.go:59-64) -- and the
        saved-block set over ``saved_hashes``, the block hashes the database holds.  The committee
        table is taken from the decoded device tensors: no validator and no member visits the host.
        ``cache_policy``: what a landing does when the cache's slots may not hold it, and
        ``pool_policy``: when the pool's capacities may not (the class's text)."""
        from prysm_amd.pending import DevicePendingAttestations, DeviceRecentHashes, DeviceSavedBlocks, ResidentRecalcState
        from prysm_amd.votes import DeviceVoteCache

        state = ResidentRecalcState.from_state(crystallized_bytes, device=device, hash_stride=hash_stride)
        return cls(DeviceVoteCache(state.nval, slot_cap, device), DevicePendingAttestations(list(caps), device),
                   DeviceRecentHashes(device=device), DeviceSavedBlocks(list(saved_hashes), device=device), state, None, device,
                   cache_policy=cache_policy, pool_policy=pool_policy)

    def chain_scalars(self):
        """``(last_justified_slot, last_state_recalc)`` of the chain's CrystallizedState: what a
        received block is checked against (service.go:281-301)."""
        return self._chain if self.lag else self._cand

    def process_serialized(self, data, offsets, eligible=None, want_digests=False):
        """A run of consecutive received blocks held as bytes, in ONE call, the run's cycle transition
        included.  One upload (offsets, ``eligible`` and bytes in one buffer); then the device queues
        split, decode, the checks with the chain's scalars, Block.Hash, the parent check against
        ``saved``, the gate, ``pz_dev_block_cycle`` and the insert of the walked hashes; then the one
        host read, as :func:`walk_serialized_blocks_saved` makes it.  After it: the tally and the pool
        append of the rows before stateRecalc; with a transition block T in the run
        ``pz_dev_state_recalc`` over the promoted ActiveState's window (log entry ``1 + t_rank``) at
        T's slot; then the tally and the append of the rows after it, against the same balance
        pointer.  The read and the recalc's own are the only waits.

        ``eligible``: CanProcessBlock alone (service.go:272, :308), one 0/1 per block (None: all).
        The run ends behind the block that promotes T's states (or before it, if that block is a
        transition too): blocks at or past ``stop`` are untouched, submit them again
        (:meth:`process_all`).

        Where the reference panics on a row of a block BEFORE ``stop`` ``ChainPanic`` is raised and
        nothing lands.  The checks and the gate run over every block of the upload before the scan
        knows ``stop``, and the gate's one panic bit covers them all; but a block at or past ``stop``
        is not processed by this call, and it was checked against scalars that may be cycles behind
        the ones the reference will check it with (a row's committee index ``slot -
        last_state_recalc`` leaves the table then, core.go:367, without any panic in the reference).
        So when the bit is set and ``stop`` cuts the run, nothing of the first submission has landed
        (the ring, the set, cache and pool are as they were) and the blocks before ``stop`` are
        submitted again alone: a second upload and read, on this path only.  The scan's decisions for a
        block depend on the blocks before it alone, so that submission stops where the first did and
        its bit speaks of the run's own blocks; the outputs returned are the first submission's,
        which cover every block of the call.

        Where stateRecalc itself panics ``ChainPanic`` is raised with the rows before it landed, the
        ring rolled and the set grown -- the reference too tallies and saves before it panics
        (service.go:313-324 precede :345) -- and nothing after it.  After that, or after any other
        error raised behind the host read (a pool or cache capacity, a ShardBlockHash longer than
        the state's ``hash_stride``), the objects no longer match the carry: the object is spent and
        every later call raises.

        Returns :func:`walk_serialized_blocks_saved`'s dict plus ``t_index`` (the transition
        block's index, None: none) and ``lag`` (the lag carried out)."""
        if self.spent:
            raise ChainPanic("an earlier call failed behind its host read: the object is spent")
        data = np.ascontiguousarray(_lib.as_u8(data), dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        if eligible is not None:
            eligible = np.ascontiguousarray(eligible, dtype=np.uint8)
            if eligible.size != n:
                raise PzError(_lib.PZ_EINVAL, "eligible holds %d entries for %d blocks" % (eligible.size, n))
        out, panic = self._submit(data, offsets, eligible, want_digests)
        if panic and out["stop"] < n:
            stop = out["stop"]
            self.resubmits += 1
            head, panic = self._submit(data, offsets[:stop + 1], None if eligible is None else eligible[:stop], False)
            if not panic and (head["stop"], head["ncand"], head["t_index"], head["lag"]) != \
                    (stop, out["ncand"], out["t_index"], out["lag"]):
                self.spent = True
                raise PzError(_lib.PZ_EINVAL, "a run submitted again without its deferred blocks stopped elsewhere")
            if "store" in head:  # the submission that landed; its rows are the call's: a prefix of the same bytes
                out["store"] = head["store"]
                out["store"]["first"] = np.concatenate([head["store"]["first"], np.full(n - stop, head["store"]["first"][-1], np.uint64)])
        if panic:
            raise ChainPanic(_RUN_PANIC)
        return out

    def _submit(self, data, offsets, eligible, want_digests):
        """One upload, the device queue, one read, and -- unless the gate's panic bit is set -- the
        landing.  Returns ``(out, panic)``; with ``panic`` nothing has landed, and the carry and the
        policies' bounds are as they were."""
        up = self._upload(data, offsets, eligible)
        self.calls += 1
        run = self._queue(*up)
        out, panic = self._read(run)
        if not panic:
            self._land_run(run)
        q = run["q"]
        if run["store"] and not panic:
            out["store"] = self._store(run)
        return _run_outputs(out, run["d"], q["walk"], q["block_status"], q["block_hash"], run["log"], want_digests), panic

    def _upload(self, data, offsets, eligible):
        """The one upload, ``offsets | eligible | bytes``, the bytes 16-byte aligned and with 4 bytes
        of slack behind them (the span hash reads whole dwords).  Returns ``(n, nbytes, d_offs, el,
        d_bytes)``: the blocks, their bytes, and the three parts on the device."""
        import torch

        n = len(offsets) - 1
        nbytes = int(offsets[-1]) if n else 0
        o_end = 8 * (n + 1)
        e_end = o_end + n
        b_beg = e_end + (-e_end) % 16
        host = np.zeros(b_beg + nbytes + 4, dtype=np.uint8)
        host[:o_end] = offsets.view(np.uint8)
        host[o_end:e_end] = 1 if eligible is None else eligible != 0
        host[b_beg:b_beg + nbytes] = data[:nbytes]
        up = _to_device(host, torch.device("cuda", self.device))
        return n, nbytes, up[:o_end].view(torch.int64), up[o_end:e_end], up[b_beg:]

    def _extras(self, buf, store):
        """The policies' bytes of the run's one read, side by side at the buffer's ``extra`` offset
        (``buf``: the buffer from there on, on the device or as read): the cache's, then the pool's,
        then, for a run with the ``store`` on, the eight of its count of saved rows."""
        cut = self._cache_room.extra_bytes
        end = cut + self._pool_room.extra_bytes
        return buf[:cut], buf[cut:end], buf[end:end + (8 if store else 0)]

    def _queue(self, n, nbytes, d_offs, el, d_bytes):
        """Everything a run queues on the device behind :meth:`_upload`: split, decode and the checks
        with the chain's scalars, :func:`_queue_run`, ``pz_dev_block_cycle`` and the policies' sums.
        Returns the run, a dict: ``d`` (:func:`_decode_check`'s), ``q`` (:func:`_queue_run`'s), the
        ``lag`` it took, ``log`` (the scan's hash log), ``vote`` / ``take`` (the two landings' columns),
        ``store`` (the attribute as this call read it) and, with it, ``sel`` (:func:`_store_select`'s)."""
        import torch

        dev = torch.device("cuda", self.device)
        lag = int(self.lag)
        store = bool(self.store)
        ljs, lsr = self.chain_scalars()
        d = _decode_check(d_bytes, d_offs, n, ljs, lsr, 128, self._narr, self._table, dev, want_committee=True)
        natt, blk = d["natt"], d["blk"]
        q = _queue_run(d, nbytes, _fold_eligible(blk["status"], el), self.saved, 8,
                       extra=self._cache_room.extra_bytes + self._pool_room.extra_bytes + (8 if store else 0))
        p = _lib.dptr
        base = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        log = torch.empty(int(lib.dll.pz_block_cycle_scratch_bytes(n, natt)), dtype=torch.uint8, device=dev)
        vote = torch.empty((2, max(natt, 1)), dtype=torch.int32, device=dev)
        take = torch.empty((2, max(natt, 1)), dtype=torch.uint8, device=dev)
        # IsCycleTransition reads the state the first candidate promotes (service.go:320-321, :345):
        # the state handle's, which with lag is a cycle ahead of the scalars the checks read
        b = _lib.BlockCycleBatch(nblocks=n, slot_number=p(blk["slot_number"]), report=p(q["report"]), block_hash=p(q["block_hash"]),
                                 has_candidate=int(bool(self.has_candidate)), candidate_slot=int(self.candidate_slot),
                                 last_state_recalc=self._cand[1], lag=lag, natt=natt, att_block=p(blk["att_block"]),
                                 vote_status=p(q["vote_status"]), pend_take=p(q["pend_take"]), parents_start=p(d["parents_start"]),
                                 vote0=vote[0].data_ptr(), vote1=vote[1].data_ptr(), take0=take[0].data_ptr(),
                                 take1=take[1].data_ptr(), walk=p(q["walk"]), base=p(base), result=p(q["result"]), log=p(log),
                                 flags=p(q["flags"]))
        lib.call("pz_dev_block_cycle", self.ring._h, ctypes.byref(b), q["sh"])
        sel = None
        if natt:  # the policies' sums over the rows each landing takes: they come along in the read
            x_cache, x_pool, x_store = self._extras(q["word"][q["at"]["extra"]:], store)
            self._cache_room.queue(x_cache, d["att"]["n_oblique"][:natt], vote[:, :natt])
            self._pool_room.queue(x_pool, d["att"], natt, d["status"].contiguous(), take)
            if store:  # the saved rows, behind the scan: its stop is read where it lies; their count comes along too
                sel = _store_select(d, q)
                x_store.copy_(sel["count"].view(torch.uint8))
        return {"d": d, "q": q, "lag": lag, "log": log, "vote": vote, "take": take, "store": store, "sel": sel}

    def _read(self, run):
        """The one host read of a queued run (:func:`_read_run`).  Adds to the run ``record`` (the
        scan's result record) and, for each landing, ``oblique`` and ``need`` (the policies' sums);
        returns ``(out, panic)``, ``out`` as far as the read fills it."""
        empty = (0, 0, int(bool(self.has_candidate)), int(self.candidate_slot) if self.has_candidate else 0, _NO_T, 0, 0, run["lag"])
        run["record"], panic, out = _read_run(run["q"], run["d"], self.saved, empty)
        t_index, lag_out = run["record"][4], run["record"][7]
        out["t_index"], out["lag"] = None if t_index == _NO_T else t_index, lag_out
        x_cache, x_pool, x_store = self._extras(run["q"]["extra_host"], run["store"])
        run["oblique"], run["need"] = self._cache_room.parse(x_cache), self._pool_room.parse(x_pool)
        run["m"] = int(np.frombuffer(x_store.tobytes(), dtype=np.uint64)[0]) if run["store"] else 0
        return out, panic

    def _store(self, run):
        """The attestation store batch of a read run (``store`` on, no panic): the digests of its
        ``m`` saved rows, queued now that ``m`` sizes them, and the one further read, ``rows | first |
        span | key | hash | lists`` in one buffer.  A run without a saved row launches and reads nothing."""
        import torch

        d, n, m, sel = run["d"], run["d"]["n"], run["m"], run["sel"]
        if not m:
            return {"rows": np.zeros(0, np.uint32), "first": np.zeros(n + 1, np.uint64), "span": np.zeros((0, 2), np.uint64),
                    "key": np.zeros((0, 32), np.uint8), "hash": np.zeros((0, 32), np.uint8), "lists": np.zeros(0, np.uint8)}
        at, end = {}, 0
        for k, size in (("rows", 4 * m), ("first", 8 * (n + 1)), ("span", 16 * m), ("key", 32 * m), ("hash", 32 * m), ("lists", 34 * m)):
            at[k] = (end + (-end) % 16, size)  # (span, key and hash 16-byte aligned, as their kernels want them)
            end = at[k][0] + size
        buf = torch.empty(end, dtype=torch.uint8, device=d["dev"])
        part = {k: buf[lo:lo + size] for k, (lo, size) in at.items()}
        part["rows"].copy_(sel["rows"][:m].view(torch.uint8))
        part["first"].copy_(sel["first"].view(torch.uint8))
        part["span"].copy_(sel["span"][:m].reshape(-1).view(torch.uint8))
        p = _lib.dptr
        b = _lib.BlockStoreBatch(natt=d["natt"], rows=p(part["rows"]), span=p(part["span"]), bytes=p(d["d_bytes"]),
                                 key=p(part["key"]), hash=p(part["hash"]), lists=p(part["lists"]))
        cols = _lib.att_cols(d["att"], ("slot", "shard_id", "shard_block_hash", "shard_block_hash_offs", "oblique_parent_hashes",
                                        "oblique_offs", "oblique_first"))
        lib.call("pz_dev_block_store_digests", ctypes.byref(b), ctypes.byref(cols), m, run["q"]["sh"])
        host = buf.cpu().numpy()  # the store's own read
        get = lambda k, dt: host[at[k][0]:at[k][0] + at[k][1]].view(dt).copy()  # noqa: E731
        return {"rows": get("rows", np.uint32), "first": get("first", np.uint64), "span": get("span", np.uint64).reshape(m, 2),
                "key": get("key", np.uint8).reshape(m, 32), "hash": get("hash", np.uint8).reshape(m, 32), "lists": get("lists", np.uint8)}

    def _land(self, run, phase):
        """calculateBlockVoteCache and processedAttestations of one side of stateRecalc (``phase`` 0:
        the rows before it, 1: behind it), each behind its policy's room."""
        d, natt, log = run["d"], run["d"]["natt"], run["log"]
        self._cache_room.fit(run["oblique"][phase], 129 + run["record"][1], log)  # (the log entries the tallies read)
        self.cache.tally_columns(d["att"], natt, run["vote"][phase], d["committee"], d["parents_start"], log, self._members,
                                 self._table[3], self.state.balance)
        self._pool_room.fit(run["need"][phase])
        self.pool.append_columns(d["att"], natt, d["status"].contiguous(), d["committee"], take=run["take"][phase])

    def _land_run(self, run):
        """The landing of a read run whose gate did not panic: the rows before stateRecalc, with a
        transition block stateRecalc and the rows behind it, then the carry."""
        _, ncand, has, cslot, t_index, t_rank, t_slot, lag_out = run["record"]
        natt, log = run["d"]["natt"], run["log"]
        try:  # from here on the ring has rolled and the set has grown: an error leaves the objects ahead of the carry
            self._cache_room.begin()
            if natt:
                self._land(run, 0)
            chain_pair = self._chain
            if t_index != _NO_T:
                window = log[32 * (1 + t_rank):32 * (1 + t_rank + 128)]  # the promoted ActiveState's RecentBlockHashes
                pre = self._cand
                scal = _recalc_resident(self.pool, self.cache, self.state, window, 128, t_slot)["scalars"]
                self._cand = (int(scal[2]), int(scal[0]))
                chain_pair = pre  # what the chain keeps until T's states are promoted
                if natt:
                    self._land(run, 1)
        except BaseException:
            self.spent = True
            raise
        self.has_candidate, self.candidate_slot, self.lag = bool(has), cslot, lag_out
        self._chain = chain_pair if lag_out else None
        self._cache_room.end(ncand)

    def process_all(self, data, offsets, eligible=None, want_digests=False):
        """:meth:`process_serialized` from ``stop`` on until the bytes are used up: a list of its
        dicts in call order, each with ``start`` (the index of its first block in ``offsets``).  A
        submission holds at most ``RUN_BLOCKS`` blocks, so that a long chain is not uploaded and
        decoded whole once per cycle."""
        data = np.ascontiguousarray(_lib.as_u8(data), dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        outs, i = [], 0
        while i < n:
            hi = min(n, i + self.RUN_BLOCKS)
            out = self.process_serialized(data[int(offsets[i]):int(offsets[hi])], offsets[i:hi + 1] - offsets[i],
                                          None if eligible is None else eligible[i:hi], want_digests)
            if out["stop"] == 0:  # (a run of one block or more always takes its first)
                raise PzError(_lib.PZ_EINVAL, "the run at block %d took nothing" % i)
            out["start"] = i
            outs.append(out)
            i += out["stop"]
        return outs


def serialize_blocks(blocks):
    """pb.BeaconBlock list -> (uint8 data, uint64 offsets[n+1]) of canonical encodings."""
    enc = [wire.beacon_block(b) for b in blocks]
    offs = np.zeros(len(enc) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(e) for e in enc], dtype=np.uint64)
    return np.frombuffer(b"".join(enc) + bytes(16), dtype=np.uint8), offs


class BeaconChain:
    """A chain from the genesis states of ``nval`` validators on one GPU."""

    def __init__(self, nval, device=None, comm=None, msg_batch=0, tally_forms=0):
        """``comm`` (a ``prysm_amd.native.Comm``): one chain over the communicator's ranks,
        each holding a validator range of the balances, the vote cache and the epoch
        (pz_chain_new_comm).  ``msg_batch`` / ``tally_forms``:
        pz_chain_options (message batches sent during the walk; the tally's general forms
        forced, _lib.TALLY_*)."""
        idx = 0
        if device is not None:
            import torch
            d = torch.device(device)
            idx = d.index or 0
        self._h = ctypes.c_void_p()
        self.comm = comm  # kept alive as long as the chain
        if comm is not None:
            lib.call("pz_chain_new_comm", nval, comm.h, ctypes.byref(self._h))
        else:
            lib.call("pz_chain_new", nval, idx, ctypes.byref(self._h))
        self.nval = nval
        if msg_batch or tally_forms:
            opts = _lib.ChainOptions(int(msg_batch), int(tally_forms))
            lib.call("pz_chain_set_options", self._h, ctypes.byref(opts))

    @classmethod
    def from_state(cls, crystallized_bytes, saved_hashes=(), device=None):
        """NewBeaconChain with a stored CrystallizedState (blockchain/core.go:86-95): resume
        from its encoding with the genesis ActiveState; ``saved_hashes`` are the block hashes
        the database holds (hasBlock)."""
        idx = 0
        if device is not None:
            import torch
            idx = torch.device(device).index or 0
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        cs = np.frombuffer(bytes(crystallized_bytes), dtype=np.uint8)
        hs = np.frombuffer(b"".join(bytes(h) for h in saved_hashes), dtype=np.uint8)
        lib.call("pz_chain_new_from_state", _lib.ptr(cs), cs.size, _lib.ptr(hs), len(saved_hashes), idx,
                 ctypes.byref(self._h))
        self.nval = None
        return self

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.dll.pz_chain_free(h)
            self._h = None

    def process_serialized(self, data, offsets):
        """Run serialized blocks; returns (block results, attestation results) as numpy
        structured arrays (``BLOCK_RESULT`` / ``ATT_RESULT``)."""
        n = len(offsets) - 1
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        br = np.zeros(max(n, 1), dtype=BLOCK_RESULT)
        cnt = ctypes.c_uint64(0)
        lib.call("pz_count_attestations", _lib.ptr(data), _lib.ptr(offsets), n, ctypes.byref(cnt))
        natt_cap = max(1, cnt.value)
        ar = np.zeros(natt_cap, dtype=ATT_RESULT)
        try:
            lib.call("pz_chain_process_blocks", self._h, _lib.ptr(data), _lib.ptr(offsets), n,
                     br.ctypes.data, ar.ctypes.data, natt_cap)
        except PzError as e:
            if e.code == _lib.PZ_EINDEX:
                raise ChainPanic(str(e)) from None
            raise
        natt = int(br["natt"][:n].sum()) if n else 0
        return br[:n], ar[:natt]

    def process_blocks(self, blocks):
        """pb.BeaconBlock list -> per-block records (the oracle/replay.py record format)."""
        data, offs = serialize_blocks(blocks)
        br, ar = self.process_serialized(data, offs)
        recs = []
        for b, r in zip(blocks, br):
            rec = {"hash": r["hash"].tobytes(), "slot": b.slot_number, "atts": [],
                   "status": BLOCK_STATUS[int(r["status"])], "transition": bool(r["transition"])}
            for x in ar[int(r["first_att"]):int(r["first_att"]) + int(r["natt"])]:
                st = int(x["status"])
                if st == ATT_NOT_PROCESSED:
                    continue
                if st == ATT_PROCESSED:
                    rec["atts"].append({"key": x["key"].tobytes(), "hash": x["hash"].tobytes(),
                                        "msg": x["msg"].tobytes(), "msg_len": int(x["msg_len"])})
                else:
                    rec["atts"].append({"error": ATT_ERRORS.get(st, st)})
            recs.append(rec)
        return recs

    STATES = ("chain_active", "chain_crystallized", "cand_active", "cand_crystallized")

    def state_bytes(self, which):
        """The persisted proto3 encoding of a state (blockchain/core.go:161-177): ``which`` in
        ``STATES``; None for a candidate state when there is no candidate."""
        w = self.STATES.index(which)
        n = ctypes.c_uint64(0)
        try:
            lib.call("pz_chain_state_bytes", self._h, w, None, 0, ctypes.byref(n))
        except PzError as e:
            if w >= 2 and e.code == _lib.PZ_EINVAL:
                return None
            raise
        buf = np.zeros(max(n.value, 1), dtype=np.uint8)
        lib.call("pz_chain_state_bytes", self._h, w, buf.ctypes.data, n.value, ctypes.byref(n))
        return buf[:n.value].tobytes()

    def roots(self):
        """State roots (types/state.go:138-149, 237-248) of the chain's and the candidate's
        states, and the vote cache totals {hash: VoteTotalDeposit}."""
        out = (ctypes.c_uint8 * 128)()
        cand = ctypes.c_int(0)
        lib.call("pz_chain_roots", self._h, out, ctypes.byref(cand))
        raw = bytes(out)
        r = {"chain_active": raw[:32], "chain_crystallized": raw[32:64]}
        if cand.value:
            r["cand_active"], r["cand_crystallized"] = raw[64:96], raw[96:128]
        cnt = ctypes.c_uint64(0)
        lib.call("pz_chain_vote_totals", self._h, None, None, 0, ctypes.byref(cnt))
        n = cnt.value
        hashes = np.zeros(max(n, 1) * 32, dtype=np.uint8)
        totals = np.zeros(max(n, 1), dtype=np.uint64)
        if n:
            lib.call("pz_chain_vote_totals", self._h, hashes.ctypes.data, totals.ctypes.data, n, ctypes.byref(cnt))
        r["vote_totals"] = {hashes[32 * i:32 * i + 32].tobytes(): int(totals[i]) for i in range(n)}
        return r
