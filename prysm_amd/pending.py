"""ActiveState.PendingAttestations resident on one device -- Python face of ``pz_att_pool``
(prysm_amd/csrc/attpool.hip, include/prysm_hip.h).

The attestations a block contributes (processedAttestations, blockchain/service.go:280-301) become
pending attestations (computeNewActiveState, core.go:223-237) and feed the cycle transition
(core.go:433-457).  ``DevicePendingAttestations`` holds them as device columns: it is appended to
from the decoder's columns and the checks' outputs where they lie, pruned by slot, and read in
place -- as the epoch kernels' attestation inputs, as the columns ``pz_dev_wire_attestations``
encodes into the stored ActiveState's field 1, and as the crosslink winners' ShardBlockHash.
``RecalcState`` is the CrystallizedState side of ``blockchain.state_recalc_device``;
``ResidentRecalcState`` (``pz_recalc_state``, prysm_amd/csrc/recalc.hip) is the same state with its
scalars and crosslink records resident on the device, advanced by ``blockchain.state_recalc_resident``
in one ABI call.  ``DeviceRecentHashes`` (``pz_recent_hashes``, prysm_amd/csrc/blockwalk.hip) is
ActiveState.RecentBlockHashes resident on the device, rolled by ``blockchain.walk_serialized_blocks``.
"""
import numpy as np

from prysm_amd import _lib, pb, wire
from prysm_amd._lib import lib

CAPS = ("rows", "justified_block_hash", "shard_block_hash", "attester_bitfield", "oblique_elements", "oblique_bytes",
        "aggregate_sig")  # pz_att_pool_new's caps[7] / pz_att_pool_counts' counts[7]
_BYTES = ("justified_block_hash", "shard_block_hash", "attester_bitfield", "oblique_parent_hashes")


class _Raw:
    """A device address as something ``torch.as_tensor`` can wrap without a copy."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


class DeviceRecentHashes(_lib.Handle):
    """ActiveState.RecentBlockHashes resident on one device (``pz_recent_hashes``,
    prysm_amd/csrc/blockwalk.hip): 129 entries of 32 bytes with a stored length each, entry 0 one
    hash of history, entries 1..128 the window.  ``hashes``: the 128 of RecentBlockHashes (byte
    strings of at most 32 bytes, normalised here with their lengths kept, or a (128, 32) uint8 array
    with ``lens``); None: the genesis ring (types/state.go:45-49), 128 empty entries.  Any other
    count is refused (PZ_EINVAL): a shorter ring stays with the functions that take a list.

    Usable wherever ``recent_hashes`` is accepted next to a pool or a recalc state:
    ``blockchain.state_recalc_resident`` / ``state_recalc_device``,
    ``DevicePendingAttestations.active_state`` / ``active_state_root`` and
    ``blockchain.resident_state_roots``."""
    _FREE = "pz_recent_hashes_free"
    WINDOW = 128

    def __init__(self, hashes=None, lens=None, device=0):
        from prysm_amd.blockchain import _recent_array

        if hashes is None:
            rows, lens = np.zeros((self.WINDOW, 32), np.uint8), np.zeros(self.WINDOW, np.uint8)
        elif isinstance(hashes, np.ndarray):
            rows = _recent_array(hashes)
            lens = np.full(len(rows), 32, np.uint8) if lens is None else np.ascontiguousarray(lens, dtype=np.uint8)
        else:
            hashes = [bytes(h) for h in hashes]
            rows = _recent_array(hashes)
            lens = np.array([min(len(h), 32) for h in hashes], dtype=np.uint8) if lens is None else \
                np.ascontiguousarray(lens, dtype=np.uint8)
        assert lens.shape == (len(rows),)
        self._new("pz_recent_hashes_new", _lib.ptr(rows), _lib.ptr(lens), len(rows), device)
        self.device = device

    def view(self):
        """``(hashes (128, 32) uint8, lens (128) uint8)``: torch tensors over the live window where
        it lies (no copy), valid until the ring's next ``append`` or walk."""
        import torch

        h, n = _lib.ctypes.c_void_p(), _lib.ctypes.c_void_p()
        lib.call("pz_recent_hashes_view", self._h, _lib.ctypes.byref(h), _lib.ctypes.byref(n))
        dev = torch.device("cuda", self.device)
        return (torch.as_tensor(_Raw(h.value, 32 * self.WINDOW), device=dev).view(self.WINDOW, 32),
                torch.as_tensor(_Raw(n.value, self.WINDOW), device=dev))

    def read(self, history=False):
        """``(hashes (128, 32) uint8, lens (128) uint8)`` as numpy arrays (``pz_recent_hashes_read``;
        waits for the ring's last call); with ``history`` all 129 entries, the history entry first."""
        rows, lens = np.zeros((self.WINDOW + 1, 32), np.uint8), np.zeros(self.WINDOW + 1, np.uint8)
        lib.call("pz_recent_hashes_read", self._h, rows.ctypes.data, lens.ctypes.data)
        return (rows, lens) if history else (rows[1:], lens[1:])

    def hashes(self):
        """RecentBlockHashes as the stored byte strings (the last ``len`` bytes of each entry)."""
        rows, lens = self.read()
        return [rows[i, 32 - int(lens[i]):].tobytes() for i in range(self.WINDOW)]

    def append(self, d_hashes, take=None):
        """computeNewActiveState's append (core.go:230-237): the rows of ``d_hashes`` ((n, 32) uint8,
        a torch device tensor: on the current stream, asynchronous; or a numpy array / byte strings:
        synchronous) with ``take[j] != 0`` (None: all) go in, in order.  Once a hash went in every
        entry is stored with 32 bytes, as the reference stores RecentBlockHashes() back."""
        if hasattr(d_hashes, "data_ptr"):
            n = d_hashes.numel() // 32
            lib.call("pz_dev_recent_hashes_append", self._h, _lib.dptr(d_hashes), _lib.dptr(take), n,
                     _lib.stream_ptr(self.device))
            return
        from prysm_amd.blockchain import _recent_array

        rows = _recent_array(d_hashes)
        take = None if take is None else np.ascontiguousarray(take, dtype=np.uint8)
        lib.call("pz_recent_hashes_append", self._h, _lib.ptr(rows), _lib.ptr(take), len(rows))


class DeviceSavedBlocks(_lib.Handle):
    """The hashes of the blocks saveBlock stored (blockchain/service.go:324, core.go:565-577) resident on
    one device (``pz_block_set``, prysm_amd/csrc/blockparents.hip): what hasBlock (core.go:560-562)
    answers from, so that ``blockchain.walk_serialized_blocks_saved`` resolves the parent check of
    a whole run (service.go:261-269) on the device.  ``hashes``: the block hashes a stored DB holds
    (byte strings or an (n, 32) uint8 array; None: none -- a chain from genesis, whose first blocks
    have slot <= 1); ``min_keys``: room to start with (the set grows by itself, rehashing on the
    device)."""
    _FREE = "pz_block_set_free"
    _STICKY = (_lib.PZ_ERANGE,)

    def __init__(self, hashes=None, min_keys=1024, device=0):
        rows = self._rows(() if hashes is None else hashes)
        self._new("pz_block_set_new", _lib.ptr(rows), len(rows), int(min_keys), device)
        self.device = device
        self._count = None if len(rows) else 0  # the count as last read (None: not read yet)

    @staticmethod
    def _rows(hashes):
        if isinstance(hashes, np.ndarray):
            return np.ascontiguousarray(hashes, dtype=np.uint8).reshape(-1, 32)
        hashes = [bytes(h) for h in hashes]
        assert all(len(h) == 32 for h in hashes), "a block hash is 32 bytes"
        return np.frombuffer(b"".join(hashes), dtype=np.uint8).reshape(-1, 32)

    def count(self, strict=True):
        """The number of distinct hashes (``pz_block_set_count``; waits for the set's last call)."""
        n = _lib.ctypes.c_uint64(0)
        self._rc(lib.dll.pz_block_set_count(self._h, _lib.ctypes.byref(n)), strict)
        self._count = int(n.value)
        return self._count

    __len__ = count

    def hashes(self, strict=True):
        """Every stored hash as a byte string, in no particular order (``pz_block_set_read``)."""
        cap = self.count(strict)
        out = np.zeros((max(cap, 1), 32), dtype=np.uint8)
        n = _lib.ctypes.c_uint64(0)
        self._rc(lib.dll.pz_block_set_read(self._h, out.ctypes.data, cap, _lib.ctypes.byref(n)), strict)
        return [out[i].tobytes() for i in range(int(n.value))]

    def contains(self, hashes):
        """hasBlock (core.go:560-562) per hash: a uint8 torch tensor for an (n, 32) uint8 device tensor
        (current stream, asynchronous), else a numpy bool array (synchronous)."""
        if hasattr(hashes, "data_ptr"):
            import torch

            n = hashes.numel() // 32
            out = torch.empty(n, dtype=torch.uint8, device=hashes.device)
            lib.call("pz_dev_block_set_contains", self._h, _lib.dptr(hashes), n, _lib.dptr(out), _lib.stream_ptr(self.device))
            return out
        rows = self._rows(hashes)
        out = np.zeros(len(rows), dtype=np.uint8)
        lib.call("pz_block_set_contains", self._h, _lib.ptr(rows), len(rows), _lib.ptr(out))
        return out.astype(bool)

    def reserve(self, min_keys, device_form=False):
        """Room for ``min_keys`` hashes: when they need more cells every key is rehashed on the device
        (``pz_[dev_]block_set_reserve``; ``device_form``: on the current stream, asynchronous)."""
        if device_form:
            lib.call("pz_dev_block_set_reserve", self._h, int(min_keys), _lib.stream_ptr(self.device))
        else:
            lib.call("pz_block_set_reserve", self._h, int(min_keys))

    def insert(self, hashes, take=None):
        """saveBlock's key (core.go:565-577) for the caller that decides for itself -- the transition
        block's path: the rows with ``take[j] != 0`` (None: all) become keys, duplicates once.  An
        (n, 32) uint8 device tensor goes in on the current stream, asynchronously, after a reserve from
        the count last read; a numpy array or byte strings synchronously."""
        if hasattr(hashes, "data_ptr"):
            n = hashes.numel() // 32
            self.reserve((self.count() if self._count is None else self._count) + n, device_form=True)
            lib.call("pz_dev_block_set_insert", self._h, _lib.dptr(hashes), _lib.dptr(take), n, _lib.stream_ptr(self.device))
            self._count = None
            return
        rows = self._rows(hashes)
        take = None if take is None else np.ascontiguousarray(take, dtype=np.uint8)
        lib.call("pz_block_set_insert", self._h, _lib.ptr(rows), _lib.ptr(take), len(rows))
        self._count = None


def recent_of(recent, recent_len=None):
    """``(rows, lens)`` on the host of what a ``recent_hashes`` argument names: a
    ``DeviceRecentHashes`` is downloaded with its stored lengths, anything else passes through."""
    if isinstance(recent, DeviceRecentHashes):
        return recent.read()
    return recent, recent_len


class DevicePendingAttestations(_lib.Handle):
    """``caps``: the seven capacities (``CAPS``' order) the pool starts with; :meth:`reserve` raises
    them on the device, as append grows the reference's slice (core.go:223-237), and ``self.caps``
    stays the current ones.  A call that would exceed one changes nothing (PZ_ERANGE, sticky) --
    :meth:`need_columns` tells beforehand what an append would add; a kept row with an inverted
    range lands empty (PZ_EINVAL, sticky).  Every read raises the sticky error; ``strict=False``
    returns what the pool holds regardless."""
    _FREE = "pz_att_pool_free"
    _STICKY = (_lib.PZ_EINVAL, _lib.PZ_ERANGE)

    def __init__(self, caps, device=0):
        self.caps = np.ascontiguousarray(caps, dtype=np.uint64)
        assert self.caps.shape == (7,)
        self._new("pz_att_pool_new", self.caps.ctypes.data, device)
        self.device = device

    def _stream(self):
        return _lib.stream_ptr(self.device)

    # ---- writes ------------------------------------------------------------------------------
    def append_columns(self, cols, n, status, committee, take=None):
        """Appends the rows of ``cols`` (torch device tensors keyed as ``wire.ATT_COLS``, e.g. from
        ``wire.unwire_attestations_device``; a missing or None column follows pz_attestation_cols'
        NULL rules) whose ``status`` (int32) is PZ_ATT_PROCESSED and whose ``take`` (uint8,
        optional) is not 0; ``committee`` (int32): the checks' committee ids.  On the current
        stream, asynchronous (``pz_dev_att_pool_append``)."""
        import torch

        c = _lib.att_cols(cols)
        scratch = torch.empty(max(int(lib.dll.pz_att_pool_scratch_bytes(n)), 16), dtype=torch.uint8, device=status.device)
        p = _lib.dptr
        lib.call("pz_dev_att_pool_append", self._h, _lib.ctypes.byref(c), n, p(status), p(committee), p(take),
                 scratch.data_ptr(), self._stream())

    def append_host(self, cols, n, status, committee, take=None):
        """The same append over host arrays (numpy; ``pz_att_pool_append``, synchronous)."""
        c = _lib.att_cols(cols)
        status = np.ascontiguousarray(status, dtype=np.int32)
        committee = np.ascontiguousarray(committee, dtype=np.uint32)
        take = None if take is None else np.ascontiguousarray(take, dtype=np.uint8)
        lib.call("pz_att_pool_append", self._h, _lib.ctypes.byref(c), n, _lib.ptr(status), _lib.ptr(committee),
                 _lib.ptr(take))

    def prune(self, last_state_recalc):
        """stateRecalc's filter (core.go:444-450): keeps the rows with ``slot > last_state_recalc``.
        On the current stream, asynchronous."""
        lib.call("pz_dev_att_pool_prune", self._h, int(last_state_recalc), self._stream())

    def reserve(self, min_caps, device_form=False):
        """append's own growth of the list (core.go:223-237): the capacities become
        ``max(caps, min_caps)`` column by column, exactly; where none rises nothing is launched.  One
        launch moves the live rows, whose counts the host does not read; counts, rows, contents and
        the sticky error are unchanged (``pz_[dev_]att_pool_reserve``; ``device_form``: on the
        current stream, asynchronous).  Addresses from :meth:`view` taken before it stay readable by
        what is already queued but are no longer the pool."""
        min_caps = np.ascontiguousarray(min_caps, dtype=np.uint64)
        assert min_caps.shape == (7,)
        if device_form:
            lib.call("pz_dev_att_pool_reserve", self._h, min_caps.ctypes.data, self._stream())
        else:
            lib.call("pz_att_pool_reserve", self._h, min_caps.ctypes.data)
        self.caps = self.capacity()

    def capacity(self):
        """The seven capacities now (``CAPS``' order) as a uint64 array (``pz_att_pool_capacity``;
        the host's own record, no device call)."""
        out = np.zeros(7, dtype=np.uint64)
        lib.call("pz_att_pool_capacity", self._h, out.ctypes.data)
        return out

    @staticmethod
    def need_columns(cols, n, status, take0=None, take1=None):
        """What :meth:`append_columns` of these rows would add to the seven counts, for ``take0`` and
        for ``take1`` (None: every PROCESSED row): a (2, 7) int64 device tensor, left on the device.
        The append's size and scan launches without a commit, on the current stream, asynchronous
        (``pz_dev_att_pool_need``)."""
        import torch

        c = _lib.att_cols(cols)
        dev = status.device
        need = torch.empty((2, 7), dtype=torch.int64, device=dev)
        scratch = torch.empty(max(int(lib.dll.pz_att_pool_need_scratch_bytes(n)), 16), dtype=torch.uint8, device=dev)
        p = _lib.dptr
        lib.call("pz_dev_att_pool_need", _lib.ctypes.byref(c), n, p(status), p(take0), p(take1), need.data_ptr(),
                 scratch.data_ptr(), _lib.stream_ptr(dev))
        return need

    @staticmethod
    def need_host(cols, n, status, take0=None, take1=None):
        """The same sums over host arrays, a (2, 7) uint64 array (``pz_att_pool_need``, synchronous)."""
        c = _lib.att_cols(cols)
        status = np.ascontiguousarray(status, dtype=np.int32)
        take0 = None if take0 is None else np.ascontiguousarray(take0, dtype=np.uint8)
        take1 = None if take1 is None else np.ascontiguousarray(take1, dtype=np.uint8)
        need = np.zeros((2, 7), dtype=np.uint64)
        lib.call("pz_att_pool_need", _lib.ctypes.byref(c), n, _lib.ptr(status), _lib.ptr(take0), _lib.ptr(take1),
                 need.ctypes.data)
        return need

    # ---- reads -------------------------------------------------------------------------------
    def counts(self, strict=True):
        """The seven counts (``CAPS``' order) as a uint64 array; waits for the last call."""
        out = np.zeros(7, dtype=np.uint64)
        self._rc(lib.dll.pz_att_pool_counts(self._h, out.ctypes.data), strict)
        return out

    def __len__(self):
        return int(self.counts(strict=False)[0])

    def view(self):
        """``(AttestationCols, committee, shard32)``: device addresses into the live buffer set,
        valid until the next prune or reserve."""
        c = _lib.AttestationCols()
        comm, s32 = _lib.ctypes.c_void_p(), _lib.ctypes.c_void_p()
        lib.call("pz_att_pool_view", self._h, _lib.ctypes.byref(c), _lib.ctypes.byref(comm), _lib.ctypes.byref(s32))
        return c, comm.value, s32.value

    def raw_columns(self):
        """The live buffer set's bytes columns and ``aggregate_sig`` at their full capacities, as
        uint8 torch tensors over the pool's own memory (no copy; tests write canaries through them)."""
        import torch

        c, _, _ = self.view()
        cap = dict(zip(CAPS, (int(x) for x in self.caps)))
        size = {"justified_block_hash": cap["justified_block_hash"], "shard_block_hash": cap["shard_block_hash"],
                "attester_bitfield": cap["attester_bitfield"], "oblique_parent_hashes": cap["oblique_bytes"],
                "aggregate_sig": 8 * cap["aggregate_sig"]}
        dev = torch.device("cuda", self.device)
        return {k: torch.as_tensor(_Raw(getattr(c, k), nb), device=dev) for k, nb in size.items() if nb}

    def shard32(self):
        """The ``shard32`` column (ShardId saturated to UINT32_MAX: the epoch kernels' ``att_shard``)
        as a uint32 array."""
        import torch

        rows = len(self)
        if not rows:
            return np.zeros(0, dtype=np.uint32)
        _, _, s32 = self.view()
        t = torch.as_tensor(_Raw(s32, 4 * rows), device=torch.device("cuda", self.device))
        return t.cpu().numpy().view(np.uint32)

    def columns(self, strict=True):
        """Everything the pool holds as numpy arrays keyed as ``wire.ATT_COLS``, plus ``committee``
        (``pz_att_pool_read``)."""
        n = self.counts(strict=False)
        rows = int(n[0])
        size = wire.att_sizes(rows, n[1:])
        cols = {k: np.zeros(max(size[k], 1), dtype=np.uint8 if k in _BYTES else np.uint64) for k in wire.ATT_COLS}
        committee = np.zeros(max(rows, 1), dtype=np.uint32)
        out = _lib.AttestationColsOut(*[cols[k].ctypes.data for k in wire.ATT_COLS], None, None, None)
        caps = np.ascontiguousarray(n[1:])
        self._rc(lib.dll.pz_att_pool_read(self._h, _lib.ctypes.byref(out), committee.ctypes.data, caps.ctypes.data), strict)
        res = {k: v[:size[k]] for k, v in cols.items()}
        res["committee"] = committee[:rows]
        return res

    def records(self, strict=True):
        """PendingAttestations() as ``pb.AttestationRecord``s, in order."""
        c = self.columns(strict)
        span = lambda k, i: c[k][int(c[k + "_offs"][i]):int(c[k + "_offs"][i + 1])].tobytes()  # noqa: E731
        oo, data = c["oblique_offs"], c["oblique_parent_hashes"]
        out = []
        for i in range(len(c["slot"])):
            e0, e1 = int(c["oblique_first"][i]), int(c["oblique_first"][i + 1])
            s0, s1 = int(c["aggregate_sig_first"][i]), int(c["aggregate_sig_first"][i + 1])
            out.append(pb.AttestationRecord(
                slot=int(c["slot"][i]), shard_id=int(c["shard_id"][i]), justified_slot=int(c["justified_slot"][i]),
                justified_block_hash=span("justified_block_hash", i), shard_block_hash=span("shard_block_hash", i),
                attester_bitfield=span("attester_bitfield", i),
                oblique_parent_hashes=[data[int(oo[e]):int(oo[e + 1])].tobytes() for e in range(e0, e1)],
                aggregate_sig=[int(x) for x in c["aggregate_sig"][s0:s1]]))
        return out

    def wire(self, field_num=1):
        """The pool's view encoded where it lies by ``pz_dev_wire_attestations`` on the current
        stream: with ``field_num=1`` the leading bytes of the stored ActiveState
        (types/state.go:141).  Returns ``(bytes, offsets[n+1] uint64)``."""
        import torch

        rows, jb, sb, bf, ne, eb, ns = (int(x) for x in self.counts())
        if not rows:
            return b"", np.zeros(1, dtype=np.uint64)
        dev = torch.device("cuda", self.device)
        c, _, _ = self.view()
        out = torch.empty(max(int(lib.dll.pz_wire_attestations_bound(rows, jb + sb + bf + eb, ne, ns)), 1),
                          dtype=torch.uint8, device=dev)
        offs = torch.empty(rows + 1, dtype=torch.int64, device=dev)
        scr = torch.empty(max(int(lib.dll.pz_wire_attestations_scratch_bytes(rows)), 16), dtype=torch.uint8, device=dev)
        lib.call("pz_dev_wire_attestations", _lib.ctypes.byref(c), rows, field_num, out.data_ptr(), offs.data_ptr(),
                 scr.data_ptr(), self._stream())
        offs = offs.cpu().numpy().view(np.uint64)
        return out[:int(offs[-1])].cpu().numpy().tobytes(), offs

    def _stored(self, recent, recent_len, want_root, strict):
        from prysm_amd.blockchain import _recent_array

        recent, recent_len = recent_of(recent, recent_len)
        rows = _recent_array(recent)
        n = len(rows)
        lens = None if recent_len is None else np.ascontiguousarray(recent_len, dtype=np.uint8)
        assert lens is None or lens.shape == (n,)
        counts = self.counts(strict=False)
        cap = int(lib.dll.pz_active_state_bound(counts.ctypes.data, n))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        length = _lib.ctypes.c_uint64(0)
        root = np.zeros(32, dtype=np.uint8)
        rc = lib.dll.pz_active_state_read(self._h, _lib.ptr(rows), _lib.ptr(lens), n, out.ctypes.data, cap,
                                          _lib.ctypes.byref(length), root.ctypes.data if want_root else None)
        self._rc(rc, strict)
        return out[:length.value].tobytes(), root.tobytes()

    def active_state(self, recent, recent_len=None, strict=True):
        """The stored ActiveState (PersistActiveState, blockchain/core.go:161-168) encoded on the
        device: the pool as field 1, then ``recent`` = RecentBlockHashes() (byte strings, normalised
        here, or a (k, 32) uint8 array) as field 2, entry i being the last ``recent_len[i]`` bytes of
        its row (None: all 32; the genesis state's entries are empty: all 0).  A
        ``DeviceRecentHashes`` stands for both: its window and its stored lengths.
        ``pz_active_state_read``."""
        return self._stored(recent, recent_len, False, strict)[0]

    def active_state_root(self, recent, recent_len=None, strict=True):
        """ActiveState.Hash() (types/state.go:138-149) of :meth:`active_state`'s message, 32 bytes."""
        return self._stored(recent, recent_len, True, strict)[1]

    def shard_block_hashes(self, rows):
        """ShardBlockHash of the named rows, a list of byte strings: what a crosslink winner writes
        into its record (core.go:550-554)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        offs = np.zeros(len(rows) + 1, dtype=np.uint64)
        out = np.zeros(1, dtype=np.uint8)
        rc = lib.dll.pz_att_pool_shard_block_hashes(self._h, _lib.ptr(rows), len(rows), None, 0, offs.ctypes.data)
        if rc == _lib.PZ_ERANGE:  # (offs is filled: the size to come back with)
            out = np.zeros(int(offs[-1]), dtype=np.uint8)
            rc = lib.dll.pz_att_pool_shard_block_hashes(self._h, _lib.ptr(rows), len(rows), out.ctypes.data, out.size,
                                                        offs.ctypes.data)
        self._rc(rc, True)
        return [out[int(offs[k]):int(offs[k + 1])].tobytes() for k in range(len(rows))]

    def epoch_batch(self, batch=None):
        """Fills the attestation side of an ``_lib.EpochBatch`` (``natt``, ``bits``, ``boffs``,
        ``max_inst_bytes``, ``att_comm``, ``att_shard``) from the view and the counts, for
        ``ninst = 1``; the caller fills the validators, committees, records and outputs (``vote`` and
        ``total`` hold ``natt`` entries).  Returns the batch."""
        b = _lib.EpochBatch() if batch is None else batch
        n = self.counts()
        c, comm, s32 = self.view()
        b.ninst = 1
        b.natt = int(n[0])
        b.bits, b.boffs = c.attester_bitfield, c.attester_bitfield_offs
        b.max_inst_bytes = int(n[3])
        b.att_comm, b.att_shard = comm, s32
        return b


class _DeviceValidators:
    """What both recalc states put on the device: ``balance``, ``start`` and ``end`` as int64
    tensors and the committees as a CSR (``members`` int32, ``coffs`` int64)."""

    def _put_validators(self, balance, start_dynasty, end_dynasty, members, coffs, device):
        import torch

        from prysm_amd.blockchain import _to_device

        dev = torch.device("cuda", device)
        u64 = lambda a: _to_device(np.ascontiguousarray(a, dtype=np.uint64), dev)  # noqa: E731
        self.device = device
        self.balance, self.start, self.end = u64(balance), u64(start_dynasty), u64(end_dynasty)
        members = np.ascontiguousarray(members, dtype=np.uint32)
        self.members = _to_device(members if members.size else np.zeros(1, np.uint32), dev)
        self.coffs = u64(coffs)

    @property
    def nval(self):
        return int(self.balance.numel())

    def balances(self):
        return self.balance.cpu().numpy().view(np.uint64)


class RecalcState(_DeviceValidators):
    """The CrystallizedState ``blockchain.state_recalc_device`` advances: ``balance``, ``start`` and
    ``end`` (the validators' Balance / StartDynasty / EndDynasty) as int64 device tensors, the
    committees as a device CSR (``members`` int32, ``coffs`` int64), the host scalars and the
    crosslink records (``pb.CrosslinkRecord``)."""

    def __init__(self, balance, start_dynasty, end_dynasty, members, coffs, crosslink_records, *, last_state_recalc=0,
                 justified_streak=0, last_justified_slot=0, last_finalized_slot=0, current_dynasty=1, total_deposits=0,
                 device=0):
        self._put_validators(balance, start_dynasty, end_dynasty, members, coffs, device)
        self.crosslink_records = [pb.CrosslinkRecord(r.dynasty, bytes(r.blockhash), r.slot) for r in crosslink_records]
        self.last_state_recalc, self.justified_streak = int(last_state_recalc), int(justified_streak)
        self.last_justified_slot, self.last_finalized_slot = int(last_justified_slot), int(last_finalized_slot)
        self.current_dynasty, self.total_deposits = int(current_dynasty), int(total_deposits)


class ResidentRecalcState(_DeviceValidators, _lib.Handle):
    """The CrystallizedState ``blockchain.state_recalc_resident`` advances, resident on one device
    (``pz_recalc_state``, prysm_amd/csrc/recalc.hip): ``RecalcState``'s constructor arguments plus
    ``hash_stride`` (the bytes a crosslink record's hash may take, a multiple of 16 in [32, 256]).
    The validators and the committee CSR are device tensors as in ``RecalcState``; the scalars and
    the crosslink records live in the handle and come back through ``read()``.  A panic of the
    reference (PZ_EINDEX) is sticky and raised by every read; ``strict=False`` returns what the
    handle holds -- the state before the panicking call -- regardless."""

    _FREE = "pz_recalc_state_free"
    _STICKY = (_lib.PZ_EINDEX,)
    _SCALARS = ("last_state_recalc", "justified_streak", "last_justified_slot", "last_finalized_slot", "current_dynasty",
                "total_deposits")

    def __init__(self, balance, start_dynasty, end_dynasty, members, coffs, crosslink_records, *, last_state_recalc=0,
                 justified_streak=0, last_justified_slot=0, last_finalized_slot=0, current_dynasty=1, total_deposits=0,
                 device=0, hash_stride=32):
        self._put_validators(balance, start_dynasty, end_dynasty, members, coffs, device)
        self.hash_stride = int(hash_stride)
        recs = list(crosslink_records)
        self.nrec = len(recs)
        scalars = np.zeros(_lib.RS_COUNT, dtype=np.uint64)
        scalars[:6] = [int(last_state_recalc), int(justified_streak), int(last_justified_slot), int(last_finalized_slot),
                       int(current_dynasty), int(total_deposits)]
        dyn = np.array([r.dynasty for r in recs], dtype=np.uint64)
        slot = np.array([r.slot for r in recs], dtype=np.uint64)
        offs = np.zeros(self.nrec + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(r.blockhash) for r in recs], dtype=np.uint64)
        data = np.frombuffer(b"".join(bytes(r.blockhash) for r in recs), dtype=np.uint8)
        self._new("pz_recalc_state_new", self.nrec, self.hash_stride, scalars.ctypes.data, _lib.ptr(dyn), _lib.ptr(slot),
                  _lib.ptr(data), offs.ctypes.data, device)

    @classmethod
    def from_state(cls, crystallized_bytes, device=0, hash_stride=32):
        """NewBeaconChain's reload (blockchain/core.go:86-95) for the resident path: the state a
        stored CrystallizedState's bytes hold, decoded on the device
        (``wire.unwire_crystallized_state_device``: one upload, the head on the host, frame, the read
        of its sizes, exact-size tensors, decode).  Beside ``balance / start / end / members / coffs``
        the object carries the other ValidatorRecord columns (``public_key``, ``withdrawal_shard``,
        ``withdrawal_address`` and ``randao_commitment`` with their ``_offs``), which
        :meth:`validator_cols` passes on; ``rest`` (the keyword arguments of :meth:`wire` the handle
        does not hold); ``table`` (``_committee_table``'s four arrays as device tensors) with
        ``narr``; and ``field12``, the received span, which :meth:`wire` / :meth:`root` take as it is.
        Exactly the canonical encoding is accepted (``PzError`` with ``.offset`` otherwise)."""
        d = wire.unwire_crystallized_state_device(crystallized_bytes, device)
        head = d["head"]
        self = cls.__new__(cls)
        self.device = device
        self.balance, self.start, self.end = d["balance"], d["start_dynasty"], d["end_dynasty"]
        self.members = d["members"] if d["members"].numel() else d["members"].new_zeros(1)
        self.coffs = d["coffs"]
        self.public_key, self.withdrawal_shard = d["public_key"], d["withdrawal_shard"]
        self.withdrawal_address, self.withdrawal_address_offs = d["withdrawal_address"], d["withdrawal_address_offs"]
        self.randao_commitment, self.randao_commitment_offs = d["randao_commitment"], d["randao_commitment_offs"]
        self._val_bytes = int(d["withdrawal_address"].numel()) + int(d["randao_commitment"].numel())
        self.table, self.narr = [d[k] for k in ("arr_offs", "arr_shard", "arr_comm", "coffs")], d["narr"]
        self.field12 = d["field12"]
        r = head["rest"]
        self.rest = dict(crosslinking_start_shard=int(r.crosslinking_start_shard),
                         dynasty_seed=bytes(r.dynasty_seed)[:r.dynasty_seed_len],
                         dynasty_seed_last_reset=int(r.dynasty_seed_last_reset))
        self.hash_stride, self.nrec = int(hash_stride), len(head["rec_dynasty"])
        self._new("pz_recalc_state_new", self.nrec, self.hash_stride, head["scalars"].ctypes.data, _lib.ptr(head["rec_dynasty"]),
                  _lib.ptr(head["rec_slot"]), _lib.ptr(head["rec_hash"]), head["rec_hash_offs"].ctypes.data, device)
        return self

    def read(self, strict=True):
        """``{"scalars": uint64[8], "rec_dynasty", "rec_slot", "rec_hash" (nrec, hash_stride) uint8,
        "rec_hash_len", "winner"}`` (``pz_recalc_state_read``; waits for the last call)."""
        n = max(self.nrec, 1)
        out = {"scalars": np.zeros(_lib.RS_COUNT, np.uint64), "rec_dynasty": np.zeros(n, np.uint64),
               "rec_slot": np.zeros(n, np.uint64), "rec_hash": np.zeros((n, self.hash_stride), np.uint8),
               "rec_hash_len": np.zeros(n, np.uint32), "winner": np.full(n, 0xFFFFFFFF, np.uint32)}
        rc = lib.dll.pz_recalc_state_read(self._h, *[out[k].ctypes.data for k in
                                                     ("scalars", "rec_dynasty", "rec_slot", "rec_hash", "rec_hash_len", "winner")])
        self._rc(rc, strict)
        return {k: (v if k == "scalars" else v[:self.nrec]) for k, v in out.items()}

    def scalar(self, index, strict=True):
        return int(self.read(strict)["scalars"][index])

    @property
    def crosslink_records(self):
        r = self.read(strict=False)
        return [pb.CrosslinkRecord(int(r["rec_dynasty"][i]), r["rec_hash"][i, :int(r["rec_hash_len"][i])].tobytes(),
                                   int(r["rec_slot"][i])) for i in range(self.nrec)]

    def winners(self, strict=True):
        """The last call's winners: one pool row (before the prune) per record, 0xFFFFFFFF: none."""
        return self.read(strict)["winner"]

    def _field12(self, field12):
        """Field 12 as a uint8 device tensor: bytes are uploaded; the ``(out, result)`` pair of
        ``wire.committees_device`` is cut at its length (a table error raises)."""
        import torch

        dev = self.balance.device
        if isinstance(field12, tuple):
            out, result = field12
            length, status = (int(x) for x in result.cpu())
            if status != _lib.PZ_OK:
                raise _lib.PzError(status, "the committee table was refused")
            return out[:length]
        if hasattr(field12, "data_ptr"):
            return field12
        raw = np.frombuffer(bytes(field12), dtype=np.uint8)
        return torch.from_numpy(raw.copy()).to(dev) if raw.size else torch.empty(0, dtype=torch.uint8, device=dev)

    def validator_cols(self):
        """``pz_validator_cols`` over the resident balance / start / end; the other fields are the
        columns a state loaded by :meth:`from_state` carries, and zero without them."""
        cols = _lib.ValidatorCols(balance=self.balance.data_ptr(), start_dynasty=self.start.data_ptr(),
                                  end_dynasty=self.end.data_ptr())
        if hasattr(self, "public_key"):
            p = _lib.dptr
            cols.public_key, cols.withdrawal_shard = p(self.public_key), p(self.withdrawal_shard)
            if self.withdrawal_address.numel():
                cols.withdrawal_address, cols.withdrawal_address_offs = p(self.withdrawal_address), p(self.withdrawal_address_offs)
            if self.randao_commitment.numel():
                cols.randao_commitment, cols.randao_commitment_offs = p(self.randao_commitment), p(self.randao_commitment_offs)
        return cols

    def _stored(self, field12, crosslinking_start_shard, dynasty_seed, dynasty_seed_last_reset, want_root, strict):
        f12 = self._field12(field12)
        seed = bytes(dynasty_seed)
        rest = _lib.CstateRest(crosslinking_start_shard=int(crosslinking_start_shard), dynasty_seed_len=len(seed),
                               dynasty_seed_last_reset=int(dynasty_seed_last_reset))
        if len(seed) <= 64:
            _lib.ctypes.memmove(rest.dynasty_seed, seed, len(seed))
        cols = self.validator_cols()
        cap = int(lib.dll.pz_crystallized_state_bound(self.nrec, self.hash_stride, self.nval, getattr(self, "_val_bytes", 0),
                                                      int(f12.numel())))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        length = _lib.ctypes.c_uint64(0)
        root = np.zeros(32, dtype=np.uint8)
        rc = lib.dll.pz_crystallized_state_read(self._h, _lib.ctypes.byref(rest), _lib.ctypes.byref(cols), self.nval,
                                                _lib.dptr(f12), int(f12.numel()), out.ctypes.data, cap,
                                                _lib.ctypes.byref(length), root.ctypes.data if want_root else None)
        self._rc(rc, strict)
        return out[:length.value].tobytes(), root.tobytes()

    def wire(self, field12, crosslinking_start_shard=0, dynasty_seed=b"", dynasty_seed_last_reset=0, strict=True):
        """The stored CrystallizedState (PersistCrystallizedState, blockchain/core.go:170-177) encoded
        on the device from the handle, the resident validators and ``field12`` -- the already encoded
        ShardAndCommitteesForSlots: bytes, a uint8 device tensor, or what ``wire.committees_device``
        returns for device columns (``pz_crystallized_state_read``).  The remaining arguments are the
        fields the handle does not hold."""
        return self._stored(field12, crosslinking_start_shard, dynasty_seed, dynasty_seed_last_reset, False, strict)[0]

    def root(self, field12, crosslinking_start_shard=0, dynasty_seed=b"", dynasty_seed_last_reset=0, strict=True):
        """CrystallizedState.Hash() (types/state.go:237-248) of :meth:`wire`'s message, 32 bytes."""
        return self._stored(field12, crosslinking_start_shard, dynasty_seed, dynasty_seed_last_reset, True, strict)[1]


for _i, _name in enumerate(ResidentRecalcState._SCALARS):
    setattr(ResidentRecalcState, _name, property(lambda self, _i=_i: self.scalar(_i, strict=False)))


__all__ = ["DevicePendingAttestations", "DeviceRecentHashes", "DeviceSavedBlocks", "RecalcState", "ResidentRecalcState", "CAPS"]
