"""Host-side mirror of the block vote cache (types/state.go:27-31 ``VoteCache`` and
blockchain/core.go:300-345 ``calculateBlockVoteCache``) over the GPU tally kernel.

The Go map ``map[[32]byte]*VoteCache`` becomes a host dict ``hash -> slot`` plus, per slot,
an nval-bit voter bitmap and the ``VoteTotalDeposit`` u64.  ``VoterIndices`` is a set here
(the bitmap; ascending order on read-out) — the reference's insertion order is never
serialized or hashed.
"""
import numpy as np

from prysm_amd import _lib
from prysm_amd._lib import lib, ptr


class VoteCache:
    def __init__(self, nval):
        self.nval = nval
        self.words = (nval + 31) // 32
        self.slot_of = {}
        self.bitmaps = np.zeros((0, self.words), dtype=np.uint32)
        self.totals = np.zeros(0, dtype=np.uint64)

    def slot(self, h):
        """Slot of hash ``h``, created empty if absent (core.go:321-324)."""
        s = self.slot_of.get(h)
        if s is None:
            s = len(self.slot_of)
            self.slot_of[h] = s
            if s >= self.totals.shape[0]:
                cap = max(16, 2 * s)
                bm = np.zeros((cap, self.words), dtype=np.uint32)
                bm[:self.bitmaps.shape[0]] = self.bitmaps
                tt = np.zeros(cap, dtype=np.uint64)
                tt[:self.totals.shape[0]] = self.totals
                self.bitmaps, self.totals = bm, tt
        return s

    def __contains__(self, h):
        return h in self.slot_of

    def total(self, h):
        s = self.slot_of.get(h)
        return 0 if s is None else int(self.totals[s])

    def voters(self, h):
        s = self.slot_of[h]
        bits = np.unpackbits(self.bitmaps[s].view(np.uint8), bitorder="little")[:self.nval]
        return np.nonzero(bits)[0].astype(np.uint32)

    def tally(self, committee, coffs, att_comm, bits, boffs, items, balance, comm=None):
        """Apply work items [(attestation index, slot)] in one GPU launch; with ``comm`` (a
        ``prysm_amd.native.Comm``) sharded by validator range over its ranks, the per-slot
        totals combined by one all-reduce (pz_comm_vote_tally)."""
        if not items:
            return
        ia = np.ascontiguousarray([a for a, _ in items], dtype=np.uint32)
        isl = np.ascontiguousarray([s for _, s in items], dtype=np.uint32)
        bm = np.ascontiguousarray(self.bitmaps)
        tt = np.ascontiguousarray(self.totals)
        args = (ptr(committee), ptr(coffs), len(coffs) - 1, ptr(att_comm), ptr(bits), ptr(boffs),
                len(att_comm), ptr(ia), ptr(isl), len(items), ptr(np.ascontiguousarray(balance, dtype=np.uint64)),
                self.nval, ptr(bm), bm.shape[0], self.words, ptr(tt))
        if comm is None:
            lib.call("pz_vote_tally", *args)
        else:
            lib.call("pz_comm_vote_tally", comm.h, *args)
        self.bitmaps, self.totals = bm, tt


_COL_KEYS = ("oblique_parent_hashes", "oblique_offs", "oblique_first")


class DeviceVoteCache(_lib.Handle):
    """The block vote cache resident on one device (``pz_vote_cache``, prysm_amd/csrc/votecache.hip):
    the map from hash to slot lives there too, so a tally takes the decoder's columns
    (``wire.ATT_COLS`` keys) and the checks' outputs as they are -- no work list, no host hash map.

    Scope, as the header states it: a tally covers the rows whose ``status`` is PZ_ATT_PROCESSED
    (and ``take[i] != 0`` when ``take`` is given).  The reference also tallies the failed
    attestations of a block whose last attestation passed; which rows those are is the block
    gate's decision (``blockchain.gate_blocks``: its ``vote_status`` goes in as ``status``), and
    ``blockchain.tally_serialized_blocks`` reports such blocks and, with ``tally_mixed``, tallies
    them that way.

    The read side is ``VoteCache``'s: ``items()``, ``voters(h)``, ``total(h)``, ``h in cache``.  A
    panic of the reference (PZ_EINDEX) or a call dropped for capacity (PZ_ERANGE) is sticky and
    raised by every read; ``strict=False`` returns what the cache holds regardless."""
    _FREE = "pz_vote_cache_free"
    _STICKY = (_lib.PZ_EINDEX, _lib.PZ_ERANGE)

    def __init__(self, nval, slot_cap, device=0):
        self._new("pz_vote_cache_new", nval, slot_cap, device)
        self.nval, self.slot_cap, self.device = nval, slot_cap, device
        self.words = (nval + 31) // 32

    @staticmethod
    def _batch(cols, have_obl, **members):
        """``VoteColsBatch`` with the bitfield and (``have_obl``) the oblique columns of ``cols``."""
        c = _lib.att_cols(cols, ("attester_bitfield", "attester_bitfield_offs") + (_COL_KEYS if have_obl else ()))
        b = _lib.VoteColsBatch(bits=c.attester_bitfield, boffs=c.attester_bitfield_offs,
                               oblique_parent_hashes=c.oblique_parent_hashes, oblique_offs=c.oblique_offs,
                               oblique_first=c.oblique_first, **members)
        b._keep = c
        return b

    def tally_columns(self, cols, n, status, committee, parents_start, recent, members, coffs, balance, take=None,
                      n_oblique_total=None):
        """One tally of ``n`` rows held as torch device tensors, on the current stream
        (``pz_dev_vote_cache_tally``; asynchronous).  ``cols``: the decoder's columns
        (``attester_bitfield``(+``_offs``), the three oblique columns, optionally ``n_oblique``);
        ``status`` int32, ``committee`` int32 and ``parents_start`` int64 as
        ``pz_dev_check_attestations`` writes them; ``recent`` (k, 32) uint8, already normalised;
        ``members`` int32 / ``coffs`` int64: the committees as CSR; ``balance`` int64 (nval);
        ``take`` uint8 (optional).  ``n_oblique_total`` defaults to the elements ``oblique_offs``
        has room for (an upper bound is enough: an element no row names is never read)."""
        import torch

        dev = status.device
        have_obl = all(cols.get(k) is not None for k in _COL_KEYS)
        if n_oblique_total is None:
            n_oblique_total = max(int(cols["oblique_offs"].numel()) - 1, 0) if have_obl else 0
        n_recent = int(recent.numel()) // 32
        p = _lib.dptr
        b = self._batch(
            cols, have_obl, natt=n, n_oblique=p(cols.get("n_oblique")), n_oblique_total=n_oblique_total,
            status=p(status), committee=p(committee), parents_start=p(parents_start), take=p(take), recent=p(recent),
            n_recent=n_recent, members=p(members), coffs=p(coffs), ncomm=max(int(coffs.numel()) - 1, 0), balance=p(balance))
        nbytes = int(lib.dll.pz_vote_cache_scratch_bytes(n, n_recent, n_oblique_total))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)  # (reused in stream order by the allocator)
        lib.call("pz_dev_vote_cache_tally", self._h, _lib.ctypes.byref(b), scratch.data_ptr(), _lib.stream_ptr(dev))

    def tally_host(self, cols, n, status, committee, parents_start, recent, members, coffs, balance, take=None):
        """The same tally over host arrays (numpy; ``pz_vote_cache_tally``, synchronous)."""
        def arr(a, dt):
            return None if a is None else np.ascontiguousarray(a, dtype=dt)

        keep = {"status": arr(status, np.int32), "committee": arr(committee, np.uint32),
                "parents_start": arr(parents_start, np.uint64), "take": arr(take, np.uint8),
                "recent": arr(recent, np.uint8), "members": arr(members, np.uint32), "coffs": arr(coffs, np.uint64),
                "balance": arr(balance, np.uint64), "n_oblique": arr(cols.get("n_oblique"), np.uint64)}
        have_obl = all(cols.get(k) is not None for k in _COL_KEYS)
        dtypes = {"attester_bitfield": np.uint8, "oblique_parent_hashes": np.uint8}
        cols = {k: arr(cols.get(k), dtypes.get(k, np.uint64)) for k in ("attester_bitfield", "attester_bitfield_offs") + _COL_KEYS}
        b = self._batch(cols, have_obl, natt=n, n_oblique_total=len(cols["oblique_offs"]) - 1 if have_obl else 0,
                        n_recent=keep["recent"].size // 32, ncomm=len(keep["coffs"]) - 1,
                        **{k: v.ctypes.data for k, v in keep.items() if v is not None and v.size})
        lib.call("pz_vote_cache_tally", self._h, _lib.ctypes.byref(b))

    def _capacity(self):
        cap = _lib.ctypes.c_uint32(0)
        lib.call("pz_vote_cache_capacity", self._h, _lib.ctypes.byref(cap))
        self.slot_cap = int(cap.value)
        return self.slot_cap

    def reserve(self, min_slots, device_form=False):
        """Room for ``min_slots`` entries, the Go map's own growth (``pz_[dev_]vote_cache_reserve``;
        ``device_form``: on the current stream, asynchronous): every entry keeps its slot id, key,
        total and voters; at or below the capacity nothing is launched.  ``slot_cap`` follows the
        handle.  Returns the capacity."""
        if device_form:
            lib.call("pz_dev_vote_cache_reserve", self._h, int(min_slots), _lib.stream_ptr(self.device))
        else:
            lib.call("pz_vote_cache_reserve", self._h, int(min_slots))
        return self._capacity()

    def retain(self, hashes):
        """Keeps exactly the entries whose key is among ``hashes`` and renumbers them by ascending
        old slot id; no hash empties the cache.  A device tensor ((k, 32) uint8, 16-byte aligned)
        takes ``pz_dev_vote_cache_retain`` on the current stream, asynchronous; a list of byte strings
        or a (k, 32) uint8 array takes ``pz_vote_cache_retain``, synchronous.  What may be dropped is
        the caller's judgement (include/prysm_hip.h): the reference's map never forgets."""
        if hasattr(hashes, "data_ptr"):
            import torch

            n = int(hashes.numel()) // 32
            nbytes = int(lib.dll.pz_vote_cache_retain_scratch_bytes(self.slot_cap, n))
            scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=hashes.device)  # (reused in stream order)
            lib.call("pz_dev_vote_cache_retain", self._h, _lib.dptr(hashes), n, scratch.data_ptr(), _lib.stream_ptr(hashes.device))
            return
        if isinstance(hashes, np.ndarray):
            q = np.ascontiguousarray(hashes, dtype=np.uint8).reshape(-1, 32)
        else:
            q = np.frombuffer(b"".join(bytes(h) for h in hashes), dtype=np.uint8).reshape(-1, 32)
        lib.call("pz_vote_cache_retain", self._h, ptr(q), len(q))

    def read(self, strict=True):
        """``(hashes (k, 32) uint8, totals (k) uint64)`` in slot order (``pz_vote_cache_read``)."""
        cnt = _lib.ctypes.c_uint64(0)
        dll = lib.dll
        rc = dll.pz_vote_cache_read(self._h, None, None, 0, _lib.ctypes.byref(cnt))
        k = cnt.value
        hashes = np.zeros((k, 32), dtype=np.uint8)
        totals = np.zeros(k, dtype=np.uint64)
        if k:
            rc = dll.pz_vote_cache_read(self._h, hashes.ctypes.data, totals.ctypes.data, k, _lib.ctypes.byref(cnt))
        self._rc(rc, strict)
        return hashes[:cnt.value], totals[:cnt.value]

    def items(self, strict=True):
        """``{hash: VoteTotalDeposit}``."""
        hashes, totals = self.read(strict)
        return {hashes[i].tobytes(): int(totals[i]) for i in range(len(totals))}

    def lookup(self, hashes):
        """``(totals uint64, slots uint32)`` of the given 32-byte hashes (a list of byte strings or
        a (k, 32) uint8 array): VoteTotalDeposit, 0 when the map has no entry, and the slot id,
        0xFFFFFFFF when absent (``pz_vote_cache_lookup``: the table is probed on the device, the
        map is not downloaded).  Raises no sticky error."""
        if isinstance(hashes, np.ndarray):
            q = np.ascontiguousarray(hashes, dtype=np.uint8).reshape(-1, 32)
        else:
            q = np.frombuffer(b"".join(bytes(h) for h in hashes), dtype=np.uint8).reshape(-1, 32)
        totals = np.zeros(len(q), dtype=np.uint64)
        slots = np.zeros(len(q), dtype=np.uint32)
        lib.call("pz_vote_cache_lookup", self._h, ptr(q), len(q), ptr(totals), ptr(slots))
        return totals, slots

    def lookup_device(self, hashes, want_slots=True):
        """The same lookup over a device tensor ((k, 32) uint8, 16-byte aligned) on the current
        stream, asynchronous (``pz_dev_vote_cache_lookup``): ``(totals int64, slots int32 or
        None)`` device tensors, to be read as unsigned."""
        import torch

        n = int(hashes.numel()) // 32
        totals = torch.empty(n, dtype=torch.int64, device=hashes.device)
        slots = torch.empty(n, dtype=torch.int32, device=hashes.device) if want_slots else None
        p = _lib.dptr
        lib.call("pz_dev_vote_cache_lookup", self._h, p(hashes), n, p(totals), p(slots), _lib.stream_ptr(hashes.device))
        return totals, slots

    def _voters(self, h, strict):
        words = np.zeros(self.words, dtype=np.uint32)
        present = _lib.ctypes.c_int(0)
        key = np.frombuffer(bytes(h), dtype=np.uint8)
        assert key.size == 32
        rc = lib.dll.pz_vote_cache_voters(self._h, key.ctypes.data, words.ctypes.data, _lib.ctypes.byref(present))
        self._rc(rc, strict)
        return words, bool(present.value)

    def voters(self, h, strict=True):
        """VoterIndices of ``h``, ascending (KeyError when the map has no entry)."""
        words, present = self._voters(h, strict)
        if not present:
            raise KeyError(h)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:self.nval]
        return np.nonzero(bits)[0].astype(np.uint32)

    def total(self, h, strict=True):
        return self.items(strict).get(bytes(h), 0)

    def __contains__(self, h):
        return self._voters(h, True)[1]


__all__ = ["VoteCache", "DeviceVoteCache", "_lib"]
