"""The device-resident pending-attestation pool (prysm_amd/csrc/attpool.hip, prysm_amd/pending.py)
on the GPU.  The model is a Python list of pb.AttestationRecord: an append adds the rows with
status PZ_ATT_PROCESSED (and take != 0), a prune keeps slot > last_state_recalc.  Every result is
integers and bytes: every comparison is exact."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from oracle import ref
from oracle import replay as oreplay
from oracle import schema as opb
from prysm_amd import _lib, casper, pb, synth, wire
from prysm_amd import blockchain as bc
from prysm_amd.pending import DevicePendingAttestations, RecalcState
from prysm_amd.votes import DeviceVoteCache

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
M64 = (1 << 64) - 1
PROCESSED = 0
STATUSES = [0, 1, 2, 3, 4, 5, 6, 7, _lib.PZ_EINVAL]  # every PZ_ATT_* and PZ_EINVAL
OTHERS = STATUSES[1:]
# the write launch's long-range threshold, as the kernels compile it
LONG = int(re.search(r"kApLongBytes = (\d+);", open(os.path.join(ROOT, "prysm_amd", "csrc", "attpool_dev.h")).read()).group(1))
_BYTES = ("justified_block_hash", "shard_block_hash", "attester_bitfield", "oblique_parent_hashes")
_USED = {"justified_block_hash": "justified_block_hash_offs", "shard_block_hash": "shard_block_hash_offs",
         "attester_bitfield": "attester_bitfield_offs", "oblique_parent_hashes": "oblique_offs"}


# ---- helpers ---------------------------------------------------------------------------------------
def sizes(recs):
    """The model's seven sums, in CAPS' order."""
    return np.array([len(recs), sum(len(r.justified_block_hash) for r in recs), sum(len(r.shard_block_hash) for r in recs),
                     sum(len(r.attester_bitfield) for r in recs), sum(len(r.oblique_parent_hashes) for r in recs),
                     sum(len(h) for r in recs for h in r.oblique_parent_hashes), sum(len(r.aggregate_sig) for r in recs)],
                    dtype=U64)


def put(a, phase=0):
    """A host array on the device between 0xA5 pads: ``phase`` bytes before it (a 16-byte phase of
    its start) and 64 after (uint32/uint64 as int32/int64)."""
    import torch

    a = np.ascontiguousarray(a)
    raw = np.concatenate([np.full(phase, 0xA5, np.uint8), a.view(np.uint8).ravel(), np.full(64, 0xA5, np.uint8)])
    t = torch.from_numpy(raw).to("cuda:0")[phase:phase + a.nbytes]
    dt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.dtype.itemsize]
    return t.view(dt) if phase == 0 else t


def dev_cols(cols, phase=0):
    """Host columns as device tensors: every bytes column cut to its used part and started at
    16-byte phase ``phase``."""
    out = {}
    for k in wire.ATT_COLS:
        v = cols.get(k)
        if v is None:
            continue
        if k in _USED:
            v = v[:int(cols[_USED[k]][-1])]
        elif k == "aggregate_sig":
            v = v[:int(cols["aggregate_sig_first"][-1])]
        out[k] = put(v, phase if k in _BYTES else 0)
    return out


def append(pool, form, cols, n, status, committee, take=None, phase=0):
    status = np.ascontiguousarray(status, dtype=np.int32)
    committee = np.ascontiguousarray(committee, dtype=np.uint32)
    take = None if take is None else np.ascontiguousarray(take, dtype=np.uint8)
    if form == "host":
        pool.append_host(cols, n, status, committee, take)
    else:
        pool.append_columns(dev_cols(cols, phase), n, put(status), put(committee), None if take is None else put(take))


def kept(recs, status, take=None):
    return [r for i, r in enumerate(recs) if status[i] == PROCESSED and (take is None or take[i])]


def check(pool, model, committee=None, strict=True):
    np.testing.assert_array_equal(pool.counts(strict), sizes(model))
    assert pool.records(strict) == model
    if committee is not None:
        np.testing.assert_array_equal(pool.columns(strict)["committee"], np.asarray(committee, dtype=np.uint32))


def pool_for(recs, slack=0, device=0):
    caps = sizes(recs) + U64(slack)
    caps[0] = max(int(caps[0]), 1)
    return DevicePendingAttestations(caps, device)


def rec(rng, slot=None, jb=32, sb=32, bf=4, elems=(), nsig=0, shard=None):
    return pb.AttestationRecord(
        slot=int(rng.integers(0, 200)) if slot is None else slot,
        shard_id=int(rng.integers(0, 1024)) if shard is None else shard, justified_slot=int(rng.integers(0, 100)),
        justified_block_hash=rng.bytes(jb), shard_block_hash=rng.bytes(sb), attester_bitfield=rng.bytes(bf),
        oblique_parent_hashes=[rng.bytes(e) for e in elems],
        aggregate_sig=[int(x) for x in rng.integers(0, 1 << 63, size=nsig, dtype=np.uint64)])


def fill_canaries(pool):
    for t in pool.raw_columns().values():
        t.fill_(0xA5)


def check_canaries(pool, n):
    """Every byte after the used part of the bytes columns and aggregate_sig is still 0xA5."""
    used = {"justified_block_hash": int(n[1]), "shard_block_hash": int(n[2]), "attester_bitfield": int(n[3]),
            "oblique_parent_hashes": int(n[5]), "aggregate_sig": 8 * int(n[6])}
    for k, t in pool.raw_columns().items():
        tail = t[used[k]:].cpu().numpy()
        assert (tail == 0xA5).all(), k


PATTERNS = {"all": lambda n: np.ones(n, bool), "none": lambda n: np.zeros(n, bool),
            "alternating": lambda n: np.arange(n) % 2 == 1, "first": lambda n: np.arange(n) == 0,
            "last": lambda n: np.arange(n) == n - 1}


# ---- 1: selection and order ------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_selection_and_order(n, form):
    """The tile edges, every keep pattern, by status alone (take NULL) and by take over statuses
    drawn from every value: ten appends into one pool equal the model."""
    rng = np.random.default_rng(n)
    batches = []
    for name, pat in PATTERNS.items():
        for with_take in (False, True):
            recs = [rec(rng, bf=int(rng.integers(0, 6)), elems=(3,) * int(rng.integers(0, 2)), nsig=int(rng.integers(0, 3)))
                    for _ in range(n)]
            keep = pat(n)
            if with_take:
                status = rng.choice(STATUSES, size=n)
                take = keep.astype(np.uint8)
            else:
                status = np.where(keep, PROCESSED, rng.choice(OTHERS, size=n))
                take = None
            batches.append((recs, status, take, rng.integers(0, 4096, size=n)))
    want, want_comm = [], []
    for recs, status, take, comm in batches:
        want += kept(recs, status, take)
        want_comm += [c for i, c in enumerate(comm) if status[i] == PROCESSED and (take is None or take[i])]
    pool = pool_for(want, slack=3)
    model = []
    for recs, status, take, comm in batches:
        append(pool, form, wire.attestation_columns(recs), n, status, comm, take)
        model += kept(recs, status, take)
        np.testing.assert_array_equal(pool.counts(), sizes(model))
    check(pool, want, want_comm)


def test_a_second_scan_round():
    """262,401 minimal rows: 1,026 tiles, so the scan launch walks a column in two rounds with a
    carry.  Compared column by column (a quarter of a million records are not built)."""
    n = 262401
    rng = np.random.default_rng(7)
    slot = rng.integers(1, 1 << 40, size=n).astype(U64)
    shard = rng.integers(0, 1024, size=n).astype(U64)
    status = rng.choice(STATUSES, size=n).astype(np.int32)
    take = (np.arange(n) % 2).astype(np.uint8)
    comm = rng.integers(0, 4096, size=n).astype(np.uint32)
    keep = (status == PROCESSED) & (take != 0)
    k = int(keep.sum())
    assert k > 10000
    pool = DevicePendingAttestations([k, 1, 1, 1, 1, 1, 1])
    pool.append_columns({"slot": put(slot), "shard_id": put(shard)}, n, put(status), put(comm), put(take))
    np.testing.assert_array_equal(pool.counts(), [k, 0, 0, 0, 0, 0, 0])
    c = pool.columns()
    np.testing.assert_array_equal(c["slot"], slot[keep])
    np.testing.assert_array_equal(c["shard_id"], shard[keep])
    np.testing.assert_array_equal(c["committee"], comm[keep])
    assert not c["justified_slot"].any()
    for key in ("justified_block_hash_offs", "shard_block_hash_offs", "attester_bitfield_offs", "oblique_first",
                "aggregate_sig_first"):
        assert c[key].shape == (k + 1,) and not c[key].any(), key
    np.testing.assert_array_equal(pool.shard32(), shard[keep].astype(np.uint32))


# ---- 2: range lengths and alignment ------------------------------------------------------------------
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 48, 64, 65, LONG - 1, LONG, LONG + 1]


@pytest.mark.parametrize("phase", range(16))
def test_range_lengths_and_alignment(phase):
    """Every length of LENGTHS in each bytes field, as one element and (times eight) as the sig
    values' bytes; a first row of ``phase`` bytes in every range sets the destination's 16-byte
    phase, a padded source column the source's; 0xA5 around the source, canaries after the
    destination."""
    rng = np.random.default_rng(100 + phase)
    recs = [rec(rng, jb=phase, sb=phase, bf=phase, elems=(phase,), nsig=0)]
    recs += [rec(rng, jb=L, sb=L, bf=L, elems=(L,), nsig=L % 67) for L in LENGTHS]
    recs += [rec(rng, jb=0, sb=0, bf=0, nsig=LONG // 8 + 1)]  # sig values longer than the threshold
    n = len(recs)
    pool = pool_for(recs, slack=40)
    fill_canaries(pool)
    status = np.zeros(n, np.int32)
    append(pool, "device", wire.attestation_columns(recs), n, status, np.arange(n), phase=(5 * phase + 3) % 16)
    check(pool, recs, np.arange(n))
    check_canaries(pool, sizes(recs))
    # a second append starts where the first one stopped: another destination phase, same source
    append(pool, "device", wire.attestation_columns(recs[1:3]), 2, status[:2], [7, 8], phase=phase)
    check(pool, recs + recs[1:3])
    check_canaries(pool, sizes(recs + recs[1:3]))


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_long_bitfield_among_short_ones(where):
    """The configs[3] shape in small: 40 rows of ~32-byte bitfields and one of 128 KiB."""
    rng = np.random.default_rng(5)
    recs = [rec(rng, bf=int(rng.integers(26, 33))) for _ in range(40)]
    recs.insert({"first": 0, "middle": 20, "last": 40}[where], rec(rng, bf=128 * 1024))
    n = len(recs)
    status = np.zeros(n, np.int32)
    status[3] = 2
    want = kept(recs, status)
    for form in ("device", "host"):
        pool = pool_for(want, slack=5)
        fill_canaries(pool)
        append(pool, form, wire.attestation_columns(recs), n, status, np.arange(n), phase=9)
        check(pool, want)
        check_canaries(pool, sizes(want))


# ---- 3: nested columns -------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
def test_nested_columns(form):
    rng = np.random.default_rng(3)
    recs = []
    for ne in (0, 1, 13, 14, 65):
        for nsig in (0, 1, 16, 17):
            elems = [0 if e % 5 == 4 else int(rng.integers(1, 41)) for e in range(ne)]  # (empty elements too)
            recs.append(rec(rng, elems=elems, nsig=nsig))
    n = len(recs)
    status = rng.choice([0, 0, 0, 3], size=n)
    want = kept(recs, status)
    pool = pool_for(want + recs[:6] * 2, slack=2)
    append(pool, form, wire.attestation_columns(recs), n, status, np.arange(n))
    check(pool, want)
    # NULL oblique and sig columns, NULL scalar columns: empty ranges and zeros
    cols = wire.attestation_columns(recs[:6])
    for k in ("oblique_parent_hashes", "oblique_offs", "oblique_first", "aggregate_sig", "aggregate_sig_first", "slot",
              "justified_slot"):
        cols[k] = None
    bare = [pb.AttestationRecord(shard_id=r.shard_id, justified_block_hash=r.justified_block_hash,
                                 shard_block_hash=r.shard_block_hash, attester_bitfield=r.attester_bitfield) for r in recs[:6]]
    append(pool, form, cols, 6, np.zeros(6, np.int32), np.arange(6))
    check(pool, want + bare)
    # every offsets column NULL: rows of scalars alone
    only = {"slot": np.arange(5, 11, dtype=U64)}
    append(pool, form, only, 6, np.zeros(6, np.int32), np.arange(6))
    check(pool, want + bare + [pb.AttestationRecord(slot=s) for s in range(5, 11)])


# ---- 4: appends accumulate -------------------------------------------------------------------------
def active_state_bytes(recs):
    a = opb.ActiveState()
    for r in recs:
        a.pending_attestations.add(slot=r.slot, shard_id=r.shard_id, justified_slot=r.justified_slot,
                                   justified_block_hash=r.justified_block_hash, shard_block_hash=r.shard_block_hash,
                                   attester_bitfield=r.attester_bitfield, oblique_parent_hashes=r.oblique_parent_hashes,
                                   aggregate_sig=r.aggregate_sig)
    return ref.marshal(a)


def test_appends_accumulate_and_wire():
    """Three appends of different shapes into one pool (device, host, device): the model's
    concatenation, offsets rebased at a non-zero base; wire(1) is ActiveState field 1."""
    rng = np.random.default_rng(4)
    shapes = [[rec(rng, bf=int(rng.integers(1, 40)), elems=(32,), nsig=2) for _ in range(300)],
              [rec(rng, jb=0, sb=33, bf=700, elems=(1, 0, 40), nsig=0) for _ in range(7)],
              [rec(rng, jb=31, sb=0, bf=0, elems=(), nsig=17, shard=0, slot=0) for _ in range(70)]]
    model, comm = [], []
    pool = pool_for([r for s in shapes for r in s], slack=1)
    assert pool.wire(1)[0] == b""
    for k, (recs, form) in enumerate(zip(shapes, ["device", "host", "device"])):
        status = rng.choice([0, 0, 5], size=len(recs))
        append(pool, form, wire.attestation_columns(recs), len(recs), status, np.arange(len(recs)) + 1000 * k)
        model += kept(recs, status)
        comm += [i + 1000 * k for i in range(len(recs)) if status[i] == PROCESSED]
        check(pool, model, comm)
    raw, offs = pool.wire(1)
    assert raw == active_state_bytes(model)
    host_raw, host_offs = wire.attestations_device(wire.attestation_columns(model), len(model), 1)
    assert raw == host_raw
    np.testing.assert_array_equal(offs, host_offs)
    assert pool.wire(0)[0] == wire.attestations_device(wire.attestation_columns(model), len(model), 0)[0]


# ---- 5: capacity -----------------------------------------------------------------------------------
def raw_snapshot(pool):
    return {k: t.cpu().numpy().copy() for k, t in pool.raw_columns().items()}


@pytest.mark.parametrize("form", ["device", "host"])
@pytest.mark.parametrize("c", range(7))
def test_a_call_that_does_not_fit_changes_nothing(c, form):
    """Capacity c alone is one short for the second call: counts, every column and the canaries
    are those of a twin pool that never saw it; counts() reports PZ_ERANGE; a call that fits lands."""
    rng = np.random.default_rng(50 + c)
    first = [rec(rng, elems=(5, 0), nsig=3) for _ in range(9)]
    second = [rec(rng, bf=int(rng.integers(1, 9)), elems=(2,), nsig=1) for _ in range(300)]  # (two tiles)
    caps = sizes(first + second) + U64(11)
    caps[c] = sizes(first + second)[c] - U64(1)
    pool, twin = DevicePendingAttestations(caps), DevicePendingAttestations(caps)
    for p in (pool, twin):
        fill_canaries(p)
        append(p, form, wire.attestation_columns(first), len(first), np.zeros(len(first), np.int32), np.arange(9))
    append(pool, form, wire.attestation_columns(second), len(second), np.zeros(len(second), np.int32), np.arange(300))
    with pytest.raises(_lib.PzError) as e:
        pool.counts()
    assert e.value.code == _lib.PZ_ERANGE
    np.testing.assert_array_equal(pool.counts(strict=False), twin.counts())
    a, b = pool.columns(strict=False), twin.columns()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    ra, rb = raw_snapshot(pool), raw_snapshot(twin)
    for k in ra:
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    check_canaries(pool, sizes(first))
    check(pool, first, strict=False)
    append(pool, form, wire.attestation_columns(second[:-1]), len(second) - 1, np.zeros(len(second) - 1, np.int32), np.arange(299))
    check(pool, first + second[:-1], strict=False)


# ---- 6: prune ---------------------------------------------------------------------------------------
def test_prune():
    rng = np.random.default_rng(6)
    recs = [rec(rng, slot=int(s), bf=int(rng.integers(0, 40)), elems=(7,) * int(rng.integers(0, 4)), nsig=int(rng.integers(0, 3)))
            for s in rng.integers(10, 100, size=600)]
    recs[17] = rec(rng, slot=99, bf=2000)  # a long range through the prune
    pool = pool_for(recs)
    fill_canaries(pool)
    pool.prune(5)  # an empty pool
    check(pool, [])
    comm = np.arange(len(recs)) * 3
    append(pool, "device", wire.attestation_columns(recs), len(recs), np.zeros(len(recs), np.int32), comm)
    check_canaries(pool, sizes(recs))
    model = list(zip(recs, comm))
    # what each buffer set held when it was last live (the second one: the zeros it was created with):
    # a prune writes the kept rows at its start and must leave every byte after them as it was
    snap, live = {0: None, 1: {k: np.zeros(t.numel(), np.uint8) for k, t in pool.raw_columns().items()}}, 0
    for lsr in (0, 9, 50, 50, 70):  # keeps all; below every slot; between; the same again; between
        snap[live] = raw_snapshot(pool)
        pool.prune(lsr)
        live ^= 1
        model = [(r, c) for r, c in model if r.slot > lsr]
        check(pool, [r for r, _ in model], [c for _, c in model])
        np.testing.assert_array_equal(pool.shard32(), [r.shard_id for r, _ in model])
        n = sizes([r for r, _ in model])
        used = {"justified_block_hash": int(n[1]), "shard_block_hash": int(n[2]), "attester_bitfield": int(n[3]),
                "oblique_parent_hashes": int(n[5]), "aggregate_sig": 8 * int(n[6])}
        for k, t in raw_snapshot(pool).items():
            np.testing.assert_array_equal(t[used[k]:], snap[live][k][used[k]:], err_msg=k)
    assert 0 < len(model) < 600
    more = [rec(rng, slot=80, elems=(3, 3)) for _ in range(30)]  # append after a prune
    append(pool, "host", wire.attestation_columns(more), 30, np.zeros(30, np.int32), np.arange(30))
    model += list(zip(more, range(30)))
    check(pool, [r for r, _ in model], [c for _, c in model])
    raw, _ = pool.wire(1)
    assert raw == active_state_bytes([r for r, _ in model])
    pool.prune(1000)  # above every slot
    check(pool, [])
    pool.prune(0)
    check(pool, [])
    append(pool, "device", wire.attestation_columns(more), 30, np.zeros(30, np.int32), np.arange(30))
    check(pool, more)


# ---- 7: errors --------------------------------------------------------------------------------------
def call(name, *args):
    return getattr(_lib.lib.dll, name)(*args)


def test_argument_errors_are_einval():
    import torch

    rng = np.random.default_rng(8)
    recs = [rec(rng, elems=(3,), nsig=1) for _ in range(4)]
    pool = pool_for(recs, slack=8)
    h = pool._h
    d = dev_cols(wire.attestation_columns(recs))
    cols = _lib.AttestationCols(*[d[k].data_ptr() for k in wire.ATT_COLS])
    status, comm = put(np.zeros(4, np.int32)), put(np.arange(4, dtype=np.uint32))
    scr = torch.zeros(int(_lib.lib.dll.pz_att_pool_scratch_bytes(4)) + 16, dtype=torch.uint8, device="cuda:0")
    sp, cp, tp = status.data_ptr(), comm.data_ptr(), scr.data_ptr()
    E = _lib.PZ_EINVAL
    assert call("pz_dev_att_pool_append", h, ctypes.byref(cols), 4, None, cp, None, tp, None) == E
    assert call("pz_dev_att_pool_append", h, ctypes.byref(cols), 4, sp, None, None, tp, None) == E
    assert call("pz_dev_att_pool_append", h, None, 4, sp, cp, None, tp, None) == E
    assert call("pz_dev_att_pool_append", h, ctypes.byref(cols), 4, sp, cp, None, None, None) == E
    assert call("pz_dev_att_pool_append", h, ctypes.byref(cols), 4, sp, cp, None, tp + 8, None) == E
    assert call("pz_dev_att_pool_append", None, ctypes.byref(cols), 4, sp, cp, None, tp, None) == E
    for data, offs in (("justified_block_hash", "justified_block_hash_offs"), ("shard_block_hash", "shard_block_hash_offs"),
                       ("attester_bitfield", "attester_bitfield_offs"), ("oblique_parent_hashes", "oblique_first"),
                       ("oblique_offs", "oblique_first"), ("aggregate_sig", "aggregate_sig_first")):
        bad = _lib.AttestationCols(*[None if k == data else d[k].data_ptr() for k in wire.ATT_COLS])
        assert call("pz_dev_att_pool_append", h, ctypes.byref(bad), 4, sp, cp, None, tp, None) == E, data
        assert call("pz_att_pool_append", h, ctypes.byref(bad), 4, sp, cp, None) == E, data
    assert call("pz_att_pool_append", h, ctypes.byref(cols), 4, None, cp, None) == E
    # n == 0 launches nothing, whatever else is NULL
    assert call("pz_dev_att_pool_append", h, None, 0, None, None, None, None, None) == _lib.PZ_OK
    assert call("pz_att_pool_append", h, None, 0, None, None, None) == _lib.PZ_OK
    out = ctypes.c_void_p()
    caps = np.array([0, 8, 8, 8, 8, 8, 8], dtype=U64)
    assert call("pz_att_pool_new", caps.ctypes.data, 0, ctypes.byref(out)) == E and not out.value
    assert call("pz_att_pool_new", None, 0, ctypes.byref(out)) == E
    assert call("pz_att_pool_new", pool.caps.ctypes.data, 0, None) == E
    assert call("pz_att_pool_counts", h, None) == E
    torch.cuda.synchronize()
    check(pool, [])  # nothing was written
    assert not scr.cpu().numpy().any()


@pytest.mark.parametrize("form", ["device", "host"])
def test_an_inverted_range_empties_its_row(form):
    rng = np.random.default_rng(9)
    recs = [rec(rng, bf=9, elems=(4,), nsig=1) for _ in range(5)]
    cols = wire.attestation_columns(recs)
    o = cols["attester_bitfield_offs"]
    o[2], o[3] = o[3], o[2]  # row 2 inverted; rows 1 and 3 (not kept) change length
    status = np.array([0, 3, 0, 3, 0], np.int32)
    pool = pool_for(recs, slack=4)
    append(pool, form, cols, 5, status, np.arange(5))
    with pytest.raises(_lib.PzError) as e:
        pool.counts()
    assert e.value.code == _lib.PZ_EINVAL
    check(pool, [recs[0], pb.AttestationRecord(), recs[4]], [0, 0xFFFFFFFF, 4], strict=False)


@pytest.mark.parametrize("form", ["device", "host"])
def test_shard32_saturates(form):
    rng = np.random.default_rng(10)
    shards = [5, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, 1 << 63, M64]
    recs = [rec(rng, shard=s) for s in shards]
    pool = pool_for(recs)
    append(pool, form, wire.attestation_columns(recs), len(recs), np.zeros(len(recs), np.int32), np.arange(len(recs)))
    check(pool, recs)
    np.testing.assert_array_equal(pool.shard32(), [5, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF])
    pool.prune(0)  # (the column travels through a prune as it is)
    keep = [r.slot > 0 for r in recs]
    np.testing.assert_array_equal(pool.shard32(), np.array([5, 0xFFFFFFFE] + [0xFFFFFFFF] * 4, np.uint32)[keep])


# ---- 8: pend_serialized_blocks on mixed and rejected blocks ----------------------------------------------
def table(cstate):
    return [[(sc.shard_id, list(sc.committee)) for sc in arr.array_shard_and_committee]
            for arr in cstate.shard_and_committees_for_slots]


def test_pend_serialized_blocks_rejected_and_mixed_blocks():
    """The four-block batch of test_tally_serialized_blocks_rejected_and_mixed_blocks against the
    genesis state: all pass / the last fails / the last passes after a failure / no attestation."""
    rng = np.random.default_rng(10)
    _, cs = ref.new_genesis_states(1024)
    tab = table(cs)

    def rec8(slot, j, good=True):
        shard, comm = tab[slot][j % len(tab[slot])]
        bits = rng.random(len(comm)) < 0.6
        return pb.AttestationRecord(slot=slot, shard_id=shard, justified_slot=0 if good else 9,
                                    attester_bitfield=np.packbits(bits.astype(np.uint8)).tobytes(),
                                    oblique_parent_hashes=[rng.bytes(33)])

    def block(slot, atts):
        return pb.BeaconBlock(parent_hash=rng.bytes(32), slot_number=slot, timestamp=pb.Timestamp(8 * slot, 0), attestations=atts)

    blocks = [block(5, [rec8(1, 0), rec8(2, 1)]), block(6, [rec8(1, 0), rec8(2, 0, good=False)]),
              block(7, [rec8(3, 0, good=False), rec8(3, 1)]), block(8, [])]
    data, offs = bc.serialize_blocks(blocks)
    clean, mixed = blocks[0].attestations, blocks[2].attestations[1]
    ids = {(s, e[0]): k for k, (s, e) in enumerate((s, e) for s, arr in enumerate(tab) for e in arr)}
    comm_of = lambda a: ids[(a.slot, a.shard_id)]  # noqa: E731
    for candidate, want in ((None, clean + [mixed]), ([1, 1, 0, 1], clean), ([0, 1, 1, 1], [mixed])):
        pool = DevicePendingAttestations([16, 600, 600, 600, 16, 600, 16])
        open_, first, status = bc.pend_serialized_blocks(pool, data, offs, 0, 0, 128, tab, candidate=candidate)
        assert list(first) == [0, 2, 4, 6, 6]
        assert list(status) == [0, 0, 0, 4, 4, 0]  # 4: PZ_ATT_JUSTIFIED
        assert list(open_) == [candidate is None or bool(candidate[0]), False, candidate is None or bool(candidate[2]), False]
        check(pool, want, [comm_of(a) for a in want])
    # tally_serialized_blocks with a pool appends the same rows from its one decode
    recent = [rng.bytes(32) for _ in range(128)]
    balance = np.array([v.balance for v in cs.validators], U64)
    pool, cache, alone = DevicePendingAttestations([16, 600, 600, 600, 16, 600, 16]), DeviceVoteCache(1024, 256), DeviceVoteCache(1024, 256)
    r1 = bc.tally_serialized_blocks(cache, data, offs, 0, 0, 128, tab, recent, balance, pending=pool)
    r0 = bc.tally_serialized_blocks(alone, data, offs, 0, 0, 128, tab, recent, balance)
    assert all(np.array_equal(a, b) for a, b in zip(r0, r1)) and cache.items() == alone.items() and cache.items()
    check(pool, clean + [mixed])


# ---- 9: the epoch from the pool ----------------------------------------------------------------------
@pytest.mark.parametrize("n,inactive", [(4096, False), (5000, True)])
def test_epoch_from_the_pool(n, inactive):
    """A synthetic instance whose attestations went through the pool in two appends: count / finish
    over pool.epoch_batch equal the same instance with the attestations uploaded directly, and the
    oracle."""
    import torch

    from epoch_ref_helpers import oracle_epoch
    from torch_epoch import DeviceEpoch

    shuffled = casper.shuffle_indices(ref.bytes_to_hash(b"A"), np.arange(n, dtype=np.uint32))
    inst = synth.epoch_batch(n, 1, seed=5, shuffled=shuffled)
    if inactive:
        rng = np.random.default_rng(1)
        inst["start"][:, rng.random(n) < 0.1] = 7
        inst["end"][:, rng.random(n) < 0.1] = 1
    natt = int(inst["natt"])
    bo = inst["boffs"].astype(np.int64)
    recs = [pb.AttestationRecord(slot=int(inst["att_slot"][a]), shard_id=int(inst["att_shard"][a]),
                                 attester_bitfield=inst["bits"][bo[a]:bo[a + 1]].tobytes()) for a in range(natt)]
    pool = pool_for(recs, slack=64)
    cut = natt // 3
    append(pool, "host", wire.attestation_columns(recs[:cut]), cut, np.zeros(cut, np.int32), inst["att_comm"][:cut])
    # the second call through the device form, every other row a failed one that is left out
    rest = [r for a in recs[cut:] for r in (a, pb.AttestationRecord(slot=1, attester_bitfield=b"\xff\xff"))]
    status = np.tile(np.array([0, 6], np.int32), natt - cut)
    append(pool, "device", wire.attestation_columns(rest), len(rest), status, np.repeat(inst["att_comm"][cut:], 2))
    np.testing.assert_array_equal(pool.counts()[[0, 3]], [natt, int(bo[-1])])

    direct, pooled = DeviceEpoch(inst, torch.device("cuda", 0)), DeviceEpoch(inst, torch.device("cuda", 0))
    b = pool.epoch_batch(pooled.parts[0].batch)
    assert b.natt == natt and b.max_inst_bytes == int(bo[-1]) and b.ninst == 1
    direct.step()
    pooled.step()
    torch.cuda.synchronize()
    want, got = direct.results(), pooled.results()
    for w, g in zip(want, got):
        np.testing.assert_array_equal(g, w)
    nb, applied, nxt, v, t, w = oracle_epoch(inst, 0)
    bal, scal, vote, total, win = got
    assert applied and bool(scal[0, _lib.SCAL_APPLIED]) and not scal[0, _lib.SCAL_ERR_XL]
    np.testing.assert_array_equal(bal[0], nb)
    assert int(scal[0, _lib.SCAL_NEXT_BAL]) == nxt
    np.testing.assert_array_equal(vote[0], v)
    np.testing.assert_array_equal(total[0], t)
    np.testing.assert_array_equal(win[0], w)
    assert (win[0] != 0xFFFFFFFF).any()


# ---- 10: the chain -----------------------------------------------------------------------------------
def late_chain(nval, nblocks, seed):
    """synth.chain_blocks with the attestations of blocks 96..127 moved to slot 65 (the committee of
    ShardAndCommitteesForSlots[1]), so the stateRecalc at block 128 (lastStateRecalc 64) both keeps
    and drops pending attestations; chain_blocks alone attests only slots 0 and 64, which every
    prune drops whole.  Parent hashes are chained again (hashlib: input generation only)."""
    blocks = synth.chain_blocks(nval, nblocks, seed=seed)
    _, cs = ref.new_genesis_states(nval)
    sc = cs.shard_and_committees_for_slots[1].array_shard_and_committee[0]
    rng = np.random.default_rng(seed + 1)
    parent = None
    for b in blocks:
        if parent is not None:
            b.parent_hash = parent
        if 96 <= b.slot_number < 128:
            k = len(sc.committee)
            bits = rng.random(8 * ((k + 7) // 8)) < 0.25
            bits[k:] = False
            a = b.attestations[0]
            a.slot, a.shard_id, a.attester_bitfield = 65, sc.shard_id, np.packbits(bits).tobytes()
        parent = hashlib.blake2b(wire.beacon_block(b), digest_size=64).digest()[:32]
    return blocks


def as_pb(a):
    return pb.AttestationRecord(a.slot, a.shard_id, a.justified_slot, bytes(a.justified_block_hash), bytes(a.shard_block_hash),
                                bytes(a.attester_bitfield), [bytes(h) for h in a.oblique_parent_hashes],
                                [int(x) for x in a.aggregate_sig])


def test_the_chain_through_the_pool():
    """130 blocks at 1,024 validators, block by block beside oracle.replay.Chain as
    test_tally_serialized_blocks_matches_the_engine steps: tally_serialized_blocks(pending=pool)
    against the state just before each block, state_recalc_device first at the two transition
    blocks.  (The transition block's own votes reach the cache after the justification loop here;
    no block of this chain comes near two thirds of the deposits, so the loop reads zeros either
    way, as the oracle's justified slot shows.)

    The oracle alone shows, and the test asserts: the transition at block 64 sets a crosslink
    record; the prune at block 128 both keeps and drops rows.  No transition of a 1,024-validator
    chain can apply the rewards: once the attesters' deposit reaches two thirds, CalculateRewards
    reads CheckBit(last bitfield, validator index) past a 2-byte committee bitfield and the
    reference panics (oracle: GoPanic at block 64 for participation (1.0, 0.5)); rewards through
    the pool are test_epoch_from_the_pool's."""
    nval, nblocks = 1024, 130
    blocks = late_chain(nval, nblocks, seed=4)
    data, offs = bc.serialize_blocks(blocks)
    engine = bc.BeaconChain(nval)
    chain = oreplay.Chain(nval)
    cache = DeviceVoteCache(nval, 512)
    pool = DevicePendingAttestations([256, 256 * 32, 256 * 32, 256 * 8, 256, 256 * 32, 512])
    cs0 = chain.C
    tab0 = table(cs0)
    state = RecalcState([v.balance for v in cs0.validators], [v.start_dynasty for v in cs0.validators],
                        [v.end_dynasty for v in cs0.validators], [v for arr in tab0 for e in arr for v in e[1]],
                        bc._committee_table(tab0)[3], cs0.crosslink_records, last_state_recalc=cs0.last_state_recalc,
                        justified_streak=cs0.justified_streak, last_justified_slot=cs0.last_justified_slot,
                        last_finalized_slot=cs0.last_finalized_slot, current_dynasty=cs0.current_dynasty,
                        total_deposits=cs0.total_deposits)
    tables = {}
    seen = {"crosslink": 0, "kept_and_dropped": 0, "transitions": 0}

    def compare(i):
        _, A, C = chain.candidate
        np.testing.assert_array_equal(state.balances(), np.array([v.balance for v in C.validators], U64))
        assert [(r.dynasty, r.slot, bytes(r.blockhash)) for r in state.crosslink_records] == \
            [(r.dynasty, r.slot, bytes(r.blockhash)) for r in C.crosslink_records], i
        assert (state.last_justified_slot, state.justified_streak, state.last_finalized_slot, state.total_deposits,
                state.last_state_recalc, state.current_dynasty) == \
            (C.last_justified_slot, C.justified_streak, C.last_finalized_slot, C.total_deposits, C.last_state_recalc,
             C.current_dynasty), i
        assert pool.records() == [as_pb(a) for a in A.data.pending_attestations], i
        raw, _ = pool.wire(1)
        assert raw and engine.state_bytes("cand_active").startswith(raw), i

    for i, blk in enumerate(blocks):
        C, A = chain.C, chain.A.data
        if C.last_state_recalc not in tables:
            tables[C.last_state_recalc] = table(C)
        transition = blk.slot_number >= state.last_state_recalc + 64
        if transition:
            before = len(pool)
            xl = [(r.dynasty, r.slot) for r in state.crosslink_records]
            bc.state_recalc_device(pool, cache, state, [bytes(h) for h in chain.candidate[1].data.recent_block_hashes],
                                   blk.slot_number)
            after = len(pool)
            seen["transitions"] += 1
            seen["crosslink"] += xl != [(r.dynasty, r.slot) for r in state.crosslink_records]
            seen["kept_and_dropped"] += 0 < after < before
        lo, hi = int(offs[i]), int(offs[i + 1])
        report, first, status = bc.tally_serialized_blocks(
            cache, data[lo:hi], np.array([0, hi - lo], dtype=U64), C.last_justified_slot, C.last_state_recalc,
            len(A.recent_block_hashes), tables[C.last_state_recalc], [bytes(h) for h in A.recent_block_hashes],
            np.array([v.balance for v in C.validators], U64), pending=pool, candidate=[1])
        assert list(report) == [bc.BLOCK_TALLIED] and (status == PROCESSED).all(), i
        r = chain.process_block(oreplay.to_pb_block(blk))
        assert r["status"] == "processed" and r["transition"] == transition, i
        engine.process_serialized(data[lo:hi], np.array([0, hi - lo], dtype=U64))
        if transition or i + 1 == nblocks:
            compare(i)
    assert seen == {"crosslink": 1, "kept_and_dropped": 1, "transitions": 2}
