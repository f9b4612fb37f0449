"""The two device-resident proto3 encoders (pz_dev_wire_validators, pz_dev_wire_attestations)
against Google's protobuf runtime (tests/wire_cases.py), byte-exact, at the edges their kernels'
addressing depends on: every scalar-column instantiation and the bytes kernel past one tile, the
64 KiB stage at its limit, every (tile base, d_out) alignment, maximum-size records; every
(segment length, source alignment) pair, every varint length in every sub-lane, the element and
value counts at the row path's limits, NULL columns and ranges that do not start at 0.

Every column is carved out of poison (a constant 0xFF, or a random stream), every output (d_out,
d_offsets, d_total) out of a larger 0xA5-filled tensor with at least 64 guard bytes on either side,
and every byte of that tensor outside the expected result must still be 0xA5 after the call.  The
scratch is 0xFF-filled before every call."""
import ctypes

import numpy as np
import pytest
import torch

import wire_cases as wc
from prysm_amd import _lib

pytestmark = pytest.mark.gpu

U64 = np.uint64
GUARD = 64
FILL = 0xA5
KEY = 0x5A
OUT_SKEWS = (0, 1, 4, 7, 8, 15)


@pytest.fixture(autouse=True)
def device_checks():
    """After every test: wait for the device (a fault surfaces here) and make one more call, whose
    return code is the library's hipGetLastError path.  A device error ends the session: nothing
    more is started on a device that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
        tot = torch.zeros(1, dtype=torch.int64, device="cuda")
        cols = _lib.ValidatorCols()
        _lib.lib.call("pz_dev_wire_validators", ctypes.byref(cols), 0, 0, None, None, tot.data_ptr(), tot.data_ptr(),
                      _lib.stream_ptr(0))
        torch.cuda.synchronize()
    except (RuntimeError, _lib.PzError) as e:
        pytest.exit("the device reported an error, no further test is run on it: %s" % e, returncode=3)


class Carve:
    """``nbytes`` at an address that is ``skew`` mod 16 inside a tensor filled with 0xA5, at least 64
    guard bytes on either side."""

    def __init__(self, nbytes, skew=0):
        self.raw = torch.full((nbytes + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device="cuda")
        self.lo = GUARD + (skew - (self.raw.data_ptr() + GUARD)) % 16
        self.ptr = self.raw.data_ptr() + self.lo
        assert self.ptr % 16 == skew and self.lo + nbytes + GUARD <= self.raw.numel()

    def check(self, want, what):
        """The area starts with ``want``; every other byte of the tensor is still 0xA5.  (The copy
        waits for the current stream only.)"""
        if isinstance(want, bytes):
            want = np.frombuffer(want, dtype=np.uint8) if want else np.zeros(0, dtype=np.uint8)
        want = np.ascontiguousarray(want).view(np.uint8)
        host, lo = self.raw.cpu().numpy(), self.lo
        assert (host[:lo] == FILL).all(), "bytes in front of %s were written" % what
        got = host[lo:lo + len(want)]
        if not np.array_equal(got, want):
            at = int(np.flatnonzero(got != want)[0])
            pytest.fail("%s differs from the reference at byte %d of %d: got %s, want %s" % (
                what, at, len(want), got[max(at - 8, 0):at + 8].tobytes().hex(), want[max(at - 8, 0):at + 8].tobytes().hex()))
        bad = np.flatnonzero(host[lo + len(want):] != FILL)
        assert not len(bad), "%s: byte %d behind its %d result bytes was written" % (what, int(bad[0]), len(want))

    def untouched(self):
        return bool((self.raw == FILL).all().item())


def put(a, poison, seed, xor=False):
    """(tensor, device address of the column): ``a`` carved out of poison on the device; with ``xor``
    produced on the current stream by an asynchronous upload from pinned memory and a device XOR."""
    buf, at = wc.embed(a, poison, seed)
    if xor:
        t = torch.from_numpy(buf ^ np.uint8(KEY)).pin_memory().to("cuda", non_blocking=True) ^ KEY
    else:
        t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0 and at % 16 == 0
    return t, t.data_ptr() + at


def scratch(nbytes):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")


def rejected(call):
    """``call`` fails with PZ_EINVAL."""
    with pytest.raises(_lib.PzError) as err:
        call()
    assert err.value.code == _lib.PZ_EINVAL


class Run:
    """One call of an entry point: the columns on the device, the carved outputs, a dirty scratch."""
    ENTRY = STRUCT = None

    def upload(self, cols, poison, seed, xor):
        self.keep, self.struct = [], self.STRUCT()
        for j, (k, a) in enumerate(sorted(cols.items())):
            t, p = put(a, poison, 100 * seed + j, xor)
            self.keep.append(t)
            setattr(self.struct, k, p)

    def launch(self, **over):
        a = dict(self.args, **over)
        _lib.lib.call(self.ENTRY, *[a[k] for k in self.ORDER], _lib.stream_ptr(0))
        return self

    def outputs(self):
        return [c for c in (self.out, self.offs, getattr(self, "tot", None)) if c is not None]

    def untouched(self):
        return all(c.untouched() for c in self.outputs())


class ValRun(Run):
    ENTRY, STRUCT = "pz_dev_wire_validators", _lib.ValidatorCols
    ORDER = ("cols", "n", "field", "out", "offs", "scr", "tot")

    def __init__(self, case, field, with_offs, poison, skew=0, seed=1, xor=False, scr=None, null_out=False):
        dll = _lib.lib.dll
        self.case, self.field = case, field
        self.upload(case.columns(poison, seed), poison, seed, xor)
        self.out = Carve(int(dll.pz_wire_validators_bound(case.n, case.bytes_total())), skew)
        self.offs = Carve(8 * (case.n + 1), 8) if with_offs else None
        self.tot = Carve(8, 8)
        self.scr = scratch(int(dll.pz_wire_scratch_bytes(case.n))) if scr is None else scr
        assert self.scr.numel() >= int(dll.pz_wire_scratch_bytes(case.n))
        self.args = dict(cols=ctypes.byref(self.struct), n=case.n, field=field, out=None if null_out else self.out.ptr,
                         offs=self.offs.ptr if with_offs else None, scr=self.scr.data_ptr(), tot=self.tot.ptr)

    def check(self):
        want, woffs = wc.framed(self.case.records(), self.field)
        self.tot.check(woffs[-1:], "d_total")
        if self.offs is not None:
            self.offs.check(woffs, "d_offsets")
        self.out.check(want, "d_out")


class AttRun(Run):
    ENTRY, STRUCT = "pz_dev_wire_attestations", _lib.AttestationCols
    ORDER = ("cols", "n", "field", "out", "offs", "scr")

    def __init__(self, recs, field, poison, ref=None, shift=False, absent=(), skew=0, seed=1, xor=False, scr=None):
        dll = _lib.lib.dll
        n = len(recs)
        self.ref = wc.att_records(recs, absent) if ref is None else ref
        self.field = field
        cols = wc.att_columns(recs, poison, seed, shift, absent)
        self.upload(cols, poison, seed, xor)
        ne = 0 if wc.OBLIQUE in absent else sum(len(r[wc.OBLIQUE]) for r in recs)
        ns = 0 if wc.SIG in absent else sum(len(r[wc.SIG]) for r in recs)
        self.out = Carve(int(dll.pz_wire_attestations_bound(n, wc.att_bytes_total(recs, absent), ne, ns)), skew)
        self.offs = Carve(8 * (n + 1), 8)
        self.scr = scratch(int(dll.pz_wire_attestations_scratch_bytes(n))) if scr is None else scr
        assert self.scr.numel() >= int(dll.pz_wire_attestations_scratch_bytes(n))
        self.args = dict(cols=ctypes.byref(self.struct), n=n, field=field, out=self.out.ptr, offs=self.offs.ptr,
                         scr=self.scr.data_ptr())

    def check(self):
        want, woffs = wc.framed(self.ref, self.field)
        self.offs.check(woffs, "d_offsets")
        self.out.check(want, "d_out")


def val_both_forms(case, field=11, skew=0):
    """Under both poisons: framed with ``field`` and no d_offsets (the staged path of the scalar
    kernels), framed with d_offsets, and bare with d_offsets (lane by lane)."""
    for poison in wc.POISONS:
        for f, with_offs in ((field, False), (field, True), (0, True)):
            ValRun(case, f, with_offs, poison, skew).launch().check()


# ==== validators ====================================================================================
@pytest.mark.parametrize("which", wc.val_scalar_sets(), ids=lambda s: "+".join(s) or "none")
def test_every_scalar_kernel_past_one_tile(which):
    """Each instantiation (0..5 non-NULL columns; all five sets of four, the path that reloads its
    columns) over two full tiles and a ragged third: the look-back, both sub-tiles, the stage and the
    lane-by-lane path, every varint length at both its ends in every column."""
    val_both_forms(wc.val_scalar_case(which, 2 * wc.VAL_TILE + 77))


@pytest.mark.parametrize("which", (wc.VAL_BYTES[:1], wc.VAL_BYTES[1:], wc.VAL_BYTES), ids="+".join)
@pytest.mark.parametrize("n", (2 * wc.VAL_TILE + 77, 3 * wc.VAL_TILE))
def test_bytes_kernel_past_one_tile(n, which):
    """The bytes-field kernel's look-back (the block-scan window), the carry across its eight
    sub-tiles and the total from a tile other than the first; bytes offsets start at 5."""
    val_both_forms(wc.val_bytes_case(which, n))


@pytest.mark.parametrize("kernel", ("three_columns", "bytes"))
@pytest.mark.parametrize("n", wc.N_EDGES)
def test_n_edges(n, kernel):
    """Record counts at the rows (512), the sub-tiles (2,048) and the tile (4,096)."""
    if kernel == "bytes":
        case = wc.val_bytes_case(wc.VAL_BYTES, n, seed=n + 3)
    else:
        case = wc.val_scalar_case(("balance", "start_dynasty", "end_dynasty"), n, seed=n + 3)
    val_both_forms(case)


@pytest.mark.parametrize("kernel", ("three_columns", "bytes"))
def test_zero_records_touch_no_output_bytes(kernel):
    """n == 0: *d_total == 0, d_offsets[0] == 0 when given, d_out untouched and allowed to be NULL."""
    which = wc.VAL_BYTES if kernel == "bytes" else ()
    case = wc.val_bytes_case(which, 0, scalars=("balance", "start_dynasty", "end_dynasty"))
    for with_offs in (False, True):
        for null_out in (False, True):
            run = ValRun(case, 11, with_offs, 0xFF, null_out=null_out).launch()
            run.check()
            assert run.out.untouched()
            run.tot.check(np.zeros(1, dtype=U64), "d_total")
            if with_offs:
                run.offs.check(np.zeros(1, dtype=U64), "d_offsets")


@pytest.mark.parametrize("r", range(16))
def test_tile_base_and_pointer_alignment(r):
    """Tile 1's output offset is r mod 16 and d_out's address 0, 1, 4, 7, 8 or 15 mod 16: the staged
    store derives its 16-byte alignment from the offset, so an unaligned d_out leaves every dwordx4
    store unaligned.  For r in 1, 3, 14, 15 also a last tile of one 2-byte record (shorter than,
    equal to and longer than the bytes up to the next 16-byte boundary)."""
    cases = [wc.val_base_case(r)] + ([wc.val_base_case(r, single_last=True)] if r in (1, 3, 14, 15) else [])
    for case in cases:
        for skew in OUT_SKEWS:
            for poison in wc.POISONS:
                ValRun(case, 11, False, poison, skew).launch().check()


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_stage_limit(delta):
    """Tiles of exactly 65,535 / 65,536 (staged) and 65,537 bytes (lane by lane), two each, so the
    second tile's base is that number."""
    case = wc.val_stage_case(delta)
    for poison in wc.POISONS:
        for skew in (0, 7):
            ValRun(case, 11, False, poison, skew).launch().check()
    ValRun(case, 11, True, wc.RANDOM).launch().check()


def test_maximum_records():
    """61-byte records: 31,232 bytes per row of 512, the largest value of the four 16-bit row sums
    that travel in one u64."""
    val_both_forms(wc.val_max_case(), field=(1 << 29) - 1)


@pytest.mark.parametrize("field_num", wc.FIELD_NUMS)
def test_field_numbers(field_num):
    val_both_forms(wc.val_scalar_case(("balance", "start_dynasty", "end_dynasty"), wc.VAL_TILE + 77, seed=9), field=field_num)


def test_scratch_reuse_back_to_back():
    """Two calls on one stream over one scratch buffer, nothing waited for between them; the second
    has another n and another kernel.  Both reset the scratch themselves."""
    first = wc.val_scalar_case(("balance", "end_dynasty"), 3 * wc.VAL_TILE + 5, seed=4)
    second = wc.val_bytes_case(wc.VAL_BYTES, wc.VAL_TILE + 9, seed=5)
    scr = scratch(int(_lib.lib.dll.pz_wire_scratch_bytes(first.n)))
    for a, b in ((first, second), (second, first)):
        ra = ValRun(a, 11, False, 0xFF, scr=scr)
        rb = ValRun(b, 11, True, wc.RANDOM, scr=scr)
        ra.launch()
        rb.launch()
        rb.check()
        ra.check()


def test_callers_stream():
    """On a non-default stream the columns are produced right before the call (an asynchronous upload
    from pinned memory and a device XOR); the results are read back on that stream, with no
    device-wide synchronise."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert _lib.stream_ptr(0).value == s.cuda_stream != torch.cuda.default_stream().cuda_stream
        for case in (wc.val_scalar_case(("balance", "start_dynasty", "end_dynasty"), 2 * wc.VAL_TILE + 77, seed=6),
                     wc.val_bytes_case(wc.VAL_BYTES, wc.VAL_TILE + 77, seed=7)):
            for with_offs in (False, True):
                ValRun(case, 11, with_offs, wc.RANDOM, xor=True).launch().check()


def test_argument_checks():
    """PZ_EINVAL before any launch; every output tensor stays untouched."""
    case = wc.val_bytes_case(wc.VAL_BYTES[:1], 100)
    run = ValRun(case, 11, True, 0xFF)
    no_data = _lib.ValidatorCols()
    ctypes.memmove(ctypes.byref(no_data), ctypes.byref(run.struct), ctypes.sizeof(no_data))
    no_data.withdrawal_address = None
    for over in (dict(cols=None), dict(field=1 << 29), dict(cols=ctypes.byref(no_data)), dict(scr=None), dict(tot=None),
                 dict(out=None)):
        rejected(lambda: run.launch(**over))
        assert run.untouched(), over
    run.launch().check()


# ==== attestations ==================================================================================
@pytest.fixture(scope="module")
def grid():
    recs = wc.att_grid_records()
    return recs, wc.att_records(recs)


@pytest.fixture(scope="module")
def varints():
    recs = wc.att_varint_records()
    return recs, wc.att_records(recs)


@pytest.fixture(scope="module")
def mixed():
    recs = wc.att_mixed_records()
    return recs, wc.att_records(recs)


@pytest.mark.parametrize("poison", wc.POISONS, ids=str)
@pytest.mark.parametrize("field_num", (0, 1))
def test_segment_grid(grid, field_num, poison):
    """Every (length 0..80, source address mod 16) pair of each bytes field and of an oblique
    element: the copier's four regimes by length on the row path, the whole-wave path from 65 bytes
    on, and records at every output offset mod 16 on both."""
    recs, ref = grid
    AttRun(recs, field_num, poison, ref).launch().check()


@pytest.mark.parametrize("poison", wc.POISONS, ids=str)
@pytest.mark.parametrize("field_num", (0, 1))
def test_varint_edges_in_every_sub_lane(varints, field_num, poison):
    """Both ends of every varint length as signature values in every sub-lane of a row (the 8-, 4-,
    2- and 1-byte pieces) and in the three scalars; packed bodies and records of 127 / 128 bytes on
    the row path, records of 16,383 / 16,384 bytes on the whole-wave path."""
    recs, ref = varints
    AttRun(recs, field_num, poison, ref).launch().check()


@pytest.mark.parametrize("field_num", (0, 1))
def test_element_and_value_counts(field_num):
    """0, 1, 12, 13, 14 elements x 0, 4, 5, 16, 17 values: the sizing kernel's 12 elements and 4
    values in flight, the row path's 13 and 16; empty elements come out as ``3a 00``."""
    recs = wc.att_count_records()
    ref = wc.att_records(recs)
    assert any(b"\x3a\x00" * 14 in r for r in ref)
    for poison in wc.POISONS:
        AttRun(recs, field_num, poison, ref).launch().check()


@pytest.mark.parametrize("n", (0,) + wc.ATT_N_EDGES)
def test_att_n_edges(n):
    """Record counts at the row (4 per wave), the block (16) and the sizing tile (4,096, where whole
    rows of 512 threads fall past n), both paths in the last, partial wave."""
    recs = wc.att_n_edge_records(n)
    ref = wc.att_records(recs)
    for poison in wc.POISONS:
        for field_num in (0, 1):
            AttRun(recs, field_num, poison, ref).launch().check()


ABSENT = tuple((k,) for k in wc.ATT_FIELDS) + (wc.ATT_FIELDS,)


@pytest.mark.parametrize("absent", ABSENT, ids=lambda a: a[0] if len(a) == 1 else "all")
@pytest.mark.parametrize("field_num", (0, 1))
def test_null_columns(mixed, field_num, absent):
    """NULL = 0 everywhere / none: each field absent on its own, and all of them."""
    recs, _ = mixed
    for poison in wc.POISONS:
        run = AttRun(recs, field_num, poison, absent=absent).launch()
        run.check()
        if len(absent) > 1:
            want = b"\x0a\x00" * len(recs) if field_num else b""
            step = 2 if field_num else 0
            run.out.check(want, "d_out")
            run.offs.check(np.arange(len(recs) + 1, dtype=U64) * U64(step), "d_offsets")
            assert field_num or run.out.untouched()


@pytest.mark.parametrize("field_num", (0, 1))
def test_ranges_that_do_not_start_at_zero(mixed, field_num):
    """The form the pool's views use: bytes offsets from 5, elements from 2 (their bytes from 7),
    values from 3, poison before them."""
    recs, ref = mixed
    for poison in wc.POISONS:
        AttRun(recs, field_num, poison, ref, shift=True).launch().check()


@pytest.mark.parametrize("skew", range(16))
def test_att_pointer_alignment(mixed, skew):
    recs, ref = mixed
    for poison, field_num in zip(wc.POISONS, (0, 1)):
        AttRun(recs, field_num, poison, ref, skew=skew).launch().check()


def test_att_scratch_reuse_back_to_back(varints):
    """Two calls on one stream over one scratch buffer, nothing waited for between them, with
    different record counts (three sizing tiles, then one)."""
    big = wc.att_n_edge_records(2 * 4096 + 5)
    big_ref = wc.att_records(big)
    scr = scratch(int(_lib.lib.dll.pz_wire_attestations_scratch_bytes(len(big))))
    small, small_ref = varints
    for order in (0, 1):
        runs = [AttRun(big, 1, 0xFF, big_ref, scr=scr), AttRun(small, 0, wc.RANDOM, small_ref, scr=scr)][::1 - 2 * order]
        for run in runs:
            run.launch()
        for run in reversed(runs):
            run.check()


def test_att_callers_stream(mixed):
    recs, ref = mixed
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert _lib.stream_ptr(0).value == s.cuda_stream != torch.cuda.default_stream().cuda_stream
        for field_num in (0, 1):
            AttRun(recs, field_num, wc.RANDOM, ref, xor=True).launch().check()
            AttRun(recs, field_num, wc.RANDOM, ref, shift=True, xor=True).launch().check()


def test_att_argument_checks(mixed):
    """PZ_EINVAL before any launch; d_out and d_offsets stay untouched."""
    recs, ref = mixed
    run = AttRun(recs, 1, 0xFF, ref)

    def without(*names):
        c = _lib.AttestationCols()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(run.struct), ctypes.sizeof(c))
        for k in names:
            setattr(c, k, None)
        return ctypes.byref(c)

    for over in (dict(offs=None), dict(scr=None), dict(out=None), dict(cols=without("oblique_offs")),
                 dict(cols=without("aggregate_sig")), dict(cols=without("shard_block_hash")), dict(field=1 << 29),
                 dict(cols=None)):
        rejected(lambda: run.launch(**over))
        assert run.untouched(), list(over)
    run.launch().check()
