"""The three device-resident BLAKE2b entry points (pz_dev_blake2b512_spans / _batch / _fixed)
against hashlib (RFC 7693), bit-exact, at the edges the kernels' addressing depends on: every
(start alignment, length) pair, waves whose lanes have different block counts, spans that overlap,
repeat, descend, are empty or lie more than 4 GiB apart, every fixed-record route and mask, the
persistent kernel's walk to a second group, and the stride limit.

Every buffer comes from tests/hash_cases.py: the bytes outside the messages are poison (a constant
0xFF, or a random stream), so a byte that leaks into a digest changes it.  Every output is carved
out of a larger 0xA5-filled tensor whose guard bytes are checked after the call."""
import numpy as np
import pytest
import torch

import hash_cases as hc
from prysm_amd import _lib

pytestmark = pytest.mark.gpu

OUT_BYTES = (32, 64)
GUARD = 64
FILL = 0xA5
PREFIXES = (1, 63, 64, 65, 255, 256, 257, 3792)
FIXED_PAIRS = ((16, 0), (16, 1), (16, 16), (112, 100), (128, 127), (128, 128), (144, 129), (256, 129),
               (384, 272), (512, 500), (512, 512), (528, 512), (640, 513))
FIXED_NS = (1, 63, 64, 65, 127, 128, 129, 300)
FAR = 2 ** 32
BIG_BYTES = 2 ** 32 + 2 ** 27


def dev(a):
    """A host array on the device (u64 columns travel as their int64 bit pattern)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def guarded(n, out_bytes, launch):
    """Run ``launch(d_out)`` with d_out a 16-byte aligned (and no better: 16 mod 64) carve-out for n
    digests of a larger tensor filled with 0xA5, at least 64 guard bytes on either side; wait for the
    current stream, assert both guards are intact and return the (n, out_bytes) digest area."""
    size = n * out_bytes
    raw = torch.full((size + 2 * GUARD + 64,), FILL, dtype=torch.uint8, device="cuda")
    lo = GUARD + (16 - (raw.data_ptr() + GUARD)) % 64
    assert (raw.data_ptr() + lo) % 64 == 16 and lo + size + GUARD <= raw.numel()
    launch(raw.data_ptr() + lo)
    torch.cuda.current_stream().synchronize()
    host = raw.cpu().numpy()
    assert (host[:lo] == FILL).all(), "bytes in front of d_out were written"
    assert (host[lo + size:] == FILL).all(), "bytes behind d_out were written"
    return host[lo:lo + size].reshape(n, out_bytes)


def run_spans(msgs_ptr, d_begs, d_ends, n, ob):
    return guarded(n, ob, lambda out: _lib.lib.call(
        "pz_dev_blake2b512_spans", msgs_ptr, d_begs.data_ptr(), d_ends.data_ptr(), n, out, ob, _lib.stream_ptr(0)))


def run_batch(msgs_ptr, d_offs, n, ob):
    return guarded(n, ob, lambda out: _lib.lib.call(
        "pz_dev_blake2b512_batch", msgs_ptr, d_offs.data_ptr(), n, out, ob, _lib.stream_ptr(0)))


def run_fixed(msgs_ptr, stride, length, n, ob):
    return guarded(n, ob, lambda out: _lib.lib.call(
        "pz_dev_blake2b512_fixed", msgs_ptr, stride, length, n, out, ob, _lib.stream_ptr(0)))


def check_all_widths(run, want64):
    """``run(ob)`` for out_bytes 32 and 64: every digest equals the reference's first ob bytes."""
    for ob in OUT_BYTES:
        np.testing.assert_array_equal(run(ob), want64[:, :ob], err_msg="out_bytes=%d" % ob)


# ---- CSR kernel through the span form: the alignment grid ------------------------------------
@pytest.fixture(scope="module")
def grid():
    """The alignment grid under both poisons on the device, and its digests (the message bytes, so
    the digests, are the same under either poison)."""
    sets = {}
    for poison in hc.POISONS:
        data, begs, ends = hc.align_grid(poison=poison)
        sets[poison] = (dev(data), dev(begs), dev(ends))
    return sets, hc.want(data, begs, ends, 64)


@pytest.mark.parametrize("poison", hc.POISONS, ids=str)
@pytest.mark.parametrize("n", PREFIXES)
def test_align_grid_through_spans(grid, n, poison):
    """Every (length, start mod 128) pair, lanes of a wave at block counts from 1 to 33, for
    prefixes that end inside, at and just past a wave and a workgroup."""
    sets, want = grid
    d, b, e = sets[poison]
    check_all_widths(lambda ob: run_spans(d.data_ptr(), b, e, n, ob), want[:n])


# ---- CSR, device form --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def packed_sets():
    lengths = [length for length, _ in hc.grid_pairs()]
    sets = {}
    for lead in (0, 7):
        per = {poison: hc.packed(lengths, 11, lead, poison) for poison in hc.POISONS}
        data, offs = per[0xFF]
        sets[lead] = (per, hc.want(data, offs[:-1], offs[1:], 64))
    return sets


@pytest.mark.parametrize("lead", (0, 7))
@pytest.mark.parametrize("shift", (0, 1, 2, 3))
def test_csr_device_form(packed_sets, shift, lead):
    """pz_dev_blake2b512_batch over the grid's lengths packed back to back, d_msgs ``shift`` bytes
    into its allocation and absolute offsets that start at ``lead``."""
    per, want = packed_sets[lead]
    for poison, (data, offs) in per.items():
        buf = torch.full((shift + len(data),), 0x3C, dtype=torch.uint8, device="cuda")
        buf[shift:] = dev(data)
        d_offs = dev(offs)
        assert int(offs[0]) == lead
        check_all_widths(lambda ob: run_batch(buf.data_ptr() + shift, d_offs, len(offs) - 1, ob), want)


# ---- span shapes -------------------------------------------------------------------------------
SHAPES = ("sliding", "repeated", "nested", "descending", "empties", "gappy")


@pytest.fixture(scope="module")
def shapes():
    return {poison: hc.span_shapes(3, poison) for poison in hc.POISONS}


@pytest.mark.parametrize("poison", hc.POISONS, ids=str)
@pytest.mark.parametrize("name", SHAPES)
def test_span_shapes(shapes, name, poison):
    assert set(shapes[poison]) == set(SHAPES)
    data, begs, ends = shapes[poison][name]
    d, b, e = dev(data), dev(begs), dev(ends)
    check_all_widths(lambda ob: run_spans(d.data_ptr(), b, e, len(begs), ob), hc.want(data, begs, ends, 64))


# ---- one allocation of more than 4 GiB ---------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """One uninitialised 4 GiB + 128 MiB tensor for the far-apart spans and the stride limit; freed
    when the module ends."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 2 ** 30:
        pytest.skip("torch.cuda.mem_get_info reports %.2f GiB free, less than the 6 GiB this 4.1 GiB "
                    "allocation is allowed to ask for" % (free / 2 ** 30))
    t = torch.empty(BIG_BYTES, dtype=torch.uint8, device="cuda")
    yield t
    del t
    torch.cuda.empty_cache()


def test_spans_more_than_4gib_apart(big):
    """256 spans of the grid's first lengths and alignments, alternating lane by lane between a
    region at offset 0 and one at 2**32: begs and ends are u64 and no 32-bit offset from a wave's
    base can reach both."""
    pairs = hc.grid_pairs()[:256]
    begs = np.zeros(256, dtype=np.uint64)
    ends = np.zeros(256, dtype=np.uint64)
    want = np.zeros((256, 64), dtype=np.uint8)
    for half, base in ((0, 0), (1, FAR)):
        data, b, e = hc.materialize(*hc.place(pairs[half::2], cursor=16), 40 + half, hc.RANDOM)
        assert base + len(data) <= BIG_BYTES
        big[base:base + len(data)] = dev(data)
        begs[half::2] = b + np.uint64(base)
        ends[half::2] = e + np.uint64(base)
        want[half::2] = hc.want(data, b, e, 64)
    assert int(begs[1::2].min()) - int(ends[0::2].max()) > 2 ** 32 - 2 ** 27
    d_b, d_e = dev(begs), dev(ends)
    check_all_widths(lambda ob: run_spans(big.data_ptr(), d_b, d_e, 256, ob), want)


def test_fixed_at_the_stride_limit(big):
    """The largest stride the entry point accepts: one persistent group (64 x stride just fits 32-bit
    offsets) and a one-record tail on the plain grid."""
    stride, length, n = 2 ** 26 - 16, 272, 65
    rec = hc.fixed_records(n, 384, length, 8, hc.RANDOM)  # each record's three blocks, poison past len
    d_rec = dev(rec)
    assert (n - 1) * stride + 384 <= BIG_BYTES and hc.fixed_readable(n, stride, length) == (n - 1) * stride + 384
    for i in range(n):
        big[i * stride:i * stride + 384] = d_rec[i * 384:(i + 1) * 384]
    want = hc.want(rec, *hc.fixed_spans(n, 384, length), 64)
    check_all_widths(lambda ob: run_fixed(big.data_ptr(), stride, length, n, ob), want)


# ---- fixed-length records ----------------------------------------------------------------------
@pytest.mark.parametrize("stride,length", FIXED_PAIRS + ((128, 0),))
def test_fixed_routes_and_masks(stride, length):
    """Both fixed kernels (the persistent one when the stride holds whole blocks and the batch a full
    wave, the plain grid otherwise and for the tail), a partial last dword, chunk and block, a stride
    tighter and looser than whole blocks and one that is no multiple of 128; batches that are tail
    only, bulk only and bulk plus tail; poison in [len, stride) of every slot.  (16, 0) at n >= 64
    is the case that showed the plain kernel's unmasked fast path taking empty records; (128, 0)
    adds the empty record on a stride of whole blocks."""
    for poison in hc.POISONS:
        for n in FIXED_NS:
            data = hc.fixed_records(n, stride, length, 1000 * stride + length, poison)
            d = dev(data)
            assert d.data_ptr() % 16 == 0
            want = hc.want(data, *hc.fixed_spans(n, stride, length), 64)
            for ob in OUT_BYTES:
                np.testing.assert_array_equal(run_fixed(d.data_ptr(), stride, length, n, ob), want[:, :ob],
                                              err_msg="n=%d poison=%s out_bytes=%d" % (n, poison, ob))


@pytest.mark.parametrize("stride,length", ((128, 128), (384, 272)))
def test_fixed_persistent_walk(stride, length):
    """More groups of 64 records than the persistent grid has waves (W = 4 waves x 4 workgroups x the
    CU count), so the first waves walk on to a second group, g + W, whose first block they prefetch
    while they compress: one block per record (every iteration changes group), and three blocks with
    a partial last one (block-to-block and group-to-group transitions)."""
    W = 16 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * (W + 5) + 37
    data = hc.fixed_records(n, stride, length, 21, hc.RANDOM)
    want = hc.want(data, *hc.fixed_spans(n, stride, length), 64)
    d = dev(data)
    check_all_widths(lambda ob: run_fixed(d.data_ptr(), stride, length, n, ob), want)


# ---- argument checks ---------------------------------------------------------------------------
def rejected(call):
    """``call`` fails with PZ_EINVAL."""
    with pytest.raises(_lib.PzError) as err:
        call()
    assert err.value.code == _lib.PZ_EINVAL


@pytest.fixture(scope="module")
def small():
    """Four 128-byte records, their spans and offsets on the device."""
    data = hc.fixed_records(4, 128, 128, 6, 0xFF)
    b, e = hc.fixed_spans(4, 128, 128)
    return dev(data), dev(b), dev(e), dev(np.arange(5, dtype=np.uint64) * np.uint64(128))


def call_entry(small, entry, n, out, ob, stride=128, length=128, msgs_off=0):
    d, b, e, offs = small
    p, s = d.data_ptr() + msgs_off, _lib.stream_ptr(0)
    if entry == "fixed":
        return _lib.lib.call("pz_dev_blake2b512_fixed", p, stride, length, n, out, ob, s)
    if entry == "batch":
        return _lib.lib.call("pz_dev_blake2b512_batch", p, offs.data_ptr(), n, out, ob, s)
    return _lib.lib.call("pz_dev_blake2b512_spans", p, b.data_ptr(), e.data_ptr(), n, out, ob, s)


@pytest.mark.parametrize("entry", ("fixed", "batch", "spans"))
def test_zero_messages_touch_nothing(small, entry):
    """n == 0 is PZ_OK and writes nothing: the guards and the whole output area stay 0xA5."""
    for ob in OUT_BYTES:
        out = guarded(4, ob, lambda out: call_entry(small, entry, 0, out, ob))
        assert (out == FILL).all()


@pytest.mark.parametrize("entry", ("fixed", "batch", "spans"))
def test_out_bytes_must_be_32_or_64(small, entry):
    for ob in (0, 16, 31, 48, 128):
        for n in (0, 4):
            def call(out, n=n, ob=ob):
                rejected(lambda: call_entry(small, entry, n, out, ob))
            assert (guarded(8, 64, call) == FILL).all()


def test_fixed_rejects_bad_layouts(small):
    """PZ_EINVAL before any launch (the output stays untouched): stride == 2**26, stride % 16 != 0,
    stride < len, d_msgs or d_out not 16-byte aligned."""
    bad = (dict(stride=2 ** 26, length=128), dict(stride=2 ** 26 + 16, length=128), dict(stride=24, length=8),
           dict(stride=136, length=128), dict(stride=16, length=17), dict(stride=112, length=128),
           dict(msgs_off=8), dict(msgs_off=1))
    for kw in bad:
        def call(out, kw=kw):
            rejected(lambda: call_entry(small, "fixed", 1, out, 32, **kw))
        assert (guarded(8, 64, call) == FILL).all(), kw
    for skew in (1, 4, 8):
        def call(out, skew=skew):
            rejected(lambda: call_entry(small, "fixed", 1, out + skew, 32))
        assert (guarded(8, 64, call) == FILL).all(), skew


@pytest.mark.parametrize("entry", ("batch", "spans"))
def test_csr_forms_reject_unaligned_output(small, entry):
    for skew in (1, 4, 8):
        def call(out, skew=skew):
            rejected(lambda: call_entry(small, entry, 1, out + skew, 32))
        assert (guarded(8, 64, call) == FILL).all(), skew


# ---- the caller's stream -----------------------------------------------------------------------
def test_callers_stream():
    """A span set and a fixed set on a non-default stream: the inputs are produced on that stream
    (an asynchronous upload and a device XOR) right before the call, with no device-wide synchronise;
    the digests are right once that stream has synchronised."""
    s = torch.cuda.Stream()
    data, begs, ends = hc.span_shapes(3, hc.RANDOM)["sliding"]
    n, stride, length = 64 * 40 + 9, 384, 272
    rec = hc.fixed_records(n, stride, length, 13, hc.RANDOM)
    key = np.uint8(0x5A)
    h_data, h_rec = torch.from_numpy(data ^ key).pin_memory(), torch.from_numpy(rec ^ key).pin_memory()
    h_b, h_e = torch.from_numpy(begs.view(np.int64)).pin_memory(), torch.from_numpy(ends.view(np.int64)).pin_memory()
    want_spans = hc.want(data, begs, ends, 64)
    want_rec = hc.want(rec, *hc.fixed_spans(n, stride, length), 64)
    with torch.cuda.stream(s):
        assert _lib.stream_ptr(0).value == s.cuda_stream != torch.cuda.default_stream().cuda_stream
        for ob in OUT_BYTES:
            d = h_data.to("cuda", non_blocking=True) ^ 0x5A
            b, e = h_b.to("cuda", non_blocking=True), h_e.to("cuda", non_blocking=True)
            np.testing.assert_array_equal(run_spans(d.data_ptr(), b, e, len(begs), ob), want_spans[:, :ob])
            r = h_rec.to("cuda", non_blocking=True) ^ 0x5A
            np.testing.assert_array_equal(run_fixed(r.data_ptr(), stride, length, n, ob), want_rec[:, :ob])
