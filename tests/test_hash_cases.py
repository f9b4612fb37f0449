"""The BLAKE2b case builders (tests/hash_cases.py) deliver what they claim, and their expected
digests agree with the project's two other CPU hashers.  No GPU."""
import numpy as np
import pytest

import hash_cases as hc
from oracle import cport, ref

FIXED_PAIRS = ((16, 0), (16, 1), (16, 16), (112, 100), (128, 127), (128, 128), (144, 129), (256, 129),
               (384, 272), (512, 500), (512, 512), (528, 512), (640, 513))


def span_sets(poison):
    sets = dict(hc.span_shapes(3, poison))
    sets["align_grid"] = hc.align_grid(poison=poison)
    data, offs = hc.packed([length for length, _ in hc.grid_pairs()], 5, 7, poison)
    sets["packed"] = (data, offs[:-1], offs[1:])
    return sets


def test_grid_holds_every_pair_once():
    data, begs, ends = hc.align_grid()
    assert len(begs) == 316 * 12 == 3792
    got = sorted(zip((ends - begs).tolist(), (begs % np.uint64(128)).tolist()))
    assert got == sorted((length, res) for length in hc.GRID_LENGTHS for res in hc.GRID_RESIDUES)
    assert len(set(got)) == 3792
    assert (begs[1:] >= ends[:-1]).all() and (begs[1:] - ends[:-1] < 128).all()  # only the gaps the residues require


def test_grid_waves_mix_block_counts():
    _, begs, ends = hc.align_grid()
    lens = (ends - begs).astype(np.int64)
    blocks = np.maximum(1, (lens + 127) // 128)
    assert blocks.min() == 1 and blocks.max() == 33
    for w in range(4):
        assert len(set(blocks[64 * w:64 * w + 64].tolist())) >= 4, w


@pytest.mark.parametrize("poison", hc.POISONS)
def test_four_byte_rule_and_poison_cover(poison):
    """No message ends within 4 bytes of its buffer's end (every builder leaves 16), and every byte
    outside the messages is the poison while the bytes inside do not depend on it."""
    other = span_sets(0x00)
    for name, (data, begs, ends) in span_sets(poison).items():
        assert (ends >= begs).all(), name
        assert len(data) >= int(ends.max()) + 16, name
        m = hc.covered(len(data), begs, ends)
        seed = {"align_grid": hc.GRID_SEED, "packed": 5}.get(name, 3)
        assert np.array_equal(data[~m], hc.poison_bytes(len(data), poison, seed)[~m]), name
        assert np.array_equal(data[m], other[name][0][m]) and not other[name][0][~m].any(), name
        assert (~m).sum() >= 16, name


def test_shapes_are_what_they_say():
    s = hc.span_shapes(3)
    _, b, e = s["sliding"]
    assert len(b) == 321 and ((e - b) == 200).all() and (np.diff(b.astype(np.int64)) == 1).all()
    _, b, e = s["repeated"]
    assert len(b) == 130 and len(set(b.tolist())) == 1 and ((e - b) == 300).all()
    _, b, e = s["nested"]
    assert len(b) == 501 and (b + e == 1000).all() and b[500] == e[500]
    _, b, e = s["descending"]
    assert len(b) == 3792 and (np.diff(b.astype(np.int64)) <= 0).all()
    _, b, e = s["empties"]
    assert ((e - b)[0::2] == 0).all() and ((e - b)[1::2] == 129).all()
    assert set(b[0::2].tolist()) == {0, 1, 127, 128, int(e.max())}
    _, b, e = s["gappy"]
    assert set((e - b).tolist()) == {1, 2, 3, 4, 5} and (b[1:] - e[:-1] == 4096).all()


def test_packed_is_csr_with_a_lead():
    data, offs = hc.packed([0, 3, 128, 0, 5], 1, 7, 0xEE)
    assert offs.tolist() == [7, 7, 10, 138, 138, 143] and len(data) == 143 + 16
    assert (data[:7] == 0xEE).all() and (data[143:] == 0xEE).all()


@pytest.mark.parametrize("poison", hc.POISONS)
def test_fixed_records_layout(poison):
    for stride, length in FIXED_PAIRS:
        for n in (1, 65, 300):
            data = hc.fixed_records(n, stride, length, 9, poison)
            assert len(data) % 128 == 0 and n * stride <= len(data) < n * stride + 128
            assert len(data) >= hc.fixed_readable(n, stride, length)
            m = hc.covered(len(data), *hc.fixed_spans(n, stride, length))
            assert m.sum() == n * length
            assert np.array_equal(data[~m], hc.poison_bytes(len(data), poison, 9)[~m])
            assert np.array_equal(data[m], hc.fixed_records(n, stride, length, 9, 0)[m])


def test_want_agrees_with_ref_sum512():
    for name, (data, begs, ends) in span_sets(hc.RANDOM).items():
        w = hc.want(data, begs, ends, 64)
        raw = data.tobytes()
        step = max(1, len(begs) // 97)
        for i in list(range(0, len(begs), step)) + [len(begs) - 1]:
            assert w[i].tobytes() == ref.sum512(raw[int(begs[i]):int(ends[i])]), (name, i)
        assert np.array_equal(hc.want(data, begs, ends, 32), w[:, :32]), name


def test_want_agrees_with_the_c_port_on_strided_sets():
    for stride, length in FIXED_PAIRS:
        n = 65
        data = hc.fixed_records(n, stride, length, 4, hc.RANDOM)
        for ob in (32, 64):
            got = cport.hash_fixed(data[:n * stride].reshape(n, stride), length, ob)
            assert np.array_equal(got, hc.want(data, *hc.fixed_spans(n, stride, length), ob)), (stride, length, ob)
