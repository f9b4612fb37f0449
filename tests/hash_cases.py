"""Case builders for the BLAKE2b device entry points (plain numpy; no GPU, no torch).

Every builder returns host arrays: a byte buffer and the spans of the messages in it.  Bytes that
belong to a message are random; every other byte of the buffer, and at least 16 bytes after the
highest message end, is *poison*: a constant byte, or a seeded random stream (``poison="random"``).
A kernel that lets a neighbour's byte or the padding into a digest then computes a wrong digest,
whatever it would have read from a zero-filled buffer.

The rule every builder follows: no message ends closer than 4 bytes to the end of its buffer (the
CSR contract of include/prysm_hip.h), and no fixed-record buffer is shorter than the header's
readable-bytes formula (``fixed_readable``).  Over-reads are detected by changing the bytes outside
a message, never by placing a message where an over-read would fault.
"""
import hashlib

import numpy as np

GRID_LENGTHS = list(range(0, 301)) + [383, 384, 385, 511, 512, 513, 639, 640, 641, 1023, 1024, 1025,
                                      4095, 4096, 4097]
GRID_RESIDUES = (0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 127)  # start address mod 128
GRID_SEED = 2   # the first four waves of this order each mix >= 6 block counts (test_hash_cases.py)
TAIL = 16       # poison bytes after the highest message end
RANDOM = "random"
POISONS = (0xFF, RANDOM)


def poison_bytes(size, poison, seed):
    """``size`` poison bytes: the constant ``poison``, or for ``RANDOM`` a stream seeded by ``seed``."""
    if poison == RANDOM:
        return np.random.default_rng([seed, 0x9015]).integers(0, 256, size=size, dtype=np.uint8)
    return np.full(size, poison, dtype=np.uint8)


def covered(size, begs, ends):
    """Boolean mask of the bytes of [0, size) that lie in at least one span."""
    d = np.zeros(size + 1, dtype=np.int64)
    np.add.at(d, np.asarray(begs, dtype=np.int64), 1)
    np.add.at(d, np.asarray(ends, dtype=np.int64), -1)
    return np.cumsum(d)[:size] > 0


def materialize(begs, ends, seed, poison, size=None):
    """A buffer of ``size`` bytes (default: the highest end + TAIL): random message bytes inside the
    spans, poison everywhere else."""
    begs = np.asarray(begs, dtype=np.uint64)
    ends = np.asarray(ends, dtype=np.uint64)
    top = int(ends.max()) if len(ends) else 0
    size = top + TAIL if size is None else size
    assert size >= top + 4
    data = poison_bytes(size, poison, seed)
    msg = np.random.default_rng([seed, 0xDA7A]).integers(0, 256, size=size, dtype=np.uint8)
    m = covered(size, begs, ends)
    data[m] = msg[m]
    return data, begs, ends


def place(pairs, cursor=0):
    """Spans for (length, residue) pairs in order: each message starts at the first address at or
    after the previous end whose value mod 128 is its residue."""
    begs, ends = [], []
    for length, res in pairs:
        beg = cursor + (res - cursor) % 128
        begs.append(beg)
        cursor = beg + length
        ends.append(cursor)
    return begs, ends


def grid_pairs(seed=GRID_SEED):
    """Every (length, start residue) pair of the grid once, in an order shuffled by ``seed``."""
    pairs = [(length, res) for length in GRID_LENGTHS for res in GRID_RESIDUES]
    order = np.random.default_rng([seed, 0x0DE2]).permutation(len(pairs))
    return [pairs[k] for k in order]


def align_grid(seed=GRID_SEED, poison=0xFF):
    """(data, begs, ends): one message per (length, start mod 128) pair, 316 x 12 = 3,792 in all, in
    shuffled order (a wave of 64 lanes mixes block counts from 1 to 33), separated by the gaps the
    residues require."""
    return materialize(*place(grid_pairs(seed)), seed, poison)


def packed(lengths, seed, lead, poison=0xFF):
    """(data, offsets), the CSR form: contiguous messages, offsets[0] == lead, ``lead`` poison bytes in
    front and TAIL behind."""
    offsets = np.full(len(lengths) + 1, lead, dtype=np.uint64)
    offsets[1:] += np.cumsum(np.asarray(lengths, dtype=np.uint64))
    data, _, _ = materialize(offsets[:-1], offsets[1:], seed, poison, size=int(offsets[-1]) + TAIL)
    return data, offsets


def span_shapes(seed, poison=0xFF):
    """Named (data, begs, ends) sets whose spans overlap, repeat, nest, descend, are empty or lie far
    apart."""
    shapes = {}
    shapes["sliding"] = ([i for i in range(321)], [i + 200 for i in range(321)])
    shapes["repeated"] = ([37] * 130, [337] * 130)
    shapes["nested"] = ([k for k in range(501)], [1000 - k for k in range(501)])
    gb, ge = place(grid_pairs(seed))
    order = np.argsort(np.asarray(gb), kind="stable")[::-1]
    shapes["descending"] = ([gb[k] for k in order], [ge[k] for k in order])
    # 129-byte spans at shifting alignments; between them empty spans at 0, 1, 127, 128 and the top
    full = [(5 + 133 * j + rep, 5 + 133 * j + rep + 129) for rep in range(13) for j in range(5)]
    top = max(e for _, e in full)
    b, e = [], []
    for k, (fb, fe) in enumerate(full):
        at = (0, 1, 127, 128, top)[k % 5]
        b += [at, fb]
        e += [at, fe]
    shapes["empties"] = (b, e)
    b, e, cur = [], [], 0
    for i in range(200):
        b.append(cur)
        e.append(cur + 1 + i % 5)
        cur = e[-1] + 4096
    shapes["gappy"] = (b, e)
    return {name: materialize(bb, ee, seed, poison) for name, (bb, ee) in shapes.items()}


def fixed_readable(n, stride, length):
    """The bytes include/prysm_hip.h says pz_dev_blake2b512_fixed may read."""
    if n == 0 or length == 0:
        return 0
    whole = 128 * ((length + 127) // 128)
    return (n - 1) * stride + (whole if stride >= whole else 16 * ((length + 15) // 16))


def fixed_spans(n, stride, length):
    begs = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    return begs, begs + np.uint64(length)


def fixed_records(n, stride, length, seed, poison=0xFF):
    """Record i at i * stride: ``length`` random bytes, then poison up to the stride; the buffer is
    n * stride rounded up to 128 bytes (the round-up is poison too)."""
    assert stride >= length
    size = (n * stride + 127) // 128 * 128
    assert size >= fixed_readable(n, stride, length)
    data = poison_bytes(size, poison, seed)
    if length:
        rec = data[:n * stride].reshape(n, stride)
        rec[:, :length] = np.random.default_rng([seed, 0xDA7A]).integers(0, 256, size=(n, length), dtype=np.uint8)
    return data


def want(data, begs, ends, out_bytes):
    """The hashlib (RFC 7693) digests of data[begs[i]:ends[i]] as an (n, out_bytes) array."""
    raw = data.tobytes()
    dig = b"".join(hashlib.blake2b(raw[int(b):int(e)], digest_size=64).digest()[:out_bytes]
                   for b, e in zip(begs, ends))
    return np.frombuffer(dig, dtype=np.uint8).reshape(len(begs), out_bytes)
