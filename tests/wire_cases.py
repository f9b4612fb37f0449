"""Case builders and the reference for the proto3 encoders' device entry points,
pz_dev_wire_validators and pz_dev_wire_attestations (plain numpy; no GPU, no torch).

The reference is Google's protobuf runtime over oracle/schema.py, record by record
(``SerializeToString``); the framing is a plain varint of ``(field_num << 3) | 2`` and of the
record's length.  prysm_amd/wire.py is not consulted.

Every column a builder returns is meant to be carved out of *poison* (``embed``): a constant 0xFF
or a seeded random stream lies before and behind it, and inside a bytes column before the first
offset and behind the last.  A kernel that reads outside the ranges its offsets name then encodes a
wrong byte, whatever it would have read from a zero-filled or freshly allocated buffer.  Offsets
that no record names are in range but wrong: a kernel that used one would copy the wrong bytes, not
fault.
"""
import numpy as np

from oracle import schema as opb

U64 = np.uint64
RANDOM = "random"
POISONS = (0xFF, RANDOM)
TAIL = 16   # poison bytes behind the last range of a bytes column
PAD = 64    # poison bytes before and behind every embedded column (keeps 16-byte alignment)

# both ends of every varint length 1..10: 2^(7k-7) and 2^(7k) - 1 (the last capped at 2^64 - 1)
EDGES = tuple(v for k in range(1, 11) for v in (1 << (7 * k - 7), min((1 << (7 * k)) - 1, (1 << 64) - 1)))


def varint(x):
    out = bytearray()
    while x >= 0x80:
        out.append((x & 0x7F) | 0x80)
        x >>= 7
    out.append(x)
    return bytes(out)


def vlen(x):
    return max(1, (int(x).bit_length() + 6) // 7)


def poison_bytes(size, poison, seed):
    """``size`` poison bytes: the constant ``poison``, or for ``RANDOM`` a stream seeded by ``seed``."""
    if poison == RANDOM:
        return np.random.default_rng([seed, 0x9015]).integers(0, 256, size=size, dtype=np.uint8)
    return np.full(size, poison, dtype=np.uint8)


def embed(a, poison, seed):
    """(buffer, offset): the bytes of array ``a`` at ``offset`` of a poison buffer, PAD poison bytes
    before and behind them."""
    raw = np.ascontiguousarray(a).view(np.uint8).ravel()
    buf = poison_bytes(PAD + len(raw) + PAD, poison, seed)
    buf[PAD:PAD + len(raw)] = raw
    return buf, PAD


def bytes_column(blobs, lead, poison, seed):
    """(data, offsets), the CSR form of ``blobs``: offsets[0] == lead, ``lead`` poison bytes in front
    and TAIL behind."""
    offs = np.full(len(blobs) + 1, lead, dtype=U64)
    if blobs:
        offs[1:] += np.cumsum([len(b) for b in blobs], dtype=U64)
    data = poison_bytes(int(offs[-1]) + TAIL, poison, seed)
    if int(offs[-1]) > lead:
        data[lead:int(offs[-1])] = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    return data, offs


def framed(records, field_num):
    """(bytes, offsets[n+1]): the records back to back, each framed as length-delimited field
    ``field_num`` (0: bare)."""
    if field_num:
        tag = varint((field_num << 3) | 2)
        records = [tag + varint(len(r)) + r for r in records]
    offs = np.zeros(len(records) + 1, dtype=U64)
    if records:
        offs[1:] = np.cumsum([len(r) for r in records], dtype=U64)
    return b"".join(records), offs


# ---- validators ----------------------------------------------------------------------------------
VAL_SCALARS = ("public_key", "withdrawal_shard", "balance", "start_dynasty", "end_dynasty")
VAL_BYTES = ("withdrawal_address", "randao_commitment")
VAL_TILE = 4096
BYTES_LENGTHS = (0, 1, 20, 32, 127, 128, 300)
BYTES_LEAD = 5
N_EDGES = (0, 1, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097)
FIELD_NUMS = (1, 15, 16, 2047, 2048, (1 << 29) - 1)
STAGE_BYTES = 65536


class ValCase:
    """``n`` validator records as columns: ``scalars`` maps a field to its u64 column, ``blobs`` a
    bytes field to its list of values; a field in neither is a NULL column."""

    def __init__(self, n, scalars, blobs=None):
        self.n, self.scalars, self.blobs = n, dict(scalars), dict(blobs or {})
        assert all(len(c) == n and c.dtype == U64 for c in self.scalars.values())
        assert all(len(b) == n for b in self.blobs.values())
        self._records = None

    def records(self):
        """The reference: the protobuf runtime's bytes of every record."""
        if self._records is None:
            cols = {k: c.tolist() for k, c in self.scalars.items()}
            cols.update(self.blobs)
            self._records = [opb.ValidatorRecord(**{k: c[i] for k, c in cols.items()}).SerializeToString()
                             for i in range(self.n)]
        return self._records

    def columns(self, poison, seed):
        """name -> array: the scalar columns, and data + ``_offs`` of every bytes column (offsets
        start at BYTES_LEAD)."""
        cols = dict(self.scalars)
        for j, (k, b) in enumerate(sorted(self.blobs.items())):
            cols[k], cols[k + "_offs"] = bytes_column(b, BYTES_LEAD, poison, seed + j)
        return cols

    def bytes_total(self):
        return sum(len(x) for b in self.blobs.values() for x in b)


def edge_column(n, seed, rot=0):
    """A u64 column of edge values, zeros and random magnitudes; its first 21 entries are every
    edge value and 0, rotated by ``rot``."""
    rng = np.random.default_rng([seed, 0xC01])
    vals = np.array(EDGES + (0,), dtype=U64)
    col = vals[rng.integers(0, len(vals), size=n)]
    wild = (rng.integers(0, 1 << 63, size=n, dtype=U64) * U64(2) + U64(1)) >> rng.integers(0, 64, size=n).astype(U64)
    col = np.where(rng.random(n) < 0.3, wild, col).astype(U64)
    k = min(n, len(vals))
    col[:k] = np.roll(vals, rot)[:k]
    return col


def val_scalar_sets():
    """Sets of non-NULL scalar columns: one of each size 0..5, and all five of size 4."""
    sets = [(), ("balance",), ("public_key", "end_dynasty"), ("balance", "start_dynasty", "end_dynasty")]
    sets += [tuple(c for c in VAL_SCALARS if c != drop) for drop in VAL_SCALARS]
    return sets + [VAL_SCALARS]


def val_scalar_case(which, n, seed=1):
    return ValCase(n, {k: edge_column(n, seed * 16 + j, 3 * j) for j, k in enumerate(which)})


def val_bytes_case(which, n, seed=2, scalars=("public_key", "balance")):
    """Bytes columns ``which`` with lengths from BYTES_LENGTHS (the first seven records hold each
    length), scalar columns partly NULL."""
    rng = np.random.default_rng([seed, 0xB17E])
    blobs = {}
    for j, k in enumerate(which):
        lens = rng.choice(BYTES_LENGTHS, size=n)
        m = min(n, len(BYTES_LENGTHS))
        lens[:m] = np.roll(BYTES_LENGTHS, j)[:m]
        blobs[k] = [rng.integers(0, 256, size=int(x), dtype=np.uint8).tobytes() for x in lens]
    return ValCase(n, {k: edge_column(n, seed * 16 + j, 5 * j) for j, k in enumerate(scalars)}, blobs)


def val_base_case(r, single_last=False):
    """Field 11 over (balance, start_dynasty, end_dynasty): tile 0 is 4,095 records of 4 bytes
    (``5a 02 28 20``) and one of 4 + r, so tile 1 starts at an offset that is r mod 16.  Tile 1 is
    77 records of edge values, or with ``single_last`` one all-zero record (``5a 00``)."""
    n = VAL_TILE + (1 if single_last else 77)
    cols = {k: np.zeros(n, dtype=U64) for k in ("balance", "start_dynasty", "end_dynasty")}
    cols["balance"][:VAL_TILE] = 32
    lb, ls = next((lb, ls) for lb in range(1, 11) for ls in range(0, 11)
                  if 2 + 1 + lb + (1 + ls if ls else 0) == 4 + r)
    cols["balance"][0] = 1 << (7 * lb - 7) if lb > 1 else 32
    cols["start_dynasty"][0] = 1 << (7 * ls - 7) if ls else 0
    if not single_last:
        for j, k in enumerate(cols):
            cols[k][VAL_TILE:] = edge_column(77, 40 + j, 7 * j)
    return ValCase(n, cols)


def val_stage_case(delta):
    """Two tiles of 4,096 16-byte records under field 11 (balance 2^28, start 2^14, end 2^14: body
    14, frame 2); with delta = +1 / -1 one record of each tile has start 2^21 / 2^7, so each tile
    encodes to 65,536 + delta bytes."""
    n = 2 * VAL_TILE
    cols = {"balance": np.full(n, 1 << 28, dtype=U64), "start_dynasty": np.full(n, 1 << 14, dtype=U64),
            "end_dynasty": np.full(n, 1 << 14, dtype=U64)}
    if delta:
        cols["start_dynasty"][[1234, VAL_TILE + 2345]] = {1: 1 << 21, -1: 1 << 7}[delta]
    return ValCase(n, cols)


def val_max_case():
    """All five columns at 2^64 - 1: with field (1 << 29) - 1, 61 bytes per record."""
    n = VAL_TILE + 600
    return ValCase(n, {k: np.full(n, (1 << 64) - 1, dtype=U64) for k in VAL_SCALARS})


# ---- attestations --------------------------------------------------------------------------------
ATT_SCALARS = ("slot", "shard_id", "justified_slot")
ATT_BYTES = ("justified_block_hash", "shard_block_hash", "attester_bitfield")
OBLIQUE, SIG = "oblique_parent_hashes", "aggregate_sig"
ATT_FIELDS = ATT_SCALARS + ATT_BYTES + (OBLIQUE, SIG)
SEG_KINDS = ATT_BYTES + (OBLIQUE,)
SEG_LENGTHS = tuple(range(81))
ROW_BYTES, ROW_ELEMS, ROW_SIGS, ROW_SEG = 768, 13, 16, 64  # the row path's limits (wire_att.hip)
ATT_N_EDGES = (1, 3, 4, 5, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 5)
SIG_COUNTS = (1, 4, 5, 16, 17, 64, 65, 130)
COUNT_ELEMS, COUNT_SIGS = (0, 1, 12, 13, 14), (0, 4, 5, 16, 17)


def att(**kw):
    """One record: every field, zero / empty unless given."""
    rec = {k: 0 for k in ATT_SCALARS}
    rec.update({k: b"" for k in ATT_BYTES})
    rec.update({OBLIQUE: [], SIG: []})
    assert set(kw) <= set(rec)
    rec.update(kw)
    return rec


def att_records(recs, absent=()):
    """The reference: the protobuf runtime's bytes of every record, the fields in ``absent`` left out."""
    return [opb.AttestationRecord(**{k: v for k, v in r.items() if k not in absent}).SerializeToString() for r in recs]


def on_row_path(rec, size):
    """Whether wire_att.hip writes this record (of ``size`` encoded bytes, frame included) by a
    16-lane row; otherwise the whole wave writes it."""
    segs = [len(rec[k]) for k in ATT_BYTES] + [len(e) for e in rec[OBLIQUE]]
    return size <= ROW_BYTES and len(rec[OBLIQUE]) <= ROW_ELEMS and len(rec[SIG]) <= ROW_SIGS and max(segs) <= ROW_SEG


def att_columns(recs, poison, seed, shift=False, absent=()):
    """name -> array, the fields in ``absent`` missing (NULL columns).  With ``shift`` no range starts
    at 0, as in the views of the pending pool: every bytes offsets column starts at 5,
    oblique_first at 2 with oblique_offs[2] == 7, aggregate_sig_first at 3; what lies before is poison
    (bytes and values) or in range and wrong (the two element offsets no record names)."""
    cols = {k: np.array([r[k] for r in recs], dtype=U64) for k in ATT_SCALARS if k not in absent}
    for j, k in enumerate(ATT_BYTES):
        if k not in absent:
            cols[k], cols[k + "_offs"] = bytes_column([r[k] for r in recs], 5 if shift else 0, poison, seed + j)
    if OBLIQUE not in absent:
        skip, lead = (2, 7) if shift else (0, 0)
        data, offs = bytes_column([e for r in recs for e in r[OBLIQUE]], lead, poison, seed + 3)
        first = np.full(len(recs) + 1, skip, dtype=U64)
        first[1:] += np.cumsum([len(r[OBLIQUE]) for r in recs], dtype=U64)
        cols[OBLIQUE], cols["oblique_first"] = data, first
        cols["oblique_offs"] = np.concatenate([offs[-1] - np.arange(skip, dtype=U64), offs])
    if SIG not in absent:
        skip = 3 if shift else 0
        vals = np.array([v for r in recs for v in r[SIG]], dtype=U64)
        first = np.full(len(recs) + 1, skip, dtype=U64)
        first[1:] += np.cumsum([len(r[SIG]) for r in recs], dtype=U64)
        pad = poison_bytes(8 * (skip + 1), poison, seed + 4).view(U64)  # (values no record names: before, one behind)
        cols[SIG], cols["aggregate_sig_first"] = np.concatenate([pad[:skip], vals, pad[skip:]]), first
    return cols


def att_bytes_total(recs, absent=()):
    return sum(len(r[k]) for r in recs for k in ATT_BYTES if k not in absent) + (
        0 if OBLIQUE in absent else sum(len(e) for r in recs for e in r[OBLIQUE]))


def grid_sequence(start, seed):
    """Segment lengths in an order such that, laid back to back from an address that is ``start``
    mod 16, every (length 0..80, start address mod 16) pair occurs; a few pairs occur twice where
    the walk has to move on to a residue with pairs left."""
    rng = np.random.default_rng([seed, 0x691D])
    left = {c: set(SEG_LENGTHS) for c in range(16)}
    seq, c, remaining = [], start % 16, 16 * len(SEG_LENGTHS)
    while remaining:
        if left[c]:
            pool = sorted(left[c])
            keys = rng.random(len(pool))
            length = max(zip(pool, keys), key=lambda p: (len(left[(c + p[0]) % 16]), p[1]))[0]
            left[c].discard(length)
            remaining -= 1
        else:
            length = max(range(1, 16), key=lambda x: len(left[(c + x) % 16]))
        seq.append(length)
        c = (c + length) % 16
    return seq


_SHORT = (0, 1, 7, 32, 16, 3, 64, 15)


def att_grid_records(seed=3):
    """Four runs of records, one per segment kind (the three bytes fields, an oblique element): in
    its run a kind's segments walk ``grid_sequence`` -- in the oblique run one to four elements per
    record, all at most 64 bytes or all longer -- while the other segments stay short, so a record
    is on the row path exactly when its grid segments are at most 64 bytes."""
    rng = np.random.default_rng([seed, 0x5E6])
    blob = lambda n: rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()  # noqa: E731
    recs, used = [], {k: 0 for k in SEG_KINDS}
    for kind in SEG_KINDS:
        seq = grid_sequence(used[kind], seed + len(recs))
        groups, at, g = [], 0, 0
        while at < len(seq):
            want = 1 if kind != OBLIQUE else (1, 2, 3, 4)[g % 4]
            take = 1
            while take < want and at + take < len(seq) and (seq[at + take] > ROW_SEG) == (seq[at] > ROW_SEG):
                take += 1
            groups.append(seq[at:at + take])
            at, g = at + take, g + 1
        for j, group in enumerate(groups):
            r = att(slot=EDGES[j % 20], shard_id=j % 3, justified_slot=EDGES[(j + 9) % 20] if j % 5 else 0,
                    aggregate_sig=[EDGES[(j + v) % 20] for v in range(j % 3)])
            for q, k in enumerate(ATT_BYTES):
                r[k] = blob(group[0] if k == kind else _SHORT[(j + 3 * q) % len(_SHORT)])
            r[OBLIQUE] = [blob(x) for x in group] if kind == OBLIQUE else [blob(5)] * (j % 2)
            for k in ATT_BYTES:
                used[k] += len(r[k])
            used[OBLIQUE] += sum(len(e) for e in r[OBLIQUE])
            recs.append(r)
    return recs


def segment_pairs(cols, kind):
    """[(length, start mod 16)] of every segment of ``kind`` in ``cols``, in record order (the start is
    the offset: the data column's address is 16-byte aligned)."""
    offs = cols["oblique_offs" if kind == OBLIQUE else kind + "_offs"]
    return list(zip((offs[1:] - offs[:-1]).tolist(), (offs[:-1] % U64(16)).tolist()))


def att_varint_records(seed=5):
    """The edge values as signature values in records of 1, 4, 5, 16, 17, 64, 65 and 130 values --
    twenty 16-value records rotate them, so every value sits in every sub-lane of a row -- and in
    slot, shard_id and justified_slot; then the length-prefix limits: packed bodies of 127 and 128
    bytes (15 x 8 + 7 and 16 x 8) and records of 127 and 128 bytes on the row path, records of 16,383
    and 16,384 bytes (a long bitfield) on the whole-wave path."""
    rng = np.random.default_rng([seed, 0x7A1])
    blob = lambda n: rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()  # noqa: E731
    recs = []
    for count in SIG_COUNTS:
        for rot in range(20 if count == 16 else 5 if count < 16 else 2):
            k = len(recs)
            recs.append(att(slot=EDGES[k % 20], shard_id=EDGES[(k + 7) % 20], justified_slot=EDGES[(k + 13) % 20],
                            shard_block_hash=blob(k % 33),
                            aggregate_sig=[EDGES[(rot * (1 if count == 16 else 7) + j) % 20] for j in range(count)]))
    v8, v7 = 1 << 49, 1 << 42
    recs.append(att(slot=1, aggregate_sig=[v8] * 15 + [v7]))
    recs.append(att(slot=1, aggregate_sig=[v8] * 16))
    for bits in (55, 56):  # 2 + 34 + 34 + 2 + bits = 127, 128
        recs.append(att(slot=1, justified_block_hash=blob(32), shard_block_hash=blob(32), attester_bitfield=blob(bits)))
    for bits in (16380, 16381):  # 1 + 2 + bits = 16,383, 16,384
        recs.append(att(attester_bitfield=blob(bits)))
    return recs


def att_count_records(seed=7):
    """0, 1, 12, 13 and 14 elements crossed with 0, 4, 5, 16 and 17 values, the elements all empty
    or all 32 bytes."""
    rng = np.random.default_rng([seed, 0xC07])
    blob = lambda n: rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()  # noqa: E731
    recs = []
    for size in (0, 32):
        for ne in COUNT_ELEMS:
            for ns in COUNT_SIGS:
                k = len(recs)
                recs.append(att(slot=k + 1, shard_id=EDGES[k % 20], justified_block_hash=blob(32 * (k % 2)),
                                attester_bitfield=blob(k % 9), oblique_parent_hashes=[blob(size) for _ in range(ne)],
                                aggregate_sig=[EDGES[(k + j) % 20] for j in range(ns)]))
    return recs


def att_mixed_records():
    """The count and varint records interleaved: both paths in most waves."""
    a, b = att_count_records(), att_varint_records()
    return [r for pair in zip(a, b) for r in pair] + a[len(b):] + b[len(a):]


_POOL = []


def att_n_edge_records(n):
    """``n`` records drawn from the grid and the varint records; from n = 3 on the last two are one of
    the row path and one of the whole-wave path, so both sit in the last, partial wave."""
    if not _POOL:
        grid, var = att_grid_records(), att_varint_records()
        _POOL.extend(grid[k] if k % 8 else var[(k // 8) % len(var)] for k in range(len(grid)))
    recs = [_POOL[(k * 7) % len(_POOL)] for k in range(n)]
    if n >= 3:
        recs[-2] = att(slot=3, shard_block_hash=bytes(range(33)), aggregate_sig=list(EDGES[:9]))
        recs[-1] = att(slot=4, attester_bitfield=bytes(range(70)), aggregate_sig=list(EDGES[5:]))
    return recs
