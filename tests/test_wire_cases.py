"""The proto3 encoders' case builders (tests/wire_cases.py) deliver what they claim, and their
framing agrees with the protobuf runtime's own repeated fields.  No GPU."""
import numpy as np
import pytest

import wire_cases as wc
from oracle import schema as opb

U64 = np.uint64


def test_edges_are_both_ends_of_every_varint_length():
    assert len(wc.EDGES) == 20 and len(set(wc.EDGES)) == 20
    for k in range(1, 11):
        lo, hi = wc.EDGES[2 * k - 2], wc.EDGES[2 * k - 1]
        assert len(wc.varint(lo)) == len(wc.varint(hi)) == k == wc.vlen(lo) == wc.vlen(hi)
        assert lo == 1 or len(wc.varint(lo - 1)) == k - 1
        assert hi == (1 << 64) - 1 or len(wc.varint(hi + 1)) == k + 1


def test_framing_is_the_runtimes_repeated_field():
    """``framed`` with field 11 / field 1 is what the runtime emits for CrystallizedState.validators /
    ActiveState.pending_attestations."""
    case = wc.val_bytes_case(wc.VAL_BYTES, 300)
    state = opb.CrystallizedState()
    for r in case.records():
        state.validators.add().ParseFromString(r)
    raw, offs = wc.framed(case.records(), 11)
    assert raw == state.SerializeToString() and int(offs[-1]) == len(raw) and offs[0] == 0
    recs = wc.att_count_records()
    active = opb.ActiveState()
    for r in wc.att_records(recs):
        active.pending_attestations.add().ParseFromString(r)
    assert wc.framed(wc.att_records(recs), 1)[0] == active.SerializeToString()
    bare, offs = wc.framed(wc.att_records(recs), 0)
    assert bare == b"".join(wc.att_records(recs)) and np.array_equal(np.diff(offs), [len(r) for r in wc.att_records(recs)])


def test_embed_and_bytes_column_surround_with_poison():
    for poison in wc.POISONS:
        buf, at = wc.embed(np.arange(5, dtype=U64), poison, 3)
        assert at == wc.PAD and len(buf) == 40 + 2 * wc.PAD and at % 16 == 0
        want = wc.poison_bytes(len(buf), poison, 3)
        assert np.array_equal(buf[:at], want[:at]) and np.array_equal(buf[at + 40:], want[at + 40:])
        assert buf[at:at + 40].view(U64).tolist() == [0, 1, 2, 3, 4]
        data, offs = wc.bytes_column([b"ab", b"", b"cde"], 5, poison, 9)
        assert offs.tolist() == [5, 7, 7, 10] and len(data) == 10 + wc.TAIL and data[5:10].tobytes() == b"abcde"
        want = wc.poison_bytes(len(data), poison, 9)
        assert np.array_equal(data[:5], want[:5]) and np.array_equal(data[10:], want[10:])


# ---- validators ----------------------------------------------------------------------------------
def test_scalar_sets_cover_every_kernel():
    sets = wc.val_scalar_sets()
    assert sorted(set(len(s) for s in sets)) == [0, 1, 2, 3, 4, 5]
    assert len(set(s for s in sets if len(s) == 4)) == 5
    for s in sets:
        assert list(s) == [c for c in wc.VAL_SCALARS if c in s]  # field order


def test_every_scalar_column_holds_every_edge():
    case = wc.val_scalar_case(wc.VAL_SCALARS, 2 * wc.VAL_TILE + 77)
    for k, col in case.scalars.items():
        assert set(wc.EDGES) | {0} <= set(col.tolist()), k
    assert len(case.records()) == 2 * wc.VAL_TILE + 77


def test_bytes_case_lengths_lead_and_poison():
    for which in (wc.VAL_BYTES[:1], wc.VAL_BYTES[1:], wc.VAL_BYTES):
        case = wc.val_bytes_case(which, 2 * wc.VAL_TILE + 77)
        assert set(case.scalars) < set(wc.VAL_SCALARS)  # partly NULL
        for poison in wc.POISONS:
            cols = case.columns(poison, 11)
            for j, k in enumerate(sorted(which)):
                data, offs = cols[k], cols[k + "_offs"]
                assert offs[0] == wc.BYTES_LEAD == 5 and len(data) == int(offs[-1]) + wc.TAIL
                assert set(np.diff(offs).tolist()) == set(wc.BYTES_LENGTHS)
                want = wc.poison_bytes(len(data), poison, 11 + j)
                assert np.array_equal(data[:5], want[:5]) and np.array_equal(data[int(offs[-1]):], want[int(offs[-1]):])
                assert data[5:int(offs[-1])].tobytes() == b"".join(case.blobs[k])


@pytest.mark.parametrize("r", range(16))
def test_base_case_puts_tile_1_at_r(r):
    case = wc.val_base_case(r)
    assert case.n == wc.VAL_TILE + 77 and set(case.scalars) == {"balance", "start_dynasty", "end_dynasty"}
    _, offs = wc.framed(case.records(), 11)
    assert int(offs[wc.VAL_TILE]) % 16 == r and int(offs[wc.VAL_TILE]) <= wc.STAGE_BYTES
    single = wc.val_base_case(r, single_last=True)
    raw, offs = wc.framed(single.records(), 11)
    assert single.n == wc.VAL_TILE + 1 and int(offs[wc.VAL_TILE]) % 16 == r and raw[int(offs[wc.VAL_TILE]):] == b"\x5a\x00"


def test_stage_cases_sit_at_the_limit():
    for delta in (-1, 0, 1):
        case = wc.val_stage_case(delta)
        _, offs = wc.framed(case.records(), 11)
        assert case.n == 2 * wc.VAL_TILE
        assert int(offs[wc.VAL_TILE]) == wc.STAGE_BYTES + delta == 65536 + delta
        assert int(offs[2 * wc.VAL_TILE] - offs[wc.VAL_TILE]) == 65536 + delta
    sizes = np.diff(wc.framed(wc.val_stage_case(0).records(), 11)[1])
    assert (sizes == 16).all()


def test_max_case_fills_the_packed_row_sums():
    case = wc.val_max_case()
    _, offs = wc.framed(case.records(), (1 << 29) - 1)
    sizes = np.diff(offs)
    assert case.n == wc.VAL_TILE + 600 and (sizes == 61).all() and int(sizes[:512].sum()) == 31232 < 1 << 16


# ---- attestations --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    recs = wc.att_grid_records()
    return recs, wc.att_columns(recs, 0xFF, 1), wc.att_records(recs)


def test_grid_holds_every_pair_for_every_kind(grid):
    """All 81 x 16 (length, source address mod 16) pairs per kind, and every pair of at most 64
    bytes in a record the row path writes."""
    recs, cols, ref = grid
    row = [wc.on_row_path(r, len(b)) for r, b in zip(recs, ref)]
    every = {(length, res) for length in range(81) for res in range(16)}
    assert len(every) == 81 * 16 == 1296
    for kind in wc.SEG_KINDS:
        pairs = wc.segment_pairs(cols, kind)
        assert every <= set(pairs), kind
        if kind == wc.OBLIQUE:
            owner = [i for i, r in enumerate(recs) for _ in r[wc.OBLIQUE]]
        else:
            owner = list(range(len(recs)))
        assert len(owner) == len(pairs)
        on_row = {p for p, i in zip(pairs, owner) if row[i]}
        assert {p for p in every if p[0] <= wc.ROW_SEG} <= on_row, kind
        assert {p for p, i in zip(pairs, owner) if not row[i]} >= {p for p in every if p[0] > wc.ROW_SEG}, kind
    assert len(recs) < 6000


@pytest.mark.parametrize("field_num", (0, 1))
def test_grid_output_offsets_take_every_residue_on_both_paths(grid, field_num):
    recs, _, ref = grid
    _, offs = wc.framed(ref, field_num)
    sizes = np.diff(offs).tolist()
    row = np.array([wc.on_row_path(r, s) for r, s in zip(recs, sizes)])
    res = (offs[:-1] % U64(16)).astype(int)
    assert set(res[row].tolist()) == set(range(16)) == set(res[~row].tolist())


def test_varint_records_put_every_edge_in_every_sub_lane():
    recs = wc.att_varint_records()
    ref = wc.att_records(recs)
    seen = {(v, j) for r, b in zip(recs, ref) if wc.on_row_path(r, len(b) + 3) for j, v in enumerate(r[wc.SIG])}
    assert {(v, j) for v in wc.EDGES for j in range(16)} <= seen
    assert {len(r[wc.SIG]) for r in recs} >= set(wc.SIG_COUNTS)
    for k in wc.ATT_SCALARS:
        assert set(wc.EDGES) <= {r[k] for r in recs}, k
    # the length-prefix limits: packed bodies of 127 / 128 bytes, records of 127 / 128 and 16,383 / 16,384
    packed = {sum(wc.vlen(v) for v in r[wc.SIG]): r for r in recs if len(r[wc.SIG]) in (15, 16) and r["slot"] == 1}
    assert {127, 128} <= set(packed) and all(wc.on_row_path(packed[s], s + 5) for s in (127, 128))
    by_size = {len(b): r for r, b in zip(recs, ref)}
    for size in (127, 128):
        assert wc.on_row_path(by_size[size], size + 3)
    for size in (16383, 16384):
        assert not wc.on_row_path(by_size[size], size + 4)
    assert len(wc.varint(127)) == 1 and len(wc.varint(128)) == 2 == len(wc.varint(16383)) and len(wc.varint(16384)) == 3


def test_count_records_cross_elements_and_values():
    recs = wc.att_count_records()
    for size in (0, 32):
        got = {(len(r[wc.OBLIQUE]), len(r[wc.SIG])) for r in recs if all(len(e) == size for e in r[wc.OBLIQUE])}
        assert {(e, s) for e in wc.COUNT_ELEMS for s in wc.COUNT_SIGS} <= got
    r = next(r for r in recs if len(r[wc.OBLIQUE]) == 12 and not r[wc.OBLIQUE][0])
    assert b"\x3a\x00" * 12 in wc.att_records([r])[0]
    paths = {wc.on_row_path(r, len(b)) for r, b in zip(recs, wc.att_records(recs))}
    assert paths == {True, False}


@pytest.mark.parametrize("n", wc.ATT_N_EDGES)
def test_n_edge_records_end_on_both_paths(n):
    recs = wc.att_n_edge_records(n)
    assert len(recs) == n
    if n >= 3:
        last = recs[4 * ((n - 1) // 4):] if n % 4 != 1 else recs[-5:]
        sizes = [len(b) for b in wc.att_records(last)]
        assert {wc.on_row_path(r, s) for r, s in zip(last, sizes)} == {True, False}
        assert wc.on_row_path(recs[-2], 60) and not wc.on_row_path(recs[-1], 160)


def test_shifted_columns_start_nowhere_at_zero():
    recs = wc.att_count_records()
    for poison in wc.POISONS:
        cols = wc.att_columns(recs, poison, 21, shift=True)
        plain = wc.att_columns(recs, poison, 21)
        for j, k in enumerate(wc.ATT_BYTES):
            assert cols[k + "_offs"][0] == 5 and np.array_equal(cols[k][:5], wc.poison_bytes(5, poison, 21 + j))
            assert np.array_equal(cols[k + "_offs"] - U64(5), plain[k + "_offs"])
        assert cols["oblique_first"][0] == 2 and cols["oblique_offs"][2] == 7
        assert np.array_equal(cols[wc.OBLIQUE][:7], wc.poison_bytes(7, poison, 24))
        assert (cols["oblique_offs"][:2] != 7).all() and (cols["oblique_offs"][:2] <= len(cols[wc.OBLIQUE])).all()
        assert cols["aggregate_sig_first"][0] == 3
        assert np.array_equal(cols[wc.SIG][:3], wc.poison_bytes(32, poison, 25).view(U64)[:3])
        assert np.array_equal(cols[wc.SIG][3:-1], plain[wc.SIG][:-1])
        assert len(cols["oblique_offs"]) == int(cols["oblique_first"][-1]) + 1
    absent = wc.att_columns(recs, 0xFF, 1, absent=(wc.OBLIQUE, "slot"))
    assert not {"slot", wc.OBLIQUE, "oblique_offs", "oblique_first"} & set(absent)
    assert wc.att_records(recs[:3], absent=wc.ATT_FIELDS) == [b"", b"", b""]
