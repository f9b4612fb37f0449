"""The two states' case list (tests/state_wire_cases.py) delivers what it claims, and every case's
expected bytes from prysm_amd/wire.py are the protobuf runtime's over oracle/schema.py: the GPU tests
that compare against them are pinned to the reference's schema, not to our own encoder.  No GPU."""
import numpy as np
import pytest

import state_wire_cases as sc
from oracle import schema as opb
from prysm_amd import wire
from test_wire import o_cstate

TABLES = {c.name: c for c in sc.table_cases()}
HEADS = {c.name: c for c in sc.head_cases()}
RECENTS = {c.name: c for c in sc.recent_cases()}


def vlen(x):
    return len(wire.varint(x))


@pytest.mark.parametrize("name", list(TABLES))
def test_table_bytes_are_the_runtimes(name):
    case = TABLES[name]
    o = opb.CrystallizedState()
    for arr in case.pb():
        oa = o.shard_and_committees_for_slots.add()
        for e in arr.array_shard_and_committee:
            oa.array_shard_and_committee.add(shard_id=e.shard_id, committee=e.committee.tolist())
    assert case.expected == o.SerializeToString()
    cols = case.columns()
    assert int(cols["arr_offs"][-1]) == case.nentries == len(cols["arr_comm"]) == len(cols["arr_shard"])
    assert int(cols["coffs"][-1]) == len(cols["members"])
    assert wire.committee_table(case.pb())["arr_offs"].tolist() == cols["arr_offs"].tolist()


@pytest.mark.parametrize("name", list(HEADS))
def test_head_bytes_are_the_runtimes(name):
    case = HEADS[name]
    assert case.expected == o_cstate(case.state()).SerializeToString()
    assert all(len(r.blockhash) <= case.stride for r in case.records)


@pytest.mark.parametrize("name", list(RECENTS))
def test_recent_bytes_are_the_runtimes(name):
    case = RECENTS[name]
    assert case.expected == opb.ActiveState(recent_block_hashes=case.hashes()).SerializeToString()
    assert len(case.expected) == sum(2 + len(h) for h in case.hashes())


def test_tables_cover_the_sizes_members_and_shards():
    sizes = TABLES["sizes"]
    assert [len(c) for c in sizes.comms] == list(sc.SIZES) and len(sizes.arrays) == len(sc.SIZES)
    assert {127, 128, 16384} <= set(sc.SIZES) and all(int(c.max(initial=0)) < 128 for c in sizes.comms)  # packed length = size
    assert vlen(127) == 1 and vlen(128) == 2 == vlen(16383) and vlen(16384) == 3
    assert max(sc.SIZES) > 64 * sc.CHUNK  # one committee of many chunks
    assert len(TABLES["sizes_one_array"].arrays) == 1
    edges = TABLES["member_edges"]
    assert set(sc.MEMBER_EDGES) <= set(np.concatenate(edges.comms).tolist())
    for k in range(1, 6):
        assert {vlen(v) for v in sc.MEMBER_EDGES[2 * k - 2:2 * k]} == {k}
    assert any(len(c) > sc.CHUNK for c in edges.comms)
    shards = TABLES["shards"]
    assert {(s, n) for s in sc.SHARDS for n in (0, 3)} == {(s, len(shards.comms[c])) for a in shards.arrays for s, c in a}
    assert b"\x0a\x00" in shards.expected


def test_entry_and_array_lengths_sit_at_the_limits():
    bodies = [len(wire.shard_and_committee(e)) for a in TABLES["entry_lengths"].pb() for e in a.array_shard_and_committee]
    assert bodies == [127, 128, 16383, 16384]
    framed = [len(wire.shard_and_committee_array(a)) for a in TABLES["entry_framed"].pb()]  # one entry an array
    assert framed == [127, 128, 16383, 16384] and all(len(a) == 1 for a in TABLES["entry_framed"].arrays)
    bodies = [len(wire.shard_and_committee_array(a)) for a in TABLES["array_bodies"].pb()]
    assert bodies == [127, 128, 16383, 16384]


def test_shapes_of_the_table_list():
    assert TABLES["narr0"].expected == b"" and TABLES["narr1_no_entries"].expected == b"\x62\x00"
    assert TABLES["narr1_empty_entry"].expected == b"\x62\x02\x0a\x00"
    assert TABLES["empty_arrays"].expected.startswith(b"\x62\x00\x62") and TABLES["empty_arrays"].expected.endswith(b"\x62\x00\x62\x00")
    assert len(TABLES["narr128"].arrays) == 128 and [] in TABLES["narr128"].arrays
    shared = TABLES["shared"].columns()["arr_comm"].tolist()
    assert len(shared) > len(set(shared))
    gen = TABLES["genesis_1024"]
    assert len(gen.arrays) >= 128 and gen.members_total >= 2 * 1024 and gen.members_total % 1024 == 0


def test_heads_cover_the_scalars_seeds_records_and_hash_lengths():
    for j in range(8):
        assert {c.values[j] for c in HEADS.values()} >= {0, 1, sc.M64}
    assert {len(c.seed) for c in HEADS.values()} >= {0, 32, 64}
    assert {len(c.records) for c in HEADS.values()} >= {0, 1, 1024}
    assert {len(r.blockhash) for r in HEADS["hash_lengths_32"].records} >= {0, 1, 31, 32} and HEADS["hash_lengths_32"].stride == 32
    assert {len(r.blockhash) for r in HEADS["hash_lengths_48"].records} >= {33, 48} and HEADS["hash_lengths_48"].stride == 48
    assert HEADS["zero_records"].expected == b"\x52\x00" * 5 and HEADS["all_0"].expected == b""
    assert b"\x52\x00" in HEADS["records_1024"].expected


def test_recents_cover_the_genesis_state():
    assert RECENTS["genesis_128_empty"].expected == b"\x12\x00" * 128
    assert RECENTS["full_128"].expected[:2] == b"\x12\x20" and len(RECENTS["full_128"].expected) == 128 * 34
    assert set(RECENTS["mixed"].lens.tolist()) >= {0, 1, 31, 32}
