"""The case list of the two states' device encoders (prysm_amd/csrc/wire_state.hip): committee tables
for ShardAndCommitteesForSlots, heads (the CrystallizedState's fields 1-10) and recent-hash lists (the
ActiveState's field 2), each with its expected bytes from prysm_amd/wire.py.
tests/test_state_wire_cases.py pins those bytes to the protobuf runtime over oracle/schema.py;
tests/test_state_wire_gpu.py runs the device and host forms against them;
prysm_amd/csrc/tests/wire_state_san.cpp restates the list in C.  No GPU here."""
import functools

import numpy as np

from prysm_amd import pb, wire

U64 = np.uint64
M64 = (1 << 64) - 1
CHUNK = 256  # kWsChunk: the members a workgroup sizes and writes

SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4097, 16384, 70001)
MEMBER_EDGES = (0, 127, 128, 16383, 16384, 2097151, 2097152, 268435455, 268435456, (1 << 32) - 1)
SHARDS = (0, 1, 127, 128, M64)


def small(n, first=0):
    """n members of one byte each."""
    return ((np.arange(n, dtype=np.int64) + first) % 128).astype(np.uint32)


class TableCase:
    """``arrays``: per array a list of ``(shard_id, committee id)``; ``comms``: the committees."""

    def __init__(self, name, arrays, comms):
        self.name, self.arrays = name, [list(a) for a in arrays]
        self.comms = [np.ascontiguousarray(c, dtype=np.uint32) for c in comms]

    @property
    def nentries(self):
        return sum(len(a) for a in self.arrays)

    @property
    def members_total(self):
        return sum(len(self.comms[c]) for a in self.arrays for _, c in a)

    def columns(self):
        """The columns of pz_committee_table (``wire.TABLE_COLS``)."""
        entries = [e for a in self.arrays for e in a]
        arr_offs = np.zeros(len(self.arrays) + 1, dtype=U64)
        arr_offs[1:] = np.cumsum([len(a) for a in self.arrays], dtype=U64)
        coffs = np.zeros(len(self.comms) + 1, dtype=U64)
        coffs[1:] = np.cumsum([len(c) for c in self.comms], dtype=U64)
        return {"arr_offs": arr_offs, "arr_shard": np.array([e[0] for e in entries], dtype=U64),
                "arr_comm": np.array([e[1] for e in entries], dtype=np.uint32), "coffs": coffs,
                "members": np.concatenate(self.comms + [np.zeros(0, np.uint32)]).astype(np.uint32)}

    def pb(self):
        return [pb.ShardAndCommitteeArray([pb.ShardAndCommittee(s, self.comms[c]) for s, c in a]) for a in self.arrays]

    @functools.cached_property
    def expected(self):
        """Field 12 as wire.crystallized_state emits it (every other field absent)."""
        return wire.crystallized_state(pb.CrystallizedState(shard_and_committees_for_slots=self.pb()))


def _one_each(name, shards_and_comms, per_array=1):
    """Entry k has shard shards_and_comms[k][0] and its own committee; per_array entries an array."""
    ents = [(s, k) for k, (s, _) in enumerate(shards_and_comms)]
    arrays = [ents[i:i + per_array] for i in range(0, len(ents), per_array)]
    return TableCase(name, arrays, [c for _, c in shards_and_comms])


@functools.lru_cache(None)
def table_cases():
    rng = np.random.default_rng(12)
    cases = [
        # every committee size, an array each and all in one array: the packed length's 1 -> 2 and 2 -> 3
        # byte limits with one-byte members, and one committee of many chunks
        _one_each("sizes", [(5, small(n, n)) for n in SIZES]),
        _one_each("sizes_one_array", [(k, small(n)) for k, n in enumerate(SIZES)], per_array=len(SIZES)),
        # every varint limit of a member: alone, and through a committee of two chunks
        _one_each("member_edges", [(3, np.array([v], np.uint32)) for v in MEMBER_EDGES] +
                  [(4, np.array(MEMBER_EDGES * 30, np.uint32)), (0, np.array(MEMBER_EDGES[::-1] * 26, np.uint32))], per_array=4),
        _one_each("shards", [(s, small(n)) for s in SHARDS for n in (0, 3)], per_array=3),
        # ShardAndCommittee bodies of 127 / 128 and 16,383 / 16,384 bytes (shard 0, one-byte members)
        _one_each("entry_lengths", [(0, small(n)) for n in (125, 126, 16380, 16381)]),
        # single entries whose framed length (0a, length, body) is 127 / 128 and 16,383 / 16,384 bytes
        _one_each("entry_framed", [(0, small(n)) for n in (123, 124, 16377, 16378)]),
        # array bodies of 127 / 128 and 16,383 / 16,384 bytes
        TableCase("array_bodies", [[(0, 0)], [(0, 1), (0, 2)], [(0, 3)], [(0, 4)]],
                  [small(123), small(122), small(0), small(16377), small(16378)]),
        TableCase("empty_arrays", [[], [(1, 0)], [], []], [small(2)]),
        TableCase("narr0", [], []),
        TableCase("narr1_no_entries", [[]], []),
        TableCase("narr1_empty_entry", [[(0, 0)]], [small(0)]),
        TableCase("narr128", [[(int(rng.integers(0, 1024)), (3 * a + j) % 40) for j in range(a % 3)] for a in range(128)],
                  [rng.integers(0, 1 << 22, size=int(rng.integers(0, 300)), dtype=np.uint32) for _ in range(40)]),
        # entries that share one committee id, as the engine's tables do
        TableCase("shared", [[(7, 0), (8, 0)], [(9, 1), (7, 0), (0, 1)]], [small(300), small(1)]),
    ]
    from oracle import ref
    _, cs = ref.new_genesis_states(1024)
    tab = [[(sc.shard_id, np.array(list(sc.committee), np.uint32)) for sc in arr.array_shard_and_committee]
           for arr in cs.shard_and_committees_for_slots]
    ents = [e for arr in tab for e in arr]
    ids = iter(range(len(ents)))
    cases.append(TableCase("genesis_1024", [[(s, next(ids)) for s, _ in arr] for arr in tab], [c for _, c in ents]))
    return cases


# ---- heads -----------------------------------------------------------------------------------------
HEAD_SCALARS = ("last_state_recalc", "justified_streak", "last_justified_slot", "last_finalized_slot", "current_dynasty",
                "total_deposits")  # pz_recalc_state's, in PZ_RS_* order
HEAD_REST = ("crosslinking_start_shard", "dynasty_seed_last_reset")


class HeadCase:
    def __init__(self, name, values, seed, records, stride=32):
        """``values``: the eight scalars (HEAD_SCALARS then HEAD_REST)."""
        self.name, self.values, self.seed, self.records, self.stride = name, tuple(values), bytes(seed), list(records), stride

    def state(self):
        kw = dict(zip(HEAD_SCALARS + HEAD_REST, self.values))
        return pb.CrystallizedState(dynasty_seed=self.seed, crosslink_records=self.records, **kw)

    @functools.cached_property
    def expected(self):
        return wire.crystallized_state(self.state())


@functools.lru_cache(None)
def head_cases():
    rng = np.random.default_rng(13)
    rec = lambda n: pb.CrosslinkRecord(int(rng.integers(0, 1 << 63)), rng.bytes(n), int(rng.integers(0, 1 << 40)))  # noqa: E731
    cases = [HeadCase("all_%d" % k, [v] * 8, b"", []) for k, v in enumerate((0, 1, M64))]
    cases += [HeadCase("only_%d" % k, [M64 if j == k else 0 for j in range(8)], b"", []) for k in range(8)]
    cases += [HeadCase("seed_%d" % n, [1, 0, M64, 0, 1, M64, 0, 1], rng.bytes(n), [rec(32)]) for n in (0, 32, 64)]
    cases.append(HeadCase("one_record", [64, 1, 0, 0, 1, 32768, 0, 0], b"", [rec(32)]))
    cases.append(HeadCase("zero_records", [0] * 8, b"", [pb.CrosslinkRecord(0, b"", 0)] * 5))
    cases.append(HeadCase("hash_lengths_32", [128, 2, 64, 0, 1, 1 << 40, 9, 0], rng.bytes(32),
                          [rec(n) for n in (0, 1, 31, 32)] + [pb.CrosslinkRecord(0, rng.bytes(32), 0), pb.CrosslinkRecord(M64, b"", M64)]))
    cases.append(HeadCase("hash_lengths_48", [128, 2, 64, 0, 1, 1 << 40, 0, 7], b"", [rec(n) for n in (33, 48, 0, 32)], stride=48))
    cases.append(HeadCase("records_1024", [M64, 3, 5, 1, 0, 77, 1023, 0], rng.bytes(64),
                          [pb.CrosslinkRecord(s % 3, bytes([s & 255]) * (s % 33), (s % 5) << (s % 50)) for s in range(1024)]))
    return cases


# ---- recent block hashes ----------------------------------------------------------------------------
class RecentCase:
    def __init__(self, name, rows, lens):
        """``rows``: (n, 32) uint8, BytesToHash-normalised; ``lens``: per row, or None (all 32)."""
        self.name, self.rows, self.lens = name, np.ascontiguousarray(rows, np.uint8).reshape(-1, 32), lens

    def hashes(self):
        lens = [32] * len(self.rows) if self.lens is None else self.lens
        return [self.rows[i, 32 - int(n):].tobytes() for i, n in enumerate(lens)]

    @functools.cached_property
    def expected(self):
        return wire.active_state(pb.ActiveState(recent_block_hashes=self.hashes()))


@functools.lru_cache(None)
def recent_cases():
    rng = np.random.default_rng(14)
    rows = lambda n: rng.integers(0, 256, size=(n, 32), dtype=np.uint8)  # noqa: E731
    return [RecentCase("none", rows(0), None), RecentCase("one", rows(1), None), RecentCase("full_128", rows(128), None),
            RecentCase("genesis_128_empty", np.zeros((128, 32), np.uint8), np.zeros(128, np.uint8)),
            RecentCase("mixed", rows(8), np.array([0, 1, 31, 32, 32, 0, 7, 32], np.uint8)),
            RecentCase("many_1025", rows(1025), (np.arange(1025) % 33).astype(np.uint8))]
