"""Cases for processAttestation's checks (prysm_amd/csrc/attcheck.hip) and a plain model of them.

``model`` restates one attestation's checks in Go's types (blockchain/core.go:240-297 with
getSignedParentHashes :348-360, getAttesterIndices :363-374, validateAttesterBitfields :377-394):
``int(x)`` wraps to int64, so does ``slotNumber - CycleLength``; the slice bounds and the committee
index are uint64 differences that wrap; the checks run in Go's order.  It returns the three outputs
of ``pz_att_check_batch``: ``(status, committee, parents_start)``, with ``(.., 0xFFFFFFFF, 0)``
where the committee is not reached and ``parents_start = bs - s`` where it is.

``GROUPS`` are batches of named cases.  A group shares the chain state of one call
(``last_justified_slot``, ``last_state_recalc``, ``n_recent`` and the committee table); every case
is one attestation of it, named by the check it probes and tagged with the edge it sits on
(``Case.tags``), so that tests can ask whether both sides of an edge occur.  ``batch`` lays a group
out as the columns the entry points take; ``model_np`` states the model over such columns."""
import numpy as np

M64 = (1 << 64) - 1
CYCLE = 64
PROCESSED, SLOT_HIGH, SLOT_LOW, JUSTIFIED, NO_COMMITTEE, BITFIELD_LEN, TRAILING = 0, 2, 3, 4, 5, 6, 7
ERANGE, EINDEX = -7, -2
STATUSES = {PROCESSED, SLOT_HIGH, SLOT_LOW, JUSTIFIED, NO_COMMITTEE, BITFIELD_LEN, TRAILING, ERANGE, EINDEX}
NONE = 0xFFFFFFFF  # committee where it is not reached
LDS_WORDS = 12288  # the paired kernel keeps a table of at most this many 32-bit words in LDS
KS = tuple(range(18)) + (204, 205)  # committee sizes: committee c has KS[c] members
U64 = np.uint64


def i64(x):
    """Go's int(x) of a uint64 (and int arithmetic that wraps)."""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


class Table:
    """ShardAndCommitteesForSlots as pz_att_check_batch holds it.  ``arrays``: a list (one per slot)
    of lists of (shard id, committee id); ``sizes[c]``: the members of committee c (through coffs
    alone: no member is ever read).  ``offs`` replaces the offsets the arrays give (an inverted pair)."""

    def __init__(self, name, arrays, sizes=KS, offs=None, lookups=()):
        self.name, self.sizes, self.lookups = name, tuple(sizes), list(lookups)
        self.arr_offs = [0]
        for a in arrays:
            self.arr_offs.append(self.arr_offs[-1] + len(a))
        entries = [e for a in arrays for e in a]
        self.ne = len(entries)
        if offs is not None:
            assert len(offs) == len(self.arr_offs) and offs[-1] == self.ne and all(0 <= o <= self.ne for o in offs)
            self.arr_offs = list(offs)
        self.arr_shard = [e[0] for e in entries]
        self.arr_comm = [e[1] for e in entries]
        self.coffs = [0]
        for k in self.sizes:
            self.coffs.append(self.coffs[-1] + k)
        assert all(c < len(self.sizes) for c in self.arr_comm) and self.coffs[-1] <= M64

    @property
    def narr(self):
        return len(self.arr_offs) - 1

    @property
    def words(self):
        """What the paired kernel would stage: offsets, then shard, committee and size per entry."""
        return self.narr + 1 + 3 * self.ne

    @property
    def monotone(self):
        return all(a <= b for a, b in zip(self.arr_offs, self.arr_offs[1:]))

    @property
    def fits_lds(self):
        """The paired kernel walks this table in LDS (else in global memory)."""
        return (self.words <= LDS_WORDS and self.monotone and all(s >> 32 == 0 for s in self.arr_shard)
                and all(self.sizes[c] >> 32 == 0 for c in self.arr_comm))

    def entries(self, idx):
        return range(self.arr_offs[idx], self.arr_offs[idx + 1])  # (an inverted pair: empty)

    def find(self, idx, shard):
        """The first entry of array ``idx`` with ``shard``, or None."""
        for e in self.entries(idx):
            if self.arr_shard[e] == shard:
                return e
        return None

    def size_of(self, idx, shard):
        e = self.find(idx, shard)
        return None if e is None else self.sizes[self.arr_comm[e]]

    def with_size(self, k):
        """(array, shard) of an entry whose committee has ``k`` members and which its array's walk finds."""
        for idx in range(self.narr):
            for e in self.entries(idx):
                if self.sizes[self.arr_comm[e]] == k and self.find(idx, self.arr_shard[e]) == e:
                    return idx, self.arr_shard[e]
        raise KeyError(k)

    def arrays_np(self):
        """The four columns (placeholders of one entry where a column is empty)."""
        return dict(arr_offs=np.array(self.arr_offs, dtype=U64), arr_shard=np.array(self.arr_shard or [0], dtype=U64),
                    arr_comm=np.array(self.arr_comm or [0], dtype=np.uint32), coffs=np.array(self.coffs, dtype=U64))


class State:
    def __init__(self, ljs, lsr, n_recent, table):
        self.ljs, self.lsr, self.n_recent, self.table = ljs, lsr, n_recent, table


class Case:
    def __init__(self, name, s, bs, js, nob, shard, bits, tags=()):
        self.name, self.s, self.bs, self.js, self.nob, self.shard = name, s & M64, bs & M64, js & M64, nob & M64, shard
        self.bits, self.tags = bytes(bits), set(tags)

    def __repr__(self):
        return "Case(%s: s=%d bs=%d js=%d nob=%d shard=%d bits=%s)" % (self.name, self.s, self.bs, self.js, self.nob,
                                                                     self.shard, self.bits.hex())


def model(c, st, last_byte=None):
    """(status, committee, parents_start) of case ``c`` in state ``st``.  ``last_byte``: the byte the
    trailing-bits check reads, when it is not the bitfield's own last byte."""
    if i64(c.s) > i64(c.bs):  # core.go:244
        return SLOT_HIGH, NONE, 0
    if i64(c.s) < i64(i64(c.bs) - CYCLE):  # core.go:249: slotNumber - CycleLength is an int and wraps
        return SLOT_LOW, NONE, 0
    if c.js != st.ljs:  # core.go:255
        return JUSTIFIED, NONE, 0
    start, end = (c.bs - c.s) & M64, (c.bs - c.s - c.nob + CYCLE) & M64  # core.go:349-353
    if start > end or end > st.n_recent:
        return ERANGE, NONE, 0
    t = st.table
    idx = (c.s - st.lsr) & M64  # core.go:364-367
    if idx >= t.narr:
        return EINDEX, NONE, 0
    e = t.find(idx, c.shard)
    if e is None:
        return NO_COMMITTEE, NONE, start
    comm = t.arr_comm[e]
    k = (t.coffs[comm + 1] - t.coffs[comm]) & M64
    if (k + 7) // 8 != len(c.bits):  # core.go:379
        return BITFIELD_LEN, comm, start
    if k % 8:  # core.go:385-392: bits k .. of the last byte, most significant first
        last = c.bits[-1] if last_byte is None else last_byte
        if last & (0xFF >> (k % 8)):
            return TRAILING, comm, start
    return PROCESSED, comm, start


def good_bits(k, blen=None):
    """A bitfield of ``blen`` bytes (default: what k members need) with every member's bit set and,
    where the length is right, no trailing bit."""
    need = (k + 7) // 8
    blen = need if blen is None else blen
    b = bytearray(b"\xff" * blen)
    if blen == need and k % 8:
        b[-1] = (0xFF << (8 - k % 8)) & 0xFF
    return bytes(b)


# ---- the tables ------------------------------------------------------------------------------------
def _perm(j):
    return (7 * j + 3) % len(KS)  # entry j of array 0 -> its committee: non-monotone, a bijection


_A0 = [(3 * j, _perm(j)) for j in range(len(KS))]  # shard 0 first, shard 57 last, every size once
_A2 = [(9, 5), (9, 11), (4, 5)]  # shard 9 twice (the first wins); committee 5 shared with array 0
_PLAIN = [_A0, [], _A2, [(77, 2)], [(1, 19), (2, 18)]]
_PLAIN_LOOKUPS = [("empty_array", 1, 0), ("first_entry_shard0", 0, 0), ("last_entry", 0, 57), ("duplicate_shard", 2, 9),
                  ("after_duplicate", 2, 4), ("neighbour_only_below", 2, 77), ("neighbour_only_above", 4, 77),
                  ("in_its_array", 3, 77), ("shard_plus_2_32", 3, 77 + (1 << 32)), ("shard0_absent", 3, 0),
                  ("last_array_last_entry", 4, 2)]


def _fill(n, first):
    """n filler entries with distinct shard ids from ``first`` on; the last one's shard is 999,999."""
    return [(first + j, j % len(KS)) for j in range(n - 1)] + [(999_999, 13)]


def plain_table():
    return Table("plain", _PLAIN, lookups=_PLAIN_LOOKUPS)


def lds_limit_table():
    """narr + 1 + 3 ne == 12,288: the largest table the paired kernel stages."""
    t = Table("lds_limit", [_A0 + _A2, _fill(4095 - 23, 1000)],
              lookups=[("duplicate_shard", 0, 9), ("tables_last_entry", 1, 999_999), ("first_of_second", 1, 1000),
                       ("neighbour_only", 0, 1000), ("shard_plus_2_32", 1, 1000 + (1 << 32)), ("absent", 1, 5)])
    assert t.words == LDS_WORDS and t.narr == 2 and t.ne == 4095
    return t


def over_limit_table():
    """narr + 1 + 3 ne == 12,289: one word too many, so the global walk."""
    t = Table("over_limit", [_A0 + _A2, [], _fill(4095 - 23, 1000)],
              lookups=[("duplicate_shard", 0, 9), ("empty_array", 1, 0), ("tables_last_entry", 2, 999_999),
                       ("neighbour_only", 0, 1000), ("shard_plus_2_32", 2, 1000 + (1 << 32)), ("absent", 2, 5)])
    assert t.words == LDS_WORDS + 1 and t.narr == 3 and t.ne == 4095
    return t


def wide_table():
    """256 arrays of 16 entries (12,545 words: the global walk); the sizes sit in arrays 0 and 1."""
    arrays = [[((16 * a + j) * 5 % 4099, (16 * a + j) % len(KS)) for j in range(16)] for a in range(256)]
    t = Table("wide", arrays, lookups=[("first_entry_shard0", 0, 0), ("last_entry", 0, 75), ("neighbour_only", 1, 75),
                                       ("last_array_first", 255, 255 * 16 * 5 % 4099),
                                       ("tables_last_entry", 255, 4095 * 5 % 4099),
                                       ("shard_plus_2_32", 7, 7 * 16 * 5 % 4099 + (1 << 32)), ("absent", 200, 4098)])
    assert t.narr == 256 and t.ne == 4096
    return t


def big_shard_table():
    """The plain table with one shard id >= 2^32: the whole table goes to the global walk."""
    arrays = [list(a) for a in _PLAIN]
    arrays[3].append(((1 << 32) + 78, 10))
    return Table("big_shard", arrays, lookups=_PLAIN_LOOKUPS + [("big_shard_exact", 3, (1 << 32) + 78),
                                                                 ("big_shard_low_half", 3, 78),
                                                                 ("big_shard_other_high", 3, (1 << 33) + 78)])


HUGE = (1 << 32) + 5


def huge_committee_table():
    """The plain table plus committee 20 of 2^32 + 5 members (coffs alone says so)."""
    arrays = [list(a) for a in _PLAIN]
    arrays[4].append((555, 20))
    return Table("huge_committee", arrays, sizes=KS + (HUGE,), lookups=_PLAIN_LOOKUPS)


def inverted_table():
    """The plain table with arr_offs[2] < arr_offs[1], both in range: array 1 reads as empty and
    array 2 starts two entries early.  (The host form refuses it: device form only.)"""
    t = Table("inverted", _PLAIN, offs=[0, 20, 18, 23, 24, 26],
              lookups=_PLAIN_LOOKUPS + [("inverted_reads_empty", 1, 54), ("inverted_reads_empty_2", 1, 57),
                                        ("early_start", 2, 54)])
    assert not t.monotone
    return t


def empty_table():
    return Table("narr0", [])


# ---- the cases -------------------------------------------------------------------------------------
BS_EDGES = (0, 1, 63, 64, 65, 200, (1 << 63) - 1, 1 << 63, (1 << 63) + 63, (1 << 63) + 64, M64)


def build_cases(st):
    """Every case of one group, by the check it probes.  The first and the last case have k = 0 and
    an empty bitfield, so that a batch starts with boffs 0, 0 however it is rotated."""
    t, out, seen = st.table, [], set()
    nob0 = max(0, CYCLE - st.n_recent)  # with bs == s the slice [0, 64 - nob0) fits n_recent

    def add(name, a=0, d=0, nob=None, shard=None, bits=None, js=None, s=None, bs=None, tags=()):
        s = (st.lsr + a) & M64 if s is None else s & M64
        bs = (s + d) & M64 if bs is None else bs & M64
        idx = (s - st.lsr) & M64
        if shard is None:  # the first entry of the array the slot selects, when there is one
            shard = t.arr_shard[t.entries(idx)[0]] if idx < t.narr and len(t.entries(idx)) else 0
        if bits is None:
            k = t.size_of(idx, shard) if idx < t.narr else None
            bits = good_bits(k) if k is not None and k < (1 << 20) else b"\x80"
        assert name not in seen, name
        seen.add(name)
        out.append(Case(name, s, bs, st.ljs if js is None else js, nob0 if nob is None else nob, shard, bits, tags))

    if t.narr:
        a0, sh0 = t.with_size(0)
        add("first_row_k0_empty", a=a0, shard=sh0, bits=b"", tags={"k0_blen0"})

    # slot window: int(s) > int(bs), int(s) < int(bs) - 64 (core.go:244-253)
    pairs = []
    for bs in BS_EDGES:
        for s in (bs, bs + 1, bs - 64, bs - 65, 0, 1 << 63, M64):
            if (s & M64, bs) not in pairs:
                pairs.append((s & M64, bs))
    for s, bs in pairs:
        tags = set()
        if s == (bs - 64) & M64:
            tags.add("s==bs-64")
        if s == (bs - 65) & M64:
            tags.add("s==bs-65")
        if s == (bs + 1) & M64:
            tags.add("s==bs+1")
        if s == bs:
            tags.add("s==bs")
        if s == 0 and bs < 64:
            tags.add("s0_bs<64")
        if 1 << 63 <= bs < (1 << 63) + 64:
            tags.add("bs-64_wraps")
        if (s, bs) == (1 << 63, (1 << 63) - 1):
            tags.add("low_not_high")
        if (s, bs) == (M64, 0):
            tags.add("minus_one_over_zero")
        add("window_s%x_bs%x" % (s, bs), s=s, bs=bs, tags=tags)

    # justified slot (core.go:255)
    for name, js in (("ljs-1", st.ljs - 1), ("ljs+1", st.ljs + 1), ("ljs+2^32", st.ljs + (1 << 32))):
        add("justified_" + name, js=js, tags={"justified_" + name})

    # slice bounds [d, d - nob + 64) of n_recent hashes (core.go:349-353)
    add("slice_d64_nob0", d=64, nob=0, tags={"end==128"})
    for d in (0, 10):
        for nob in dict.fromkeys((64, 65, d + 64, d + 65, M64)):  # (d 10, nob 65: start > end alone;
            # d 0, nob 65: end wraps, end > n_recent alone)
            add("slice_d%d_nob%x" % (d, nob), d=d, nob=nob, tags={"nob%d_d%d" % (nob, d)} if nob in (64, 65) else set())
    # end == n_recent and end == n_recent + 1, where the window lets a row get there
    for what, end in (("end==n_recent", st.n_recent), ("end==n_recent+1", st.n_recent + 1)):
        d = max(0, end - CYCLE)
        if d <= CYCLE and end <= 2 * CYCLE:
            add("slice_" + what, d=d, nob=d + CYCLE - end, tags={what})
    add("slice_erange_and_eindex", a=t.narr, d=10, nob=65, tags={"erange_and_eindex"})

    # the array index s - last_state_recalc (core.go:364-367)
    add("index_s_lsr-1", s=st.lsr - 1, tags={"s<lsr"})
    add("index_narr", a=t.narr, tags={"idx==narr"})
    if t.narr:
        add("index_narr-1", a=t.narr - 1, tags={"idx==narr-1"})

    if t.narr:
        # the walk of one array (core.go:368-373)
        for name, a, shard in t.lookups:
            add("lookup_" + name, a=a, shard=shard, tags={"lookup_" + name})
        if HUGE in t.sizes:
            a, sh = t.with_size(HUGE)
            add("huge_committee_blen1", a=a, shard=sh, bits=b"\xf8", tags={"huge_committee"})  # fits k = 5

        # the bitfield: its length and the trailing bits of its last byte (core.go:379-392)
        for k in KS:
            a, sh = t.with_size(k)
            need = (k + 7) // 8
            for blen in sorted({need, need + 1, max(need - 1, 0), 0}):
                if (k, blen) != (0, 0):
                    add("bits_k%d_blen%d" % (k, blen), a=a, shard=sh, bits=good_bits(k, blen),
                        tags={"blen-need=%d" % (blen - need)} if blen else {"blen0"})
        for r in range(1, 8):
            a, sh = t.with_size(r)
            for bit in range(8):
                add("trailing_r%d_bit%d" % (r, bit), a=a, shard=sh, bits=bytes([1 << bit]), tags={("r_bit", r, bit)})
        for k in (8, 16):
            a, sh = t.with_size(k)
            add("trailing_r0_ff_k%d" % k, a=a, shard=sh, bits=b"\xff" * (k // 8), tags={"r0_ff"})
        add("last_row_k0_empty", a=a0, shard=sh0, bits=b"", tags={"k0_blen0"})
    return out


class Group:
    def __init__(self, name, st, partial=None):
        self.name, self.st, self.partial = name, st, partial
        self.cases = build_cases(st)
        self.want = [model(c, st) for c in self.cases]

    @property
    def host_form(self):
        return self.st.table.monotone  # pz_check_attestations refuses offsets that are not monotone


_groups = None


def groups():
    """name -> Group (built once).  ``partial``: why a group cannot hold all nine statuses."""
    global _groups
    if _groups is None:
        gs = [Group("plain", State(5, 0, 128, plain_table())),
              Group("lsr64", State(60, 64, 127, plain_table())),
              Group("wide", State(1 << 40, 3, 100, wide_table())),
              Group("lds_limit", State(0, 0, 64, lds_limit_table())),
              Group("over_limit", State(1, 1, 0, over_limit_table())),
              Group("big_shard", State(5, 0, 128, big_shard_table())),
              Group("huge_committee", State(5, 0, 128, huge_committee_table())),
              Group("inverted", State(5, 0, 128, inverted_table())),
              Group("narr0", State(5, 0, 128, empty_table()),
                    partial="with no array every row that passes the slice bounds is EINDEX")]
        _groups = {g.name: g for g in gs}
    return _groups


def batch(cases, complement_last=False):
    """The attestation columns of ``cases`` in order, plus ``last_byte`` (each bitfield's last byte;
    0xFF for an empty one, which no check may read).  ``complement_last``: the last byte of every
    bitfield is complemented in ``bits`` (``last_byte`` keeps the real one)."""
    n = len(cases)
    cols = dict(slot=np.array([c.s for c in cases], dtype=U64), justified_slot=np.array([c.js for c in cases], dtype=U64),
                shard_id=np.array([c.shard for c in cases], dtype=U64), n_oblique=np.array([c.nob for c in cases], dtype=U64),
                block_slot=np.array([c.bs for c in cases], dtype=U64))
    boffs = np.zeros(n + 1, dtype=U64)
    boffs[1:] = np.cumsum([len(c.bits) for c in cases], dtype=U64)
    bits = np.frombuffer(b"".join(c.bits for c in cases) + b"\0", dtype=np.uint8).copy()
    ends = boffs[1:].astype(np.int64) - 1
    last = np.where(boffs[1:] > boffs[:-1], bits[np.maximum(ends, 0)], 0xFF).astype(np.uint8)
    cols.update(bits=bits, boffs=boffs, last_byte=last)
    return complemented(cols) if complement_last else cols


def complemented(cols):
    """``cols`` with the last byte of every bitfield complemented in ``bits``: what the checks must
    not read when ``last_byte`` is given."""
    boffs, bits = cols["boffs"], cols["bits"].copy()
    bits[(boffs[1:].astype(np.int64) - 1)[boffs[1:] > boffs[:-1]]] ^= 0xFF
    return dict(cols, bits=bits)


def model_np(cols, st, last_byte=None):
    """``model`` over columns, vectorised: (status int32, committee uint32, parents_start uint64).
    ``last_byte`` (default: read from ``bits``) as in pz_att_check_batch."""
    t = st.table
    tab = t.arrays_np()
    s, bs, js, nob, shard = (cols[k] for k in ("slot", "block_slot", "justified_slot", "n_oblique", "shard_id"))
    n = len(s)
    si, bi = s.view(np.int64), bs.view(np.int64)
    with np.errstate(over="ignore"):
        lim = (bs - U64(CYCLE)).view(np.int64)  # int(bs) - 64, wrapping
        start = bs - s
        end = start - nob + U64(CYCLE)
        idx = s - U64(st.lsr)
    status = np.full(n, PROCESSED, dtype=np.int32)
    comm = np.full(n, NONE, dtype=np.uint32)
    todo = np.ones(n, dtype=bool)

    def settle(mask, code):
        status[todo & mask] = code
        todo[mask] = False

    settle(si > bi, SLOT_HIGH)
    settle(si < lim, SLOT_LOW)
    settle(js != U64(st.ljs), JUSTIFIED)
    settle((start > end) | (end > U64(st.n_recent)), ERANGE)
    settle(idx >= U64(t.narr), EINDEX)
    pstart = np.where(todo, start, U64(0))
    ix = np.where(todo, idx, U64(0)).astype(np.int64)
    lo, hi = tab["arr_offs"][ix].astype(np.int64), tab["arr_offs"][np.minimum(ix + 1, t.narr)].astype(np.int64)
    found = np.full(n, -1, dtype=np.int64)
    for j in range(int((hi - lo).max()) if n and t.narr else 0):
        e = lo + j
        hit = todo & (found < 0) & (e < hi)
        hit[hit] = tab["arr_shard"][e[hit]] == shard[hit]
        found[hit] = e[hit]
    settle(found < 0, NO_COMMITTEE)
    c = tab["arr_comm"][np.maximum(found, 0)]
    comm[todo] = c[todo]
    k = tab["coffs"][c.astype(np.int64) + 1] - tab["coffs"][c.astype(np.int64)]
    blen = cols["boffs"][1:] - cols["boffs"][:-1]
    settle((k + U64(7)) // U64(8) != blen, BITFIELD_LEN)
    r = (k % U64(8)).astype(np.int64)
    last = cols["bits"][np.maximum(cols["boffs"][1:].astype(np.int64) - 1, 0)] if last_byte is None else last_byte
    settle((r > 0) & ((last.astype(np.int64) & (0xFF >> r)) != 0), TRAILING)
    return status, comm, pstart


def port_status(cols, st):
    """The C port (oracle/c/attcheck_ref.c) over the same columns: status only."""
    from oracle import cport

    tab = st.table.arrays_np()
    port = cport.AttCheck(cols["slot"], cols["justified_slot"], cols["shard_id"], cols["n_oblique"], cols["bits"],
                          cols["boffs"], cols["block_slot"])
    try:
        return port.run(st.ljs, st.lsr, st.n_recent, tab["arr_offs"], tab["arr_shard"], tab["arr_comm"], tab["coffs"]).copy()
    finally:
        port.close()


# ---- the grid-stride mixture -----------------------------------------------------------------------
P_THREADS, P_BLOCKS_PER_CU = 512, 3  # the paired kernel: lanes per block, blocks per CU at most


def stride_rows(cus):
    """Rows one trip of the paired kernel's loop covers once its grid is full: 2 per lane."""
    return 2 * P_BLOCKS_PER_CU * cus * P_THREADS


def stride_natt(cus):
    """Two full trips, one more for the first 512 lanes, and an odd tail."""
    return 2 * stride_rows(cus) + 2 * P_THREADS + 3


def mixture(natt, st, seed, pinned=()):
    """A numpy-built batch over ``st`` (the plain table, last_state_recalc 0) in which every status
    occurs; ``pinned``: (row, name) pairs that get one of the known failing rows below."""
    rng = np.random.default_rng(seed)
    t = st.table
    assert t.name == "plain" and st.lsr == 0
    ent = rng.integers(0, t.ne, size=natt)  # the entry each row aims at
    arr = np.searchsorted(np.array(t.arr_offs), ent, side="right") - 1
    k = np.array(t.sizes, dtype=np.int64)[np.array(t.arr_comm)[ent]]
    d = rng.integers(0, 65, size=natt)
    s = arr.astype(U64)
    js = np.full(natt, st.ljs, dtype=U64)
    nob = np.zeros(natt, dtype=U64)
    shard = np.array(t.arr_shard, dtype=U64)[ent]
    blen = (k + 7) // 8
    kind = rng.integers(0, 24, size=natt)  # 0..8: one failure each, the rest pass
    names = ("high", "low", "justified", "erange", "eindex", "no_committee", "len", "trailing", "plus32")
    for row, name in pinned:
        kind[row] = names.index(name)
    d = np.where(kind == 0, -1 - (d % 3), np.where(kind == 1, 65 + d, d))
    js[kind == 2] += U64(1)
    nob[kind == 3] = U64(70)
    d = np.where(kind == 3, np.minimum(d, 5), d)  # start 0..5, end start - 6 wraps: ERANGE
    s = np.where(kind == 4, U64(t.narr) + (ent % 3).astype(U64), s)
    shard = np.where(kind == 5, U64(3001), np.where(kind == 8, shard + U64(1 << 32), shard))
    blen = np.where(kind == 6, blen + 1, blen)
    bs = (s.astype(np.int64) + d).astype(U64)
    boffs = np.zeros(natt + 1, dtype=U64)
    boffs[1:] = np.cumsum(blen, dtype=U64)
    bits = rng.integers(0, 256, size=int(boffs[-1]) + 1, dtype=np.uint8)
    ends = boffs[1:].astype(np.int64) - 1
    full = blen > 0
    r = (k % 8)[full]
    clear = np.where(r > 0, (0xFF << (8 - r)) & 0xFF, 0xFF).astype(np.uint8)
    bad = np.where((kind[full] == 7) & (r > 0), (1 << rng.integers(0, 8, size=r.size) % np.maximum(8 - r, 1)), 0)
    bits[ends[full]] = (bits[ends[full]] & clear) | bad.astype(np.uint8)
    last = np.where(full, bits[np.maximum(ends, 0)], 0xFF).astype(np.uint8)
    return dict(slot=s, justified_slot=js, shard_id=shard, n_oblique=nob, block_slot=bs, bits=bits, boffs=boffs,
                last_byte=last)
