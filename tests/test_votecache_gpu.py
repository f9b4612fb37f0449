"""The device-resident block vote cache (prysm_amd/csrc/votecache.hip: pz_vote_cache_*,
prysm_amd.votes.DeviceVoteCache, blockchain.tally_serialized_blocks) against the scalar oracle.

The oracle is oracle.ref.calculate_block_vote_cache (blockchain/core.go:300-345) applied, in
order, to the rows that are taken and PROCESSED; results compare as {hash: (sorted voters, total)},
which includes the set of present hashes.  Columns come from wire.attestation_columns; status,
committee and parents_start from blockchain.check_attestations (unless a test sets them by hand
and says so).  Every device column is followed by a pad of 0xA5 bytes, so a byte taken from beyond
a range shows in a hash or a total."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ref
from oracle import replay as oreplay
from oracle import schema as opb
from prysm_amd import _lib, pb, synth, wire
from prysm_amd import blockchain as bc
from prysm_amd.votes import DeviceVoteCache, VoteCache
from test_attcheck_gpu import table

pytestmark = pytest.mark.gpu

U64 = np.uint64
PROCESSED = 0
NONE32 = 0xFFFFFFFF
COLS = ("attester_bitfield", "attester_bitfield_offs", "oblique_parent_hashes", "oblique_offs", "oblique_first")
USED = {"attester_bitfield": "attester_bitfield_offs", "oblique_parent_hashes": "oblique_offs"}


class State:
    """A genesis chain state with the given RecentBlockHashes (32-byte strings) and balances."""

    def __init__(self, nval, recent, balances=None):
        self.nval = nval
        self.active, self.cs = ref.new_genesis_states(nval)
        if balances is not None:
            for v, b in zip(self.cs.validators, balances):
                v.balance = int(b)
        del self.active.recent_block_hashes[:]
        self.active.recent_block_hashes.extend(recent)
        self.recent = np.frombuffer(b"".join(recent), dtype=np.uint8).reshape(-1, 32).copy()
        self.tab = table(self.cs)
        self.members = np.concatenate([np.array(e[1], np.uint32) for arr in self.tab for e in arr])
        self.coffs = bc._committee_table(self.tab)[3]
        self.balance = np.array([v.balance for v in self.cs.validators], U64)

    def committee(self, slot, j=0):
        """(shard id, members) of the j-th committee of ``slot`` (counted round its committees)."""
        arr = self.tab[slot - self.cs.last_state_recalc]
        return arr[j % len(arr)]

    def check(self, atts, bslots):
        status, ci, pstart = bc.check_attestations(atts, bslots, self.cs.last_justified_slot,
                                                   self.cs.last_state_recalc, len(self.recent), self.tab)
        return status.astype(np.int32), (ci & NONE32).astype(np.uint32), pstart.astype(U64)

    def oracle(self, cache_o, atts, bslots, status, take=None):
        for i, (a, bs) in enumerate(zip(atts, bslots)):
            if status[i] == PROCESSED and (take is None or take[i]):
                ref.calculate_block_vote_cache(self.cs, self.active, cache_o, bs, a)
        return cache_o


def att(state, slot, rng, obliques=(), j=0, p=0.6):
    shard, comm = state.committee(slot, j)
    bits = rng.random(len(comm)) < p
    return opb.AttestationRecord(slot=slot, shard_id=shard, justified_slot=state.cs.last_justified_slot,
                                 attester_bitfield=np.packbits(bits.astype(np.uint8)).tobytes(),
                                 oblique_parent_hashes=list(obliques))


def put(a):
    """A host array on the device, followed by 64 bytes of 0xA5 (uint32/uint64 as int32/int64)."""
    import torch

    a = np.ascontiguousarray(a)
    raw = np.concatenate([a.view(np.uint8).ravel(), np.full(64, 0xA5, np.uint8)])
    t = torch.from_numpy(raw).to("cuda:0")[:a.nbytes]
    dt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[a.dtype.itemsize]
    return t.view(dt).view(a.shape) if a.nbytes else t.view(dt)


def dev_cols(cols):
    return {k: put(cols[k][:int(cols[USED[k]][-1])] if k in USED else cols[k]) for k in COLS if cols.get(k) is not None}


def tally_dev(cache, state, cols, n, status, comm, pstart, take=None, members=None, coffs=None):
    cache.tally_columns(dev_cols(cols), n, put(status), put(comm), put(pstart), put(state.recent),
                        put(state.members if members is None else members), put(state.coffs if coffs is None else coffs),
                        put(state.balance), take=None if take is None else put(take))


def tally_host(cache, state, cols, n, status, comm, pstart, take=None, members=None, coffs=None):
    cache.tally_host(cols, n, status, comm, pstart, state.recent, state.members if members is None else members,
                     state.coffs if coffs is None else coffs, state.balance, take)


FORMS = {"device": tally_dev, "host": tally_host}


def snapshot(cache, strict=True):
    return {h: (cache.voters(h, strict).tolist(), t) for h, t in cache.items(strict).items()}


def want(cache_o):
    return {h: (sorted(v), t) for h, (v, t) in cache_o.items()}


def rand_hashes(rng, n):
    return [rng.bytes(32) for _ in range(n)]


# ---- 1: the scenario of test_votes_gpu ---------------------------------------------------------------
@functools.lru_cache(None)
def parity_case():
    rng = np.random.default_rng(12)
    hashes = rand_hashes(rng, 128)
    st = State(3000, hashes, balances=rng.integers(1, 1000, size=3000))
    calls = []
    for block_slot in (10, 11, 12):
        atts = []
        for _ in range(6):
            s = int(rng.integers(block_slot - 3, block_slot + 1))
            obl = [hashes[int(rng.integers(0, 128))] for _ in range(int(rng.integers(0, 3)))]
            if rng.random() < 0.5:
                obl.append(b"\x07")  # short oblique: right-aligned by BytesToHash
            atts.append(att(st, s, rng, obl))
        calls.append((atts, [block_slot] * 6))
    cache_o, skipped_recent, twice = {}, 0, False
    for atts, bslots in calls:
        for a, bs in zip(atts, bslots):
            parents = ref.get_signed_parent_hashes(st.active, bs, a)
            obl = [bytes(o) for o in a.oblique_parent_hashes]
            skipped_recent += sum(h in obl for h in parents[:64 - len(obl)])
            voters = {v for i, v in enumerate(st.committee(a.slot)[1]) if ref.check_bit(a.attester_bitfield, i)}
            twice = twice or any(h not in obl and h in cache_o and voters & set(cache_o[h][0]) for h in parents)
            ref.calculate_block_vote_cache(st.cs, st.active, cache_o, bs, a)
    return st, calls, cache_o, skipped_recent, twice


@pytest.mark.parametrize("form", ["device", "host"])
def test_parity_with_the_host_listed_tally(form):
    st, calls, cache_o, skipped_recent, twice = parity_case()
    # conditions on the inputs, from the oracle alone
    assert skipped_recent >= 1 and twice
    assert any(h not in {r.tobytes() for r in st.recent} for h in cache_o)
    cache = DeviceVoteCache(st.nval, 256)
    vc = VoteCache(st.nval)
    for atts, bslots in calls:
        status, comm, pstart = st.check(atts, bslots)
        assert (status == PROCESSED).all()
        cols = wire.attestation_columns(atts)
        FORMS[form](cache, st, cols, len(atts), status, comm, pstart)
        items = []
        for ai, (a, bs) in enumerate(zip(atts, bslots)):
            obl = [bytes(o) for o in a.oblique_parent_hashes]
            items += [(ai, vc.slot(h)) for h in ref.get_signed_parent_hashes(st.active, bs, a) if h not in obl]
        vc.tally(st.members, st.coffs, comm, cols["attester_bitfield"], cols["attester_bitfield_offs"], items, st.balance)
    got = snapshot(cache)
    assert got == want(cache_o)
    assert got == {h: (vc.voters(h).tolist(), vc.total(h)) for h in vc.slot_of}
    for h in cache_o:
        assert h in cache and cache.total(h) == cache_o[h][1]
    assert b"\x55" * 32 not in cache and cache.total(b"\x55" * 32) == 0


# ---- 2: the genesis state's recent hashes ---------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
def test_all_equal_recent_is_one_slot(form):
    rng = np.random.default_rng(2)
    st = State(1024, [bytes(32)] * 128, balances=rng.integers(1, 1000, size=1024))
    atts = [att(st, s, rng, j=0) for s in (3, 3, 4, 5)]
    bslots = [6, 7, 7, 64]
    status, comm, pstart = st.check(atts, bslots)
    assert (status == PROCESSED).all() and set(pstart.tolist()) >= {3, 59}
    cache = DeviceVoteCache(st.nval, 4)
    FORMS[form](cache, st, wire.attestation_columns(atts), len(atts), status, comm, pstart)
    voters = set()
    for a in atts:
        voters |= {v for i, v in enumerate(st.committee(a.slot)[1]) if ref.check_bit(a.attester_bitfield, i)}
    assert snapshot(cache) == {bytes(32): (sorted(voters), int(st.balance[sorted(voters)].sum()))}
    assert snapshot(cache) == want(st.oracle({}, atts, bslots, status))


# ---- 3: element lengths, byte phases, m and parents_start ---------------------------------------------------
@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_element_lengths_and_alignment(phase):
    rng = np.random.default_rng(30 + phase)
    recent = rand_hashes(rng, 128)
    st = State(1024, recent, balances=rng.integers(1, 1000, size=1024))
    k = 70  # recent[k] lies in the window of a row whose parents start at 64
    atts, bslots, tag = [], [], []

    def add(name, slot, bs, obliques):
        atts.append(att(st, slot, rng, obliques, j=len(atts) % 2))
        bslots.append(bs)
        tag.append(name)

    add("phase", 2, 2, [rng.bytes(phase)])  # every later element starts at this byte phase, then moves on
    for ln in (0, 1, 31, 32, 33, 40):
        add("len%d" % ln, 1, 1, [rng.bytes(ln)])
        add("len%d+pad" % ln, 1, 65, [rng.bytes(ln), rng.bytes(4 - (ln + phase) % 4)])
    add("shares", 1, 65, [b"\x09" + recent[k]])              # its hash is recent[k]: one slot for both
    add("shares-alone", 1, 1, [b"\x09" + recent[k]])          # ... here recent[k] is no parent: the element alone
    add("skipped-by-raw", 1, 65, [b"\x09" + recent[k], recent[k]])
    add("removes-parent", 1, 65, [recent[k]])
    add("m0", 0, 0, [])
    add("m0-high", 0, 64, [])
    add("m63", 1, 1, [rng.bytes(int(rng.choice([0, 5, 32, 33]))) for _ in range(63)])
    add("m64-mixed", 1, 65, [rng.bytes(int(rng.choice([1, 31, 32, 40]))) for _ in range(64)])
    add("m64-raw", 1, 65, rand_hashes(rng, 64))
    status, comm, pstart = st.check(atts, bslots)
    assert (status == PROCESSED).all()
    assert {0, 64} <= set(pstart.tolist())  # 64 == n_recent - 64
    assert {len(a.oblique_parent_hashes) for a in atts} >= {0, 1, 63, 64}
    cols = wire.attestation_columns(atts)
    starts = cols["oblique_offs"][:-1] % 4
    assert (starts[1:3] == phase).all() and len(set(starts.tolist())) == 4
    cache_o = st.oracle({}, atts, bslots, status)
    # conditions, from the oracle alone: what each hand-made row does
    alone = {}
    for name in ("shares", "skipped-by-raw", "removes-parent", "m64-raw", "m63"):
        i = tag.index(name)
        alone[name] = st.oracle({}, [atts[i]], [bslots[i]], status[i:i + 1])
    assert len(alone["shares"]) == 63 and recent[k] in alone["shares"]  # 63 parents + the element, which shares one's slot
    assert len(alone["skipped-by-raw"]) == 61 and recent[k] not in alone["skipped-by-raw"]
    assert len(alone["removes-parent"]) == 62 and recent[k] not in alone["removes-parent"]
    assert alone["m64-raw"] == {} and 1 <= len(alone["m63"]) <= 64
    for form in ("device", "host"):
        cache = DeviceVoteCache(st.nval, 512)
        FORMS[form](cache, st, cols, len(atts), status, comm, pstart)
        assert snapshot(cache) == want(cache_o), form


# ---- 4: rows that are not PROCESSED or not taken -----------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
def test_other_statuses_and_untaken_rows_tally_nothing(form):
    """status, committee and parents_start of the dead rows are set by hand: every code a check
    or the decoder can report, with the committee and parents_start such a row may carry
    (UINT32_MAX; any value), so nothing may be read through them."""
    rng = np.random.default_rng(4)
    recent = rand_hashes(rng, 128)
    st = State(1024, recent, balances=rng.integers(1, 1000, size=1024))
    codes = [1, 2, 3, 4, 5, 6, 7, _lib.PZ_ERANGE, _lib.PZ_EINDEX, _lib.PZ_EINVAL]
    atts, bslots, dead, only_dead = [], [], {}, []
    for i in range(40):
        mark = rng.bytes(33)  # an element no other row has: its hash is in the cache iff this row is tallied
        atts.append(att(st, 1, rng, [mark], j=i % 2))
        bslots.append(1 + int(rng.integers(0, 60)))
        if i % 3 == 1:
            dead[i] = codes[(i // 3) % len(codes)]
            only_dead.append(mark[1:])
    i_inv = len(atts)  # a record the decoder refused: zero scalars and empty ranges
    atts.append(opb.AttestationRecord())
    bslots.append(1)
    status, comm, pstart = st.check(atts, bslots)
    assert (status[:i_inv] == PROCESSED).all()
    dead[i_inv] = _lib.PZ_EINVAL
    assert set(dead.values()) == set(codes)
    for i, code in dead.items():
        status[i], comm[i], pstart[i] = code, NONE32, U64(rng.integers(0, 1 << 62))
    take = np.ones(len(atts), np.uint8)
    for i in range(0, i_inv, 7):
        if i not in dead:
            take[i] = 0
            only_dead.append(bytes(atts[i].oblique_parent_hashes[0])[1:])
    take[5] = 0xA5  # any non-zero value takes the row
    assert 5 not in dead and (take == 0).sum() >= 4
    cache_o = st.oracle({}, atts, bslots, status, take)
    assert cache_o and not any(h in cache_o for h in only_dead)
    cache = DeviceVoteCache(st.nval, 256)
    FORMS[form](cache, st, wire.attestation_columns(atts), len(atts), status, comm, pstart, take=take)
    assert snapshot(cache) == want(cache_o)
    assert not any(h in cache for h in only_dead)
    # the same rows with everything dead: an empty cache
    none = DeviceVoteCache(st.nval, 4)
    FORMS[form](none, st, wire.attestation_columns(atts), len(atts), status, comm, pstart, take=np.zeros(len(atts), np.uint8))
    assert none.items() == {}


# ---- 5: collisions -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot_cap,k", [(1, 1), (2, 1), (2, 2), (4, 1), (4, 3), (4, 4)])
def test_colliding_hashes_and_the_wrap(slot_cap, k):
    """k distinct hashes whose first four bytes are FF FF FF FF: their home cell is the last cell
    of the table (le32(hash[0..4]) & (cells - 1), cells = 2, 4 or 8), so the second one wraps to
    cell 0.  Every hash is found again by a second call; slot ids are stable."""
    rng = np.random.default_rng(50 + 8 * slot_cap + k)
    pool = [b"\xff" * 4 + rng.bytes(28) for _ in range(k)]
    recent = [pool[int(i)] for i in np.concatenate([np.arange(k), rng.integers(0, k, 128 - k)])]
    st = State(1024, recent, balances=rng.integers(1, 1000, size=1024))
    calls = [([att(st, 0, rng, j=0), att(st, 1, rng, j=1)], [3, 64]), ([att(st, 2, rng, j=0), att(st, 0, rng, j=1)], [2, 5])]
    for form in ("device", "host"):
        cache, cache_o, order = DeviceVoteCache(st.nval, slot_cap), {}, None
        for atts, bslots in calls:
            status, comm, pstart = st.check(atts, bslots)
            assert (status == PROCESSED).all()
            FORMS[form](cache, st, wire.attestation_columns(atts), len(atts), status, comm, pstart)
            st.oracle(cache_o, atts, bslots, status)
            hashes, _ = cache.read()
            assert len(hashes) == k and len(cache_o) == k
            order = order if order is not None else hashes.copy()
            np.testing.assert_array_equal(hashes, order)
            assert snapshot(cache) == want(cache_o)


# ---- 6: slot order -------------------------------------------------------------------------------------------
def test_new_slots_are_numbered_by_ascending_source():
    rng = np.random.default_rng(6)
    recent = rand_hashes(rng, 128)
    recent[90] = recent[20]  # a repeated recent hash: its slot comes with position 20
    st = State(1024, recent, balances=rng.integers(1, 1000, size=1024))
    atts = [att(st, 1, rng, [rng.bytes(5), rng.bytes(33)]), att(st, 0, rng, [rng.bytes(40)]), att(st, 1, rng, [b"\x01\x02"])]
    atts.append(att(st, 1, rng, [bytes(atts[2].oblique_parent_hashes[0])]))  # an element seen before
    bslots = [65, 40, 11, 1]
    status, comm, pstart = st.check(atts, bslots)
    assert (status == PROCESSED).all()
    cols = wire.attestation_columns(atts)
    # the expected order from the source numbering alone: recent positions, then elements
    used_recent, elems = set(), []
    for a, ps in zip(atts, pstart.tolist()):
        m = len(a.oblique_parent_hashes)
        used_recent |= set(range(ps, ps + 64 - m))
        elems += [ref.bytes_to_hash(bytes(e)) for e in a.oblique_parent_hashes]  # (none is 32 bytes: all tallied)
    order = []
    for h in [recent[s] for s in sorted(used_recent)] + elems:
        if h not in order:
            order.append(h)
    assert len(order) == len(used_recent) + len(elems) - 2 and {20, 90} <= used_recent  # two repeats share a slot
    reads = []
    for form in ("device", "device", "host"):
        cache = DeviceVoteCache(st.nval, 256)
        FORMS[form](cache, st, cols, len(atts), status, comm, pstart)
        hashes, totals = cache.read()
        assert [h.tobytes() for h in hashes] == order
        reads.append((hashes, totals))
    for hashes, totals in reads[1:]:
        np.testing.assert_array_equal(hashes, reads[0][0])
        np.testing.assert_array_equal(totals, reads[0][1])


# ---- 7: capacity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
def test_a_call_that_does_not_fit_changes_nothing(form):
    rng = np.random.default_rng(7)
    st = State(1024, rand_hashes(rng, 128), balances=rng.integers(1, 1000, size=1024))
    first = ([att(st, 0, rng, j=0), att(st, 0, rng, j=1)], [0, 0])        # recent[0..64): 64 slots
    second = ([att(st, 0, rng, j=0), att(st, 1, rng, j=1)], [63, 65])     # recent[63..128): one seen + 64 new
    third = ([att(st, 0, rng, j=1)], [1])                                 # recent[1..65): one new
    calls = {}
    for name, (atts, bslots) in (("first", first), ("second", second), ("third", third)):
        status, comm, pstart = st.check(atts, bslots)
        assert (status == PROCESSED).all()
        calls[name] = (wire.attestation_columns(atts), len(atts), status, comm, pstart)
    need = len(st.oracle(st.oracle({}, *first, np.zeros(2)), *second, np.zeros(2)))
    assert need == 128
    full, twin = DeviceVoteCache(st.nval, need - 1), DeviceVoteCache(st.nval, need - 1)
    FORMS[form](full, st, *calls["first"])
    FORMS[form](twin, st, *calls["first"])
    before = snapshot(full)
    FORMS[form](full, st, *calls["second"])  # one slot more than remains
    with pytest.raises(_lib.PzError) as e:
        full.read()
    assert e.value.code == _lib.PZ_ERANGE
    with pytest.raises(_lib.PzError):
        full.voters(st.recent[0].tobytes())
    np.testing.assert_array_equal(full.read(strict=False)[0], twin.read()[0])  # nslots and keys
    assert snapshot(full, strict=False) == snapshot(twin) == before            # totals and bitmaps
    # the table too: a call that fits still finds every hash and adds its one (the error stays)
    FORMS[form](full, st, *calls["third"])
    FORMS[form](twin, st, *calls["third"])
    assert snapshot(full, strict=False) == snapshot(twin) and len(twin.items()) == 65
    with pytest.raises(_lib.PzError):
        full.items()
    fresh = DeviceVoteCache(st.nval, need)
    FORMS[form](fresh, st, *calls["first"])
    FORMS[form](fresh, st, *calls["second"])
    assert snapshot(fresh) == want(st.oracle(st.oracle({}, *first, np.zeros(2)), *second, np.zeros(2)))


# ---- 8: panics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["device", "host"])
def test_reference_panics_are_eindex(form):
    rng = np.random.default_rng(8)
    st = State(1024, rand_hashes(rng, 128))
    atts, bslots = [att(st, 1, rng, p=1.0), att(st, 2, rng, p=1.0, j=1)], [1, 2]
    status, comm, pstart = st.check(atts, bslots)
    assert (status == PROCESSED).all()
    cols = wire.attestation_columns(atts)
    # a committee member >= len(validators) (core.go:329)
    members = st.members.copy()
    members[int(st.coffs[comm[1]]) + 3] = st.nval + 5
    cache = DeviceVoteCache(st.nval, 256)
    FORMS[form](cache, st, cols, 2, status, comm, pstart, members=members)
    with pytest.raises(_lib.PzError) as e:
        cache.items()
    assert e.value.code == _lib.PZ_EINDEX
    # committee[i] >= ncomm (core.go:367): the row is dropped before anything is read through it --
    # the committee table here has exactly comm[0] + 1 entries and the members only reach that far
    ncomm = int(comm[0]) + 1
    bad = comm.copy()
    bad[1] = ncomm
    cache = DeviceVoteCache(st.nval, 256)
    FORMS[form](cache, st, cols, 2, status, bad, pstart, members=st.members[:int(st.coffs[ncomm])].copy(),
                coffs=st.coffs[:ncomm + 1].copy())
    with pytest.raises(_lib.PzError) as e:
        cache.items()
    assert e.value.code == _lib.PZ_EINDEX
    assert snapshot(cache, strict=False) == want(st.oracle({}, atts[:1], bslots[:1], status[:1]))


# ---- 9: empty and malformed arguments ----------------------------------------------------------------------------
def call(name, *args):
    return getattr(_lib.lib.dll, name)(*args)


def test_empty_batches_and_null_oblique_columns():
    import torch

    rng = np.random.default_rng(9)
    st = State(1024, rand_hashes(rng, 128))
    cache = DeviceVoteCache(st.nval, 128)
    b = _lib.VoteColsBatch()
    assert call("pz_dev_vote_cache_tally", cache._h, ctypes.byref(b), None, None) == _lib.PZ_OK
    assert call("pz_vote_cache_tally", cache._h, ctypes.byref(b)) == _lib.PZ_OK
    assert cache.items() == {} and int(_lib.lib.dll.pz_vote_cache_scratch_bytes(0, 0, 0)) % 16 == 0
    # n_oblique_total = 0 with NULL oblique columns
    atts, bslots = [att(st, 0, rng), att(st, 1, rng, j=1)], [10, 65]
    status, comm, pstart = st.check(atts, bslots)
    cols = {k: v for k, v in wire.attestation_columns(atts).items() if not k.startswith("oblique")}
    for form in ("device", "host"):
        cache = DeviceVoteCache(st.nval, 128)
        FORMS[form](cache, st, cols, 2, status, comm, pstart)
        assert snapshot(cache) == want(st.oracle({}, atts, bslots, status))
    torch.cuda.synchronize()


def test_argument_errors_are_einval():
    """Each is refused on the host, before any launch: the pointers below are never followed."""
    import torch

    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    host = np.zeros(4096, np.uint8)
    cache = DeviceVoteCache(1024, 8)
    for form, p in (("pz_dev_vote_cache_tally", buf.data_ptr()), ("pz_vote_cache_tally", host.ctypes.data)):
        def run(**kw):
            f = dict(natt=1, bits=p, boffs=p, status=p, committee=p, parents_start=p, recent=p, n_recent=64,
                     members=p, coffs=p, ncomm=1, balance=p)
            f.update(kw)
            b = _lib.VoteColsBatch(**f)
            args = (cache._h, ctypes.byref(b)) + ((p + 2048, None) if form.startswith("pz_dev") else ())
            return call(form, *args)

        for name in ("bits", "boffs", "status", "committee", "parents_start", "members", "coffs", "balance", "recent"):
            assert run(**{name: None}) == _lib.PZ_EINVAL, (form, name)
        assert run(oblique_offs=p) == _lib.PZ_EINVAL                                   # offsets without their data
        assert run(oblique_first=p, oblique_parent_hashes=p) == _lib.PZ_EINVAL         # first without offs
        assert run(n_oblique_total=1) == _lib.PZ_EINVAL                                # elements without columns
        assert run(n_oblique_total=1, oblique_parent_hashes=p, oblique_offs=p) == _lib.PZ_EINVAL
        assert run(n_recent=1 << 31) == _lib.PZ_EINVAL                                 # 2^31 sources or more
        assert run(n_recent=(1 << 31) - 5, n_oblique_total=5, oblique_parent_hashes=p, oblique_offs=p,
                   oblique_first=p) == _lib.PZ_EINVAL
        assert call(form, *((None, None) + ((None, None) if form.startswith("pz_dev") else ()))) == _lib.PZ_EINVAL
    b = _lib.VoteColsBatch(natt=1)
    assert call("pz_dev_vote_cache_tally", cache._h, ctypes.byref(b), buf.data_ptr(), None) == _lib.PZ_EINVAL
    h = ctypes.c_void_p()
    assert call("pz_vote_cache_new", 1024, 0, 0, ctypes.byref(h)) == _lib.PZ_EINVAL
    assert call("pz_vote_cache_new", 0, 8, 0, ctypes.byref(h)) == _lib.PZ_EINVAL
    assert call("pz_vote_cache_new", 1024, 8, 0, None) == _lib.PZ_EINVAL
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any() and cache.items() == {}  # nothing was written


# ---- 10: against the engine -----------------------------------------------------------------------------------
def test_tally_serialized_blocks_matches_the_engine():
    """130 blocks at 1,024 validators (two cycle transitions), block by block against the oracle
    chain's state just before each block, as test_digest_serialized_blocks_matches_the_engine
    steps: RecentBlockHashes moves with every block and the balances with every transition."""
    nval, nblocks = 1024, 130
    blocks = synth.chain_blocks(nval, nblocks, seed=4)
    data, offs = bc.serialize_blocks(blocks)
    engine = bc.BeaconChain(nval)
    engine.process_serialized(data, offs)
    chain = oreplay.Chain(nval)
    cache = DeviceVoteCache(nval, 512)
    tables = {}
    for i, blk in enumerate(blocks):
        C, A = chain.C, chain.A.data
        if C.last_state_recalc not in tables:
            tables[C.last_state_recalc] = table(C)
        lo, hi = int(offs[i]), int(offs[i + 1])
        report, first, status = bc.tally_serialized_blocks(
            cache, data[lo:hi], np.array([0, hi - lo], dtype=U64), C.last_justified_slot, C.last_state_recalc,
            len(A.recent_block_hashes), tables[C.last_state_recalc], [bytes(h) for h in A.recent_block_hashes],
            np.array([v.balance for v in C.validators], U64))
        assert list(report) == [bc.BLOCK_TALLIED], i
        assert list(first) == [0, len(blk.attestations)] and (status == PROCESSED).all()
        chain.process_block(oreplay.to_pb_block(blk))
    o_cache = chain.A.cache if chain.candidate is None else chain.candidate[1].cache
    assert len(o_cache) > 64  # (more hashes than one window holds: slots from many calls)
    assert snapshot(cache) == want(o_cache)
    assert cache.items() == engine.roots()["vote_totals"]


def test_tally_serialized_blocks_rejected_and_mixed_blocks():
    """One batch against the genesis state: a block whose attestations all pass, one whose last
    attestation fails (service.go:304-306 drops it), one whose last passes after an earlier one
    failed (the reference tallies both: left to the engine) and one without attestations."""
    rng = np.random.default_rng(10)
    st = State(1024, [rng.bytes(32) for _ in range(128)], balances=rng.integers(1, 1000, size=1024))

    def rec(slot, j, good=True):
        a = att(st, slot, rng, [rng.bytes(33)], j=j)
        return pb.AttestationRecord(slot=a.slot, shard_id=a.shard_id, justified_slot=0 if good else 9,
                                    attester_bitfield=bytes(a.attester_bitfield),
                                    oblique_parent_hashes=[bytes(h) for h in a.oblique_parent_hashes])

    def block(slot, atts):
        return pb.BeaconBlock(parent_hash=rng.bytes(32), slot_number=slot, timestamp=pb.Timestamp(8 * slot, 0), attestations=atts)

    blocks = [block(5, [rec(1, 0), rec(2, 1)]), block(6, [rec(1, 0), rec(2, 0, good=False)]),
              block(7, [rec(3, 0, good=False), rec(3, 1)]), block(8, [])]
    data, offs = bc.serialize_blocks(blocks)
    cache = DeviceVoteCache(st.nval, 256)
    report, first, status = bc.tally_serialized_blocks(cache, data, offs, 0, 0, 128, st.tab, [r.tobytes() for r in st.recent],
                                                       st.balance)
    assert list(first) == [0, 2, 4, 6, 6]
    assert list(status) == [0, 0, 0, 4, 4, 0]  # 4: PZ_ATT_JUSTIFIED
    assert list(report) == [bc.BLOCK_TALLIED, bc.BLOCK_REJECTED, bc.BLOCK_MIXED, bc.BLOCK_REJECTED]
    o_atts = oreplay.to_pb_block(blocks[0]).attestations
    assert snapshot(cache) == want(st.oracle({}, o_atts, [5, 5], [0, 0]))
    # the rejected and the mixed block alone leave a cache empty
    for b in blocks[1:3]:
        d1, o1 = bc.serialize_blocks([b])
        empty = DeviceVoteCache(st.nval, 256)
        bc.tally_serialized_blocks(empty, d1, o1, 0, 0, 128, st.tab, [r.tobytes() for r in st.recent], st.balance)
        assert empty.items() == {}
