"""tests/attcheck_cases.py on the CPU: its model of processAttestation's checks against the scalar
oracle (oracle/ref.py) and the C port (oracle/c/attcheck_ref.c), and its builders against what they
claim to cover.  Oracle against oracle: no kernel runs here."""
import os
import re

import numpy as np
import pytest

import attcheck_cases as ac
from oracle import ref
from oracle import schema as opb
from test_attcheck_gpu import oracle_code

GROUPS = ac.groups()
# a committee of 2^32 + 5 members and inverted offsets cannot be written down as a CrystallizedState
ORACLE_GROUPS = [n for n in GROUPS if n not in ("huge_committee", "inverted")]


def states_of(st):
    t = st.table
    arrs = [opb.ShardAndCommitteeArray(array_shard_and_committee=[
        opb.ShardAndCommittee(shard_id=t.arr_shard[e], committee=range(t.sizes[t.arr_comm[e]])) for e in t.entries(a)])
        for a in range(t.narr)]
    cstate = opb.CrystallizedState(last_state_recalc=st.lsr, last_justified_slot=st.ljs, shard_and_committees_for_slots=arrs)
    astate = opb.ActiveState(recent_block_hashes=[bytes(32)] * st.n_recent)
    return cstate, astate


@pytest.mark.parametrize("name", ORACLE_GROUPS)
def test_model_matches_scalar_oracle(name):
    g = GROUPS[name]
    cstate, astate = states_of(g.st)
    ran = 0
    for c, want in zip(g.cases, g.want):
        if max(c.s, c.bs, c.js, c.nob, c.shard) >> 63:
            continue
        att = opb.AttestationRecord(slot=c.s, shard_id=c.shard, justified_slot=c.js, attester_bitfield=c.bits,
                                    oblique_parent_hashes=[bytes(32)] * c.nob)
        assert oracle_code(cstate, astate, c.bs, att) == want[0], c
        if want[1] != ac.NONE:  # the committee the model names is the one the oracle finds
            assert list(range(g.st.table.sizes[want[1]])) == ref.get_attester_indices(cstate, att), c
        ran += 1
    assert ran >= 30  # (the window's cases around 2^63 and above are the port's alone)


@pytest.mark.parametrize("name", list(GROUPS))
def test_model_matches_c_port(name):
    """Every case, the huge slots included: Go's int(bs) - 64 wraps for bs in [2^63, 2^63 + 63]."""
    g = GROUPS[name]
    got = ac.port_status(ac.batch(g.cases), g.st)
    bad = [(c, int(s), w[0]) for c, s, w in zip(g.cases, got, g.want) if s != w[0]]
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", list(GROUPS))
def test_vectorised_model_matches_model(name):
    """model_np (the reference of the grid-stride test) states the same rule, also when the
    trailing-bits byte comes from the last_byte column and not from the bitfields."""
    g = GROUPS[name]
    for rot in (0, 1):
        cases = g.cases[-rot:] + g.cases[:-rot] if rot else g.cases
        want = [ac.model(c, g.st) for c in cases]
        for compl in (False, True):
            cols = ac.batch(cases, complement_last=compl)
            st, comm, ps = ac.model_np(cols, g.st, cols["last_byte"] if compl else None)
            assert [(int(a), int(b), int(c)) for a, b, c in zip(st, comm, ps)] == want
        # and read from complemented bitfields the answers change: the two sources are told apart
        st, _, _ = ac.model_np(ac.batch(cases, complement_last=True), g.st)
        if not g.partial:
            assert (st != np.array([w[0] for w in want])).any()


def test_last_byte_of_an_empty_bitfield_is_poison():
    g = GROUPS["plain"]
    cols = ac.batch(g.cases, complement_last=True)
    empty = cols["boffs"][1:] == cols["boffs"][:-1]
    assert empty.any() and (cols["last_byte"][empty] == 0xFF).all()
    assert cols["boffs"][0] == cols["boffs"][1] == 0  # k = 0, blen = 0 first: no byte to read


@pytest.mark.parametrize("name", list(GROUPS))
def test_every_status_in_every_group(name):
    g = GROUPS[name]
    seen = {w[0] for w in g.want}
    if g.partial:
        assert seen == {ac.SLOT_HIGH, ac.SLOT_LOW, ac.JUSTIFIED, ac.ERANGE, ac.EINDEX}, g.partial
    else:
        assert seen == ac.STATUSES
        # and with the first or the last row taken off (the device tests run prefixes and a rotation)
        assert {w[0] for w in g.want[1:-1]} == ac.STATUSES
    assert len({c.name for c in g.cases}) == len(g.cases) < 400


def by_tag(g, tag):
    rows = [(c, w) for c, w in zip(g.cases, g.want) if tag in c.tags]
    assert rows, "%s: no case tagged %r" % (g.name, tag)
    return rows


def statuses(g, tag):
    return {w[0] for _, w in by_tag(g, tag)}


@pytest.mark.parametrize("name", [n for n in GROUPS if not GROUPS[n].partial])
def test_bitfield_edges(name):
    g = GROUPS[name]
    for r in range(1, 8):
        for bit in range(8):
            (c, w), = by_tag(g, ("r_bit", r, bit))
            assert c.bits == bytes([1 << bit])
            assert w[0] == (ac.TRAILING if bit < 8 - r else ac.PROCESSED), c
    assert statuses(g, "r0_ff") == {ac.PROCESSED}
    assert statuses(g, "k0_blen0") == {ac.PROCESSED}
    assert g.cases[0].bits == g.cases[-1].bits == b"" and g.want[0][0] == g.want[-1][0] == ac.PROCESSED
    assert statuses(g, "blen-need=0") == {ac.PROCESSED}
    for tag in ("blen-need=1", "blen-need=-1", "blen0"):
        assert statuses(g, tag) == {ac.BITFIELD_LEN}
    ks = {int(m.group(1)) for c in g.cases for m in [re.match(r"bits_k(\d+)_blen", c.name)] if m}
    assert ks == set(ac.KS) == set(range(18)) | {204, 205}


@pytest.mark.parametrize("name", list(GROUPS))
def test_window_justified_slice_and_index_edges(name):
    g = GROUPS[name]
    window = {(c.s, c.bs): w[0] for c, w in zip(g.cases, g.want) if c.name.startswith("window_")}
    assert {bs for _, bs in window} == set(ac.BS_EDGES)
    for bs in ac.BS_EDGES:
        assert {(bs + x) & ac.M64 for x in (0, 1, -64, -65)} | {0, 1 << 63, ac.M64} == {s for s, b in window if b == bs}
    notwin = {ac.SLOT_HIGH, ac.SLOT_LOW}
    # both sides of s == bs - 64, where no int wraps on the way
    assert window[(136, 200)] not in notwin and window[(135, 200)] == ac.SLOT_LOW
    assert window[(0, 64)] not in notwin and window[(ac.M64, 64)] == ac.SLOT_LOW  # 64 - 65: int(s) == -1 < 0
    assert window[(1, 65)] not in notwin and window[(0, 65)] == ac.SLOT_LOW
    assert window[(201, 200)] == ac.SLOT_HIGH and window[(200, 200)] not in notwin
    # bs < 64: int(bs) - 64 is negative, slot 0 passes
    assert all(w[0] not in notwin for _, w in by_tag(g, "s0_bs<64")) and len(by_tag(g, "s0_bs<64")) == 3
    assert statuses(g, "low_not_high") == {ac.SLOT_LOW}
    assert statuses(g, "minus_one_over_zero") == ({ac.EINDEX} if g.st.n_recent >= 65 else {ac.ERANGE})
    # bs in [2^63, 2^63 + 63]: int(bs) - 64 wraps to a huge positive number, every slot <= bs is too low
    for c, w in by_tag(g, "bs-64_wraps"):
        assert w[0] in notwin and (w[0] == ac.SLOT_LOW) == (ac.i64(c.s) <= ac.i64(c.bs)), c
    assert window[(1 << 63, 1 << 63)] == window[((1 << 63) + 63, (1 << 63) + 63)] == ac.SLOT_LOW
    assert window[((1 << 63) + 64, (1 << 63) + 64)] not in notwin and window[(1 << 63, (1 << 63) + 64)] not in notwin
    for tag in ("justified_ljs-1", "justified_ljs+1", "justified_ljs+2^32"):
        assert statuses(g, tag) == {ac.JUSTIFIED}
    n = g.st.n_recent
    assert (ac.ERANGE in statuses(g, "end==128")) == (n < 128)
    assert ac.ERANGE not in statuses(g, "end==n_recent")
    if n < 128:  # (129 hashes would need bs - s == 65, which the window refuses)
        assert statuses(g, "end==n_recent+1") == {ac.ERANGE}
    assert ac.ERANGE not in statuses(g, "nob64_d0") and (ac.ERANGE in statuses(g, "nob64_d10")) == (n < 10)
    assert statuses(g, "nob65_d0") == statuses(g, "nob65_d10") == {ac.ERANGE}
    (c, _), = by_tag(g, "nob65_d10")
    assert c.bs - c.s == 10 and c.nob == 65  # start 10 > end 9: where n_recent >= 9, by start > end alone
    (c, _), = by_tag(g, "nob65_d0")
    assert (c.bs - c.s - c.nob + 64) & ac.M64 == ac.M64  # start 0 <= end: by end > n_recent alone
    assert statuses(g, "erange_and_eindex") == {ac.ERANGE}
    assert statuses(g, "s<lsr") == statuses(g, "idx==narr") == {ac.EINDEX}
    if g.st.table.narr:
        assert ac.EINDEX not in statuses(g, "idx==narr-1") and ac.ERANGE not in statuses(g, "idx==narr-1")


def test_slice_edges_across_groups():
    """end == 128 is accepted with 128 recent hashes and refused with 127; n_recent is one of
    128, 127, 100, 64, 0 in some group."""
    assert {g.st.n_recent for g in GROUPS.values()} == {128, 127, 100, 64, 0}
    assert statuses(GROUPS["plain"], "end==128") == {ac.PROCESSED} and statuses(GROUPS["lsr64"], "end==128") == {ac.ERANGE}
    assert {g.st.lsr for g in GROUPS.values()} >= {0, 1, 64}


def test_lookup_edges():
    g = GROUPS["plain"]
    t = g.st.table
    want = {"empty_array": ac.NO_COMMITTEE, "neighbour_only_below": ac.NO_COMMITTEE, "neighbour_only_above": ac.NO_COMMITTEE,
            "shard_plus_2_32": ac.NO_COMMITTEE, "shard0_absent": ac.NO_COMMITTEE, "in_its_array": ac.PROCESSED,
            "first_entry_shard0": ac.PROCESSED, "last_entry": ac.PROCESSED, "duplicate_shard": ac.PROCESSED}
    for k, v in want.items():
        assert statuses(g, "lookup_" + k) == {v}, k
    (c, w), = by_tag(g, "lookup_duplicate_shard")
    assert [t.arr_shard[e] for e in t.entries(2)].count(c.shard) == 2 and w[1] == 5  # the first entry's committee
    (c, w), = by_tag(g, "lookup_first_entry_shard0")
    assert c.shard == 0 and t.arr_shard[0] == 0
    (c, w), = by_tag(g, "lookup_last_entry")
    assert t.find(0, c.shard) == t.arr_offs[1] - 1
    # committees are shared and their ids are not the entries' numbers, nor monotone
    assert t.arr_comm != sorted(t.arr_comm) and len(set(t.arr_comm)) < len(t.arr_comm)
    assert all(t.arr_comm[e] != e for e in (0, 19)) and w[1] == t.arr_comm[19] != 19
    for name in ("lds_limit", "over_limit", "wide"):
        g = GROUPS[name]
        (c, w), = by_tag(g, "lookup_tables_last_entry")
        t = g.st.table
        assert w[0] == ac.PROCESSED and t.find(t.narr - 1, c.shard) == t.ne - 1
    assert statuses(GROUPS["over_limit"], "lookup_empty_array") == {ac.NO_COMMITTEE}
    assert statuses(GROUPS["big_shard"], "lookup_big_shard_exact") == {ac.PROCESSED}
    assert statuses(GROUPS["big_shard"], "lookup_big_shard_low_half") == {ac.NO_COMMITTEE}
    (c, w), = by_tag(GROUPS["huge_committee"], "huge_committee")
    assert w[0] == ac.BITFIELD_LEN and len(c.bits) == 1
    assert ac.model(c, ac.State(5, 0, 128, ac.Table("t", [[(c.shard, 5)]] * 5)))[0] == ac.PROCESSED  # a size cut to 32 bits
    g = GROUPS["inverted"]
    assert statuses(g, "lookup_inverted_reads_empty") == statuses(g, "lookup_inverted_reads_empty_2") == {ac.NO_COMMITTEE}
    assert not g.host_form and all(GROUPS[n].host_form for n in GROUPS if n != "inverted")


def test_tables_take_the_intended_walk():
    """Which groups the paired kernel walks in LDS and which in global memory, and why."""
    fits = {n: g.st.table.fits_lds for n, g in GROUPS.items()}
    assert fits == {"plain": True, "lsr64": True, "lds_limit": True, "narr0": True, "wide": False, "over_limit": False,
                    "big_shard": False, "huge_committee": False, "inverted": False}
    t = {n: g.st.table for n, g in GROUPS.items()}
    assert (t["lds_limit"].words, t["lds_limit"].narr, t["lds_limit"].ne) == (12288, 2, 4095)
    assert (t["over_limit"].words, t["over_limit"].narr, t["over_limit"].ne) == (12289, 3, 4095)
    assert (t["wide"].narr, {len(t["wide"].entries(a)) for a in range(256)}) == (256, {16})
    # each of the other three leaves the LDS walk for one reason only
    assert t["big_shard"].words < 12288 and sum(s >> 32 != 0 for s in t["big_shard"].arr_shard) == 1
    assert all(s >> 32 == 0 for s in t["huge_committee"].arr_shard) and t["huge_committee"].sizes[-1] == (1 << 32) + 5
    assert all(s >> 32 == 0 for s in t["inverted"].arr_shard) and max(t["inverted"].sizes) < 1 << 32
    # no case reads outside a buffer: every offset lies in the table, every committee id in coffs
    for tb in t.values():
        assert all(0 <= o <= tb.ne for o in tb.arr_offs) and tb.arr_offs[-1] == tb.ne == len(tb.arr_shard) == len(tb.arr_comm)
        assert all(c + 1 < len(tb.coffs) for c in tb.arr_comm)


def test_kernel_constants():
    """The sizes of the grid-stride test and of the two limit tables follow the kernel's constants."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "prysm_amd", "csrc",
                            "attcheck.hip")).read()
    val = {k: int(re.search(r"\b%s\s*=\s*(\d+)" % k, src).group(1)) for k in ("kPThreads", "kPBlocksPerCU", "kPTabWords")}
    assert val == {"kPThreads": ac.P_THREADS, "kPBlocksPerCU": ac.P_BLOCKS_PER_CU, "kPTabWords": ac.LDS_WORDS}
    assert ac.stride_rows(256) == 2 * 3 * 256 * 512 and ac.stride_natt(256) == 2 * ac.stride_rows(256) + 2 * 512 + 3


def test_mixture_holds_every_status_and_the_port_agrees():
    st = GROUPS["plain"].st
    names = ("high", "low", "justified", "erange", "eindex", "no_committee", "len", "trailing", "plus32")
    pinned = [(j, names[j % 9]) for j in (0, 1, 4998, 4999)]
    cols = ac.mixture(5000, st, seed=3, pinned=pinned)
    status, comm, ps = ac.model_np(cols, st)
    assert set(status.tolist()) == ac.STATUSES
    assert [int(status[j]) for j, _ in pinned] == [ac.SLOT_HIGH, ac.SLOT_LOW, ac.ERANGE, ac.EINDEX]
    assert (status == ac.PROCESSED).mean() > 0.5
    np.testing.assert_array_equal(status, ac.port_status(cols, st))
    cases = [ac.Case("m", int(cols["slot"][i]), int(cols["block_slot"][i]), int(cols["justified_slot"][i]),
                     int(cols["n_oblique"][i]), int(cols["shard_id"][i]),
                     cols["bits"][int(cols["boffs"][i]):int(cols["boffs"][i + 1])].tobytes()) for i in range(5000)]
    assert [ac.model(c, st) for c in cases] == list(zip(status.tolist(), comm.tolist(), ps.tolist()))
    assert ((comm == ac.NONE) == np.isin(status, (ac.SLOT_HIGH, ac.SLOT_LOW, ac.JUSTIFIED, ac.ERANGE, ac.EINDEX,
                                                  ac.NO_COMMITTEE))).all()
