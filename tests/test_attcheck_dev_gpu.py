"""pz_dev_check_attestations and pz_check_attestations (prysm_amd/csrc/attcheck.hip) against the
plain model of tests/attcheck_cases.py on all three outputs, in every form the launch can take:

  lane    the one-per-lane kernel: every column and output 8 bytes (status, committee: 4; last_byte: 1)
          off its 16-B alignment
  paired  the two-per-lane persistent kernel, its committee walk in LDS or in global memory as the
          group's table decides (attcheck_cases.Table.fits_lds)
  tail    the paired kernel's odd tail: batches of three rows, the case last
  host    pz_check_attestations over host memory

Every case sits at an even and at an odd row (the batch rotated by one).  Every form runs with
last_byte NULL and with the column given; when it is given, the bitfields' own last bytes are
complemented, so the column alone must decide.  Outputs are carved out of sentinel-filled buffers
with eight entries of guard on either side, and every entry outside the rows written must keep the
sentinel.  One large batch takes the paired kernel's lanes two and three times round their loop."""
import ctypes

import numpy as np
import pytest
import torch

import attcheck_cases as ac
from prysm_amd import _lib

pytestmark = pytest.mark.gpu

GROUPS = ac.groups()
G = 8  # guard entries on either side of an output
OUTS = (("status", np.int32, 0x5A5A5A5A), ("committee", np.uint32, 0x5A5A5A5A), ("parents_start", np.uint64, 0x5A5A5A5A5A5A5A5A))
SIGNED = {np.int32: np.int32, np.uint32: np.int32, np.uint64: np.int64}  # (torch has no unsigned 32/64-bit types)
COLS = ("slot", "justified_slot", "shard_id", "n_oblique", "block_slot", "boffs")
TABLE = ("arr_offs", "arr_shard", "arr_comm", "coffs")


def call(b, host=False):
    if host:
        return _lib.lib.call("pz_check_attestations", ctypes.byref(b) if b is not None else None)
    return _lib.lib.call("pz_dev_check_attestations", ctypes.byref(b) if b is not None else None, _lib.stream_ptr(0))


@pytest.fixture(autouse=True)
def device_checks():
    """After every test: wait for the device (a fault surfaces here) and make one more call, whose
    return code is the library's hipGetLastError path.  A device error ends the session: nothing
    more is started on a device that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
        call(_lib.AttCheckBatch(natt=0))
        torch.cuda.synchronize()
    except (RuntimeError, _lib.PzError) as e:
        pytest.exit("the device reported an error, no further test is run on it: %s" % e, returncode=3)


def place(arr, shift, host):
    """``arr`` inside 0xA5 poison, two entries (plus ``shift``) in: (what keeps it alive, its address).
    On the device the address is 16-B aligned exactly when ``shift`` is 0 and the entries are 8 bytes."""
    item = arr.itemsize
    off = (2 + shift) * item
    buf = np.full(arr.nbytes + 4 * item + 16, 0xA5, dtype=np.uint8)
    buf[off:off + arr.nbytes] = np.ascontiguousarray(arr).view(np.uint8)
    if host:
        return buf, buf.ctypes.data + off
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off


class Out:
    """The three outputs for ``n`` rows, sentinel-filled with G entries of guard on either side, and what
    they must hold afterwards: the sentinel wherever ``expect`` has not put a value."""

    def __init__(self, n, shift=0, host=False):
        self.lo, self.host = G + shift, host
        self.exp = {k: np.full(n + 2 * G + 2, s, dtype=dt) for k, dt, s in OUTS}
        self.mem = {k: v.copy() if host else torch.from_numpy(v.view(SIGNED[dt])).cuda()
                    for (k, dt, _), v in zip(OUTS, self.exp.values())}
        if not host:
            assert all(m.data_ptr() % 16 == 0 for m in self.mem.values())

    def addr(self, k, at=0):
        m = self.mem[k]
        return (m.ctypes.data if self.host else m.data_ptr()) + (self.lo + at) * self.exp[k].itemsize

    def expect(self, want, n, at=0, src=0, only=None):
        for k in only or self.exp:
            self.exp[k][self.lo + at:self.lo + at + n] = want[k][src:src + n]

    def verify(self):
        for k, dt, _ in OUTS:
            got = self.mem[k] if self.host else self.mem[k].cpu().numpy().view(dt)
            bad = np.flatnonzero(got != self.exp[k])
            if len(bad):
                i = int(bad[0])
                where = "row %d" % (i - self.lo) if self.lo <= i else "the guard in front"
                pytest.fail("%s differs at %s (%d entries differ): got %#x, want %#x" % (
                    k, where, len(bad), int(got[i]) & ac.M64, int(self.exp[k][i]) & ac.M64))


class Data:
    """A batch as columns, its table and the model's three outputs; placed on the host or the device
    on first use and kept."""

    def __init__(self, st, cols, want):
        self.st, self.n, self.want = st, len(cols["slot"]), want
        self.cols = {False: cols, True: ac.complemented(cols)}
        self.tab = st.table.arrays_np()
        self.mem = {}

    def addr(self, key, arr, shift, host):
        k = (key, shift, host)
        if k not in self.mem:
            self.mem[k] = place(arr, shift, host)
        return self.mem[k][1]

    def struct(self, out, natt=None, row0=0, at=0, lastb=False, shift=0, host=False, null=()):
        """The pz_att_check_batch of rows row0 .. row0 + natt, written to ``out`` from entry ``at`` on.
        ``lastb``: the last_byte column is given and ``bits`` holds complemented last bytes."""
        c, st = self.cols[lastb], self.st
        f = {k: self.addr(k, c[k], shift, host) + 8 * row0 for k in COLS}
        f["bits"] = self.addr(("bits", lastb), c["bits"], 0, host)
        f["last_byte"] = self.addr("last_byte", c["last_byte"], shift, host) + row0 if lastb else None
        for k in TABLE:  # (no array: no table, the pointers are NULL)
            f[k] = self.addr(k, self.tab[k], 0, host) if st.table.narr else None
        for k, _, _ in OUTS:
            f[k] = out.addr(k, at)
        for k in null:
            f[k] = None
        return _lib.AttCheckBatch(natt=self.n - row0 if natt is None else natt, last_justified_slot=st.ljs,
                                  last_state_recalc=st.lsr, n_recent=st.n_recent, narr=st.table.narr, **f)


def want_of(rows):
    return {k: np.array([w[j] for w in rows], dtype=dt) for j, (k, dt, _) in enumerate(OUTS)}


_data = {}


def data_for(name, layout, rot=0):
    """The group's cases as a batch (built and uploaded once).  ``layout``: "rot" (rotated by ``rot``),
    "tail" (2 + rot rows in front, so that every case sits at an even row >= 2 for one ``rot``) or
    "x5" (five times over: 1,025 rows and more)."""
    key = (name, layout, rot)
    if key not in _data:
        g = GROUPS[name]
        c = g.cases
        rows = {"rot": c[-rot:] + c[:-rot] if rot else c, "tail": c[-(2 + rot):] + c, "x5": c * 5}[layout]
        _data[key] = Data(g.st, ac.batch(rows), want_of([ac.model(x, g.st) for x in rows]))
    return _data[key]


def run_form(d, form, lastb, natt=None, null=()):
    """One call of ``form`` over the first ``natt`` rows of ``d`` -> the outputs and what they must hold."""
    natt = d.n if natt is None else natt
    host, shift = form == "host", 1 if form == "lane" else 0
    out = Out(natt, shift, host)
    call(d.struct(out, natt=natt, lastb=lastb, shift=shift, host=host, null=null), host)
    out.expect(d.want, natt, only=[k for k, _, _ in OUTS if k not in null])
    return out


FORMS = ("lane", "paired", "tail", "host")
CASE_PARAMS = [(n, f) for n in GROUPS for f in FORMS if f != "host" or GROUPS[n].host_form]


@pytest.mark.parametrize("lastb", [False, True], ids=["bits", "last_byte"])
@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("name,form", CASE_PARAMS)
def test_cases_match_model(name, form, rot, lastb):
    if form != "tail":
        run_form(data_for(name, "rot", rot), form, lastb).verify()
        return
    d = data_for(name, "tail", rot)
    tails = range(2, d.n, 2)  # (an even row: the three rows' columns stay 16-B aligned)
    assert len(tails) * 2 + 1 >= len(GROUPS[name].cases)
    out = Out(4 * len(tails))
    for slot, j in enumerate(tails):  # four entries per call: three results and one that must stay
        call(d.struct(out, natt=3, row0=j - 2, at=4 * slot, lastb=lastb))
        out.expect(d.want, 3, at=4 * slot, src=j - 2)
    out.verify()


GUARD_FORMS = {"lane": ("plain", "lane"), "lds": ("plain", "paired"), "global": ("big_shard", "paired"), "host": ("lsr64", "host")}


@pytest.mark.parametrize("natt", [1, 2, 3, 511, 512, 513, 1023, 1025])
@pytest.mark.parametrize("which", list(GUARD_FORMS))
def test_nothing_written_outside_natt(which, natt):
    """A prefix of a longer batch: rows [0, natt) are written (one row: the one-per-lane kernel; an
    odd count: the paired kernel's tail), nothing in front and nothing from natt on."""
    name, form = GUARD_FORMS[which]
    d = data_for(name, "x5")
    assert d.n >= 1025 + G and GROUPS[name].st.table.fits_lds == (which != "global")
    run_form(d, form, True, natt=natt).verify()


@pytest.mark.parametrize("null", [("committee",), ("parents_start",), ("committee", "parents_start")], ids="+".join)
@pytest.mark.parametrize("which", list(GUARD_FORMS) + ["tail"])
def test_optional_outputs(which, null):
    name, form = GUARD_FORMS.get(which, ("plain", "paired"))
    d = data_for(name, "rot", 1)
    natt = 3 if which == "tail" else d.n - 1 + d.n % 2  # (odd: the paired forms end in a tail)
    run_form(d, form, False, natt=natt, null=null).verify()


@pytest.mark.parametrize("field", COLS + ("status",) + TABLE + ("batch",))
@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
def test_required_null_is_einval(host, field):
    d = data_for("plain", "rot", 0)
    out = Out(d.n, 0, host)
    b = None if field == "batch" else d.struct(out, host=host, null=(field,))
    with pytest.raises(_lib.PzError) as err:
        call(b, host)
    assert err.value.code == _lib.PZ_EINVAL
    if not host:
        torch.cuda.synchronize()
    out.verify()  # nothing was launched


@pytest.mark.parametrize("host", [False, True], ids=["dev", "host"])
def test_empty_batch_touches_nothing(host):
    d = data_for("plain", "rot", 0)
    out = Out(d.n, 0, host)
    assert call(d.struct(out, natt=0, host=host), host) == _lib.PZ_OK
    assert call(_lib.AttCheckBatch(natt=0), host) == _lib.PZ_OK  # and needs no column
    out.verify()


def test_no_array_needs_no_table():
    """narr == 0: the table's four pointers may be NULL (check_args asks for them only when narr > 0);
    every row that reaches the index is PZ_EINDEX, in every form."""
    d = data_for("narr0", "rot", 0)
    assert d.struct(Out(1)).arr_offs is None
    assert set(d.want["status"].tolist()) == {ac.SLOT_HIGH, ac.SLOT_LOW, ac.JUSTIFIED, ac.ERANGE, ac.EINDEX}
    for form in ("lane", "paired", "host"):
        run_form(d, form, True, natt=d.n - 1 + d.n % 2).verify()


def test_grid_stride_loop():
    """natt = 2 (2 x 3 CUs x 512) + 2 x 512 + 3: the grid is full (3 blocks per CU), the first 512 lanes
    go three times round the paired kernel's loop, the others twice, and the tail runs.  Rows one
    stride apart differ, and the first and last row of each stride segment fail a known check."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stride, natt = ac.stride_rows(cus), ac.stride_natt(cus)
    st = GROUPS["plain"].st
    names = ("high", "low", "justified", "erange", "eindex", "no_committee", "len")
    edges = (0, stride - 1, stride, 2 * stride - 1, 2 * stride, natt - 2, natt - 1)
    codes = (ac.SLOT_HIGH, ac.SLOT_LOW, ac.JUSTIFIED, ac.ERANGE, ac.EINDEX, ac.NO_COMMITTEE, ac.BITFIELD_LEN)
    cols = ac.mixture(natt, st, seed=natt, pinned=list(zip(edges, names)))
    status, comm, pstart = ac.model_np(cols, st)
    assert set(status.tolist()) == ac.STATUSES and [int(status[r]) for r in edges] == list(codes)
    np.testing.assert_array_equal(status, ac.port_status(cols, st))  # the status is the C port's
    for j in (1, 2):  # rows one and two strides apart are not copies of each other
        assert (status[j * stride:j * stride + 1024] != status[:1024]).mean() > 0.2
        assert (pstart[j * stride:j * stride + 1024] != pstart[:1024]).mean() > 0.5
    d = Data(st, cols, dict(status=status, committee=comm, parents_start=pstart))
    for lastb in (True, False):
        run_form(d, "paired", lastb).verify()
