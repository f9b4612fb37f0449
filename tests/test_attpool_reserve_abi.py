"""The pending-attestation pool's growth in the C ABI (include/prysm_hip.h, prysm_amd/csrc/attpool.hip):
the header declares the seven entry points with their citations, the binding has them with the right
restypes, the built library exports them (and no new pz_debug_* entry), the PZ_EINVAL table that
needs no device holds, and the Python face exists.  No GPU needed."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from prysm_amd import _lib
from test_blockcycle_abi import check_resident_chain_init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"pz_att_pool_capacity": "int", "pz_dev_att_pool_reserve": "int", "pz_att_pool_reserve": "int",
           "pz_att_pool_need_scratch_bytes": "uint64_t", "pz_dev_att_pool_need": "int", "pz_att_pool_need": "int",
           "pz_att_pool_view": "int"}  # (view: its text now names the reserve)
CITES = {"pz_att_pool_capacity": r"no reference counterpart", "pz_dev_att_pool_reserve": r"core\.go:223-237; types/state\.go:169",
         "pz_att_pool_reserve": r"core\.go:223-237; types/state\.go:169", "pz_att_pool_need_scratch_bytes": r"no reference counterpart",
         "pz_dev_att_pool_need": r"service\.go:299-300", "pz_att_pool_need": r"service\.go:299-300",
         "pz_att_pool_view": r"types/state\.go:164"}


def _header():
    return open(os.path.join(ROOT, "include", "prysm_hip.h")).read()


def _comment_before(src, name):
    at = re.search(r"\b%s\s+%s\(" % (ENTRIES[name], name), src).start()
    return src[src.rindex("/*", 0, at):at]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_points_resolve(name):
    src = _header()
    assert re.search(r"\b%s\s+%s\(" % (ENTRIES[name], name), src)
    assert name in _lib.SIGNATURES
    dll = ctypes.CDLL(_lib.library_path)
    assert getattr(dll, name) is not None
    want = {"int": ctypes.c_int, "uint64_t": _lib.u64}[ENTRIES[name]]
    assert _lib._RESTYPES.get(name, ctypes.c_int) is want
    m = re.search(r"\b%s\(([^;]*?)\);" % name, src, re.S)
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_entry_cites_the_reference_or_says_it_has_no_counterpart(name):
    comment = _comment_before(_header(), name)
    assert re.search(CITES[name], comment), comment


def test_the_header_says_what_ends_a_view():
    src = _header()
    assert re.search(r"valid until the next prune, reserve or free", _comment_before(src, "pz_att_pool_view"))
    assert re.search(r"valid until\s+\*?\s*the next prune, free or reserve", _comment_before(src, "pz_dev_att_pool_reserve"))
    sec = src[src.index("ActiveState.PendingAttestations resident on the device"):src.index("typedef struct pz_att_pool")]
    assert "fixed at creation" not in sec


def test_product_library_exports_them_and_no_debug_entry():
    out = subprocess.run(["nm", "-D", _lib.library_path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(ENTRIES) <= exported
    assert not [n for n in exported if n.startswith("pz_debug")]
    # the kernels are the library's own
    assert "pz_att_pool_move_kernel" in out and "pz_att_pool_need_kernel" in out


def test_einval_without_a_device():
    dll = _lib.lib.dll
    caps = np.zeros(7, dtype=np.uint64)
    need = np.full((2, 7), 9, dtype=np.uint64)
    cols = _lib.AttestationCols()
    status = np.zeros(4, dtype=np.int32)
    E = _lib.PZ_EINVAL
    assert dll.pz_att_pool_capacity(None, caps.ctypes.data) == E
    assert dll.pz_dev_att_pool_reserve(None, caps.ctypes.data, None) == E
    assert dll.pz_att_pool_reserve(None, caps.ctypes.data) == E
    assert b"null" in dll.pz_last_error()
    # need: NULL a or status with n > 0, a NULL or misaligned output, a NULL or misaligned scratch
    byref = ctypes.byref
    assert dll.pz_att_pool_need(None, 4, status.ctypes.data, None, None, need.ctypes.data) == E
    assert dll.pz_att_pool_need(byref(cols), 4, None, None, None, need.ctypes.data) == E
    assert dll.pz_att_pool_need(byref(cols), 4, status.ctypes.data, None, None, None) == E
    assert dll.pz_dev_att_pool_need(None, 4, status.ctypes.data, None, None, 4096, 4096, None) == E
    assert dll.pz_dev_att_pool_need(byref(cols), 4, None, None, None, 4096, 4096, None) == E
    assert dll.pz_dev_att_pool_need(byref(cols), 4, status.ctypes.data, None, None, None, 4096, None) == E
    assert dll.pz_dev_att_pool_need(byref(cols), 4, status.ctypes.data, None, None, 4100, 4096, None) == E
    assert dll.pz_dev_att_pool_need(byref(cols), 4, status.ctypes.data, None, None, 4096, None, None) == E
    assert dll.pz_dev_att_pool_need(byref(cols), 4, status.ctypes.data, None, None, 4096, 4104, None) == E
    assert dll.pz_dev_att_pool_need(byref(cols), 0, None, None, None, None, 4096, None) == E
    # offsets without their data column
    offs = np.zeros(5, dtype=np.uint64)
    bad = _lib.AttestationCols(attester_bitfield_offs=offs.ctypes.data)
    assert dll.pz_att_pool_need(byref(bad), 4, status.ctypes.data, None, None, need.ctypes.data) == E
    assert dll.pz_dev_att_pool_need(byref(bad), 4, status.ctypes.data, None, None, 4096, 4096, None) == E
    # no row: zeros, and nothing is launched by the host form
    assert dll.pz_att_pool_need(None, 0, None, None, None, need.ctypes.data) == _lib.PZ_OK
    assert not need.any()
    assert dll.pz_att_pool_need_scratch_bytes(0) >= 16
    assert dll.pz_att_pool_need_scratch_bytes(513) >= 2 * 7 * 3 * 8


def test_python_face():
    from prysm_amd import blockchain, pending
    for name in ("reserve", "capacity", "need_columns", "need_host"):
        assert callable(getattr(pending.DevicePendingAttestations, name)), name
    assert list(inspect.signature(pending.DevicePendingAttestations.reserve).parameters) == ["self", "min_caps", "device_form"]
    assert "fixed for the pool's lifetime" not in pending.DevicePendingAttestations.__doc__
    assert "reserve" in pending.DevicePendingAttestations.view.__doc__
    RC = blockchain.ResidentChain
    assert RC.POOL_POLICIES == ("fixed", "grow")
    check_resident_chain_init(RC)
    assert inspect.signature(RC.from_state).parameters["pool_policy"].default == "fixed"
    # an unknown policy is refused before any object is made (the arguments are never looked at)
    with pytest.raises(_lib.PzError) as e:
        RC(None, None, None, None, None, None, pool_policy="shrink")
    assert e.value.code == _lib.PZ_EINVAL
