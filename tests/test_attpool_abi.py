"""The pending-attestation pool's C ABI (include/prysm_hip.h, prysm_amd/csrc/attpool.hip): the
header declares its entry points, the binding has them with the right restypes, the built library
exports them (and no new pz_debug_* entry), and the Python face exists.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import pytest

from prysm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"pz_att_pool_new": "int", "pz_att_pool_free": "void", "pz_att_pool_scratch_bytes": "uint64_t",
           "pz_dev_att_pool_append": "int", "pz_att_pool_append": "int", "pz_dev_att_pool_prune": "int",
           "pz_att_pool_counts": "int", "pz_att_pool_view": "int", "pz_att_pool_read": "int",
           "pz_att_pool_shard_block_hashes": "int"}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_points_resolve(name):
    src = open(os.path.join(ROOT, "include", "prysm_hip.h")).read()
    assert re.search(r"\b%s\s+%s\(" % (ENTRIES[name], name), src)
    assert name in _lib.SIGNATURES
    dll = ctypes.CDLL(_lib.library_path)
    assert getattr(dll, name) is not None
    want = {"int": ctypes.c_int, "void": None, "uint64_t": _lib.u64}[ENTRIES[name]]
    assert _lib._RESTYPES.get(name, ctypes.c_int) is want


def test_argument_counts_match_the_header():
    src = open(os.path.join(ROOT, "include", "prysm_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"\b%s\(([^;]*?)\);" % name, src, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name


def test_product_library_has_no_pool_debug_entry():
    out = subprocess.run(["nm", "-D", _lib.library_path], capture_output=True, text=True, check=True).stdout
    assert "pz_att_pool_new" in out
    assert not [ln for ln in out.splitlines() if "pz_debug_att_pool" in ln]


def test_every_entry_cites_its_reference_line():
    src = open(os.path.join(ROOT, "include", "prysm_hip.h")).read()
    sec = src[src.index("ActiveState.PendingAttestations resident on the device"):src.index("typedef struct pz_block_result")]
    for name in ENTRIES:
        at = sec.index(name + "(")
        comment = sec[sec.rindex("/*", 0, at):at]
        assert re.search(r"\.go:\d+|no reference counterpart|No device call", comment), name


def test_python_face_exists():
    from prysm_amd import blockchain, pending
    for name in ("append_columns", "append_host", "prune", "counts", "columns", "records", "wire", "shard_block_hashes",
                 "epoch_batch"):
        assert hasattr(pending.DevicePendingAttestations, name), name
    assert callable(blockchain.pend_serialized_blocks) and callable(blockchain.state_recalc_device)
    assert hasattr(pending, "RecalcState")
    import inspect
    sig = inspect.signature(blockchain.tally_serialized_blocks)
    assert sig.parameters["pending"].default is None and sig.parameters["candidate"].default is None
