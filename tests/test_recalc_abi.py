"""The resident transition's C ABI (include/prysm_hip.h, prysm_amd/csrc/recalc.hip and the vote
cache's lookup in votecache.hip): the header declares its entry points, the binding has them with
the right restypes, the built library exports them (and no new pz_debug_* entry),
pz_recalc_batch -- passed by pointer from ctypes -- has the header's field order, and the Python
face exists.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import pytest

from prysm_amd import _lib
from test_attdigest_abi import header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"pz_dev_vote_cache_lookup": "int", "pz_vote_cache_lookup": "int", "pz_recalc_state_new": "int",
           "pz_recalc_state_free": "void", "pz_recalc_state_read": "int", "pz_state_recalc_scratch_bytes": "uint64_t",
           "pz_dev_state_recalc": "int"}


def header():
    return open(os.path.join(ROOT, "include", "prysm_hip.h")).read()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_points_resolve(name):
    assert re.search(r"\b%s\s+%s\(" % (ENTRIES[name], name), header())
    assert name in _lib.SIGNATURES
    dll = ctypes.CDLL(_lib.library_path)
    assert getattr(dll, name) is not None
    want = {"int": ctypes.c_int, "void": None, "uint64_t": _lib.u64}[ENTRIES[name]]
    assert _lib._RESTYPES.get(name, ctypes.c_int) is want


def test_argument_counts_match_the_header():
    src = header()
    for name in ENTRIES:
        m = re.search(r"\b%s\(([^;]*?)\);" % name, src, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name


def test_product_library_has_no_recalc_debug_entry():
    out = subprocess.run(["nm", "-D", _lib.library_path], capture_output=True, text=True, check=True).stdout
    assert "pz_dev_state_recalc" in out and "pz_dev_vote_cache_lookup" in out
    assert not [ln for ln in out.splitlines() if "pz_debug_state_recalc" in ln or "pz_debug_vote_cache_lookup" in ln]


def test_every_entry_cites_its_reference_line():
    src = header()
    for name in ENTRIES:
        at = src.index(name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        assert re.search(r"\.go:\d+|no reference counterpart", comment), name


def test_recalc_batch_layout():
    fields = header_fields("pz_recalc_batch")
    assert [f for _, f in fields] == [f for f, _ in _lib.RecalcBatch._fields_]
    for (ctype, name), (_, t) in zip(fields, _lib.RecalcBatch._fields_):
        if "*" in ctype:
            assert t is _lib.vp, name
        else:  # every member is a pointer or a uint64_t: no padding to get wrong
            assert ctype == "uint64_t" and t is _lib.u64, name
    assert len(fields) == 9 and ctypes.sizeof(_lib.RecalcBatch) == 72


def test_scalar_indices_match_the_header():
    src = header()
    for name in ("LAST_STATE_RECALC", "JUSTIFIED_STREAK", "LAST_JUSTIFIED_SLOT", "LAST_FINALIZED_SLOT", "CURRENT_DYNASTY",
                 "TOTAL_DEPOSITS", "COUNT"):
        m = re.search(r"#define PZ_RS_%s\s+(\d+)" % name, src)
        assert m and int(m.group(1)) == getattr(_lib, "RS_" + name), name


def test_python_face_exists():
    from prysm_amd import blockchain, pending, votes
    assert callable(votes.DeviceVoteCache.lookup) and callable(votes.DeviceVoteCache.lookup_device)
    for name in ("read", "balances", "crosslink_records", "winners", "last_state_recalc", "justified_streak",
                 "last_justified_slot", "last_finalized_slot", "current_dynasty", "total_deposits"):
        assert hasattr(pending.ResidentRecalcState, name), name
    import inspect
    want = list(inspect.signature(pending.RecalcState.__init__).parameters) + ["hash_stride"]
    assert list(inspect.signature(pending.ResidentRecalcState.__init__).parameters) == want
    assert inspect.signature(pending.ResidentRecalcState.__init__).parameters["hash_stride"].default == 32
    assert list(inspect.signature(blockchain.state_recalc_resident).parameters) == \
        list(inspect.signature(blockchain.state_recalc_device).parameters)
    assert callable(blockchain.state_recalc_device) and hasattr(pending, "RecalcState")  # the model stays
