"""The device vote cache's C ABI (include/prysm_hip.h, prysm_amd/csrc/votecache.hip): the header
declares its entry points, the binding has them, the built library exports them, and
pz_vote_cols_batch -- passed by pointer from ctypes -- has the header's field order and types.
No GPU needed."""
import ctypes
import os
import re

import pytest

from prysm_amd import _lib
from test_attdigest_abi import header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"pz_vote_cache_new": "int", "pz_vote_cache_free": "void", "pz_vote_cache_scratch_bytes": "uint64_t",
           "pz_dev_vote_cache_tally": "int", "pz_vote_cache_tally": "int", "pz_vote_cache_read": "int",
           "pz_vote_cache_voters": "int"}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_points_resolve(name):
    src = open(os.path.join(ROOT, "include", "prysm_hip.h")).read()
    assert re.search(r"\b%s\s+%s\(" % (ENTRIES[name], name), src)
    assert name in _lib.SIGNATURES
    dll = ctypes.CDLL(_lib.library_path)
    assert getattr(dll, name) is not None
    want = {"int": ctypes.c_int, "void": None, "uint64_t": _lib.u64}[ENTRIES[name]]
    assert _lib._RESTYPES.get(name, ctypes.c_int) is want


def test_vote_cols_batch_layout():
    fields = header_fields("pz_vote_cols_batch")
    assert [f for _, f in fields] == [f for f, _ in _lib.VoteColsBatch._fields_]
    for (ctype, name), (_, t) in zip(fields, _lib.VoteColsBatch._fields_):
        if "*" in ctype:
            assert t is _lib.vp, name
        else:  # every member is a pointer or a uint64_t: no padding to get wrong
            assert ctype == "uint64_t" and t is _lib.u64, name
    assert len(fields) == 18
    assert ctypes.sizeof(_lib.VoteColsBatch) == 8 * len(fields)


def test_vote_cols_batch_reuses_the_column_names():
    """The columns carry the names they have in pz_attestation_cols, pz_att_check_batch and
    pz_att_msg_batch, so a decoded batch and a check's results can be passed on by name."""
    names = [f for f, _ in _lib.VoteColsBatch._fields_]
    assert {"oblique_parent_hashes", "oblique_offs", "oblique_first"} <= {f for f, _ in _lib.AttestationCols._fields_} & set(names)
    assert {"natt", "n_oblique", "bits", "boffs", "status", "committee", "parents_start"} <= \
        {f for f, _ in _lib.AttCheckBatch._fields_} & set(names)
    assert {"recent", "n_recent"} <= {f for f, _ in _lib.AttMsgBatch._fields_} & set(names)


def test_python_face_exists():
    from prysm_amd import blockchain, votes
    for name in ("tally_columns", "tally_host", "items", "voters", "total", "__contains__"):
        assert hasattr(votes.DeviceVoteCache, name), name
    assert callable(blockchain.tally_serialized_blocks)
