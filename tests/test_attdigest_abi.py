"""pz_att_msg_batch is passed by pointer from ctypes: field order and types must match
include/prysm_hip.h, and the four attestation-digest entry points must be in the built library.
No GPU needed."""
import ctypes
import os
import re

import pytest

from prysm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pz_dev_attestation_keys", "pz_attestation_keys", "pz_dev_attestation_messages",
           "pz_attestation_messages")


def header_fields(name):
    """[(type text, field name)] of a typedef'd struct of the header, comments removed."""
    src = open(os.path.join(ROOT, "include", "prysm_hip.h")).read()
    body = src[src.index("typedef struct %s" % name):src.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body.split("{", 1)[1], flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        base = " ".join(first.replace("*", " * ").split()[:-1])  # e.g. "const uint64_t *"
        stem = base.replace("*", "").strip()
        fields.append((base, first.replace("*", " ").split()[-1]))
        for r in rest:
            r = r.strip()
            fields.append((stem + (" *" if r.startswith("*") else ""), r.lstrip("*").strip()))
    return fields


def test_att_msg_batch_layout():
    fields = header_fields("pz_att_msg_batch")
    assert [f for _, f in fields] == [f for f, _ in _lib.AttMsgBatch._fields_]
    for (ctype, name), (_, t) in zip(fields, _lib.AttMsgBatch._fields_):
        if "*" in ctype:
            assert t is _lib.vp, name
        else:  # every member is a pointer or a uint64_t: no padding to get wrong
            assert ctype == "uint64_t" and t is _lib.u64, name
    assert ctypes.sizeof(_lib.AttMsgBatch) == 8 * len(fields)


def test_att_msg_batch_reuses_the_column_names():
    """Its columns carry the names they have in pz_attestation_cols and pz_att_check_batch, so
    a decoded batch and a check's results can be passed on by name."""
    names = [f for f, _ in _lib.AttMsgBatch._fields_]
    cols = {f for f, _ in _lib.AttestationCols._fields_}
    assert [n for n in names if n in cols] == ["slot", "shard_id", "shard_block_hash", "shard_block_hash_offs",
                                               "oblique_parent_hashes", "oblique_offs", "oblique_first"]
    check = {f for f, _ in _lib.AttCheckBatch._fields_}
    assert {"natt", "status", "parents_start", "n_recent"} <= check & set(names)


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_points_resolve(name):
    assert name in _lib.SIGNATURES
    dll = ctypes.CDLL(_lib.library_path)
    assert getattr(dll, name) is not None
    src = open(os.path.join(ROOT, "include", "prysm_hip.h")).read()
    assert re.search(r"\bint %s\(" % name, src)
