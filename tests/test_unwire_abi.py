"""The decoder's two output structs (pz_attestation_cols_out, pz_block_cols_out) are passed by
pointer from ctypes: field order and packing must match include/prysm_hip.h.  No GPU needed."""
import os
import re

import pytest

from prysm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,cls", [("pz_attestation_cols_out", "AttestationColsOut"),
                                       ("pz_block_cols_out", "BlockColsOut")])
def test_struct_layout(name, cls):
    cls = getattr(_lib, cls)
    src = open(os.path.join(ROOT, "include", "prysm_hip.h")).read()
    body = src[src.index("typedef struct %s" % name):src.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body.split("{", 1)[1], flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            fields += [first.split()[-1].lstrip("*")] + [r.strip().lstrip("*") for r in rest]
    assert fields == [f for f, _ in cls._fields_]
    assert all(t is _lib.vp for _, t in cls._fields_)  # every member is a pointer: no padding to get wrong


def test_attestation_cols_out_extends_the_encoder_struct():
    """Same order and meaning as pz_attestation_cols, then the three decoder-only columns."""
    n = len(_lib.AttestationCols._fields_)
    assert _lib.AttestationColsOut._fields_[:n] == _lib.AttestationCols._fields_
    assert [f for f, _ in _lib.AttestationColsOut._fields_[n:]] == ["n_oblique", "last_byte", "status"]
