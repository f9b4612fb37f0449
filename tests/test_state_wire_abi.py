"""The ABI of the two states' encoders (include/prysm_hip.h, prysm_amd/csrc/wire_state.hip): the new
structs' ctypes mirrors against the header, and the new entry points exported and bound.  No GPU:
nothing is called except the host-only bound functions."""
import ctypes
import os
import re

import pytest

from prysm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pz_wire_committees_bound", "pz_wire_committees_scratch_bytes", "pz_dev_wire_committees", "pz_wire_committees",
       "pz_crystallized_state_bound", "pz_crystallized_state_scratch_bytes", "pz_dev_crystallized_state_bytes",
       "pz_crystallized_state_read", "pz_active_state_bound", "pz_dev_active_state_bytes", "pz_active_state_read")
C_TYPES = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "uint8_t": ctypes.c_uint8}


def header_fields(name):
    """``[(field, ctypes type)]`` of a struct of the header: pointers are void*, ``x[n]`` an array."""
    src = open(os.path.join(ROOT, "include", "prysm_hip.h")).read()
    body = src[src.index("typedef struct %s {" % name):src.index("} %s;" % name)].split("{", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        words = decl.replace("const", "").split()
        if not words:
            continue
        ctype, field = words[0], words[-1]
        if "*" in decl:
            out.append((field.lstrip("*"), ctypes.c_void_p))
        elif "[" in field:
            field, count = field.rstrip("]").split("[")
            out.append((field, C_TYPES[ctype] * int(count)))
        else:
            out.append((field, C_TYPES[ctype]))
    return out


@pytest.mark.parametrize("name,cls", [("pz_committee_table", _lib.CommitteeTable), ("pz_cstate_rest", _lib.CstateRest)])
def test_struct_layout(name, cls):
    want = header_fields(name)
    assert [f for f, _ in cls._fields_] == [f for f, _ in want]
    for (f, got), (_, exp) in zip(cls._fields_, want):
        assert ctypes.sizeof(got) == ctypes.sizeof(exp), f

    class Twin(ctypes.Structure):  # natural C alignment, as the compiler lays the header's struct out
        _fields_ = want
    assert ctypes.sizeof(cls) == ctypes.sizeof(Twin)
    assert [getattr(cls, f).offset for f, _ in want] == [getattr(Twin, f).offset for f, _ in want]


def test_cstate_rest_is_88_bytes_with_the_seed_at_8():
    assert ctypes.sizeof(_lib.CstateRest) == 88 and _lib.CstateRest.dynasty_seed.offset == 8
    assert _lib.CstateRest.dynasty_seed_len.offset == 72 and _lib.CstateRest.dynasty_seed_last_reset.offset == 80


def test_new_entry_points_are_exported_and_bound():
    dll = ctypes.CDLL(_lib.library_path)
    assert [n for n in NEW if not hasattr(dll, n)] == []
    assert [n for n in NEW if n not in _lib.SIGNATURES] == []
    for n in NEW:
        if n.endswith(("_bound", "_scratch_bytes")):
            assert _lib._RESTYPES.get(n) is _lib.u64, n


def test_bounds_hold_the_largest_encodings():
    dll = _lib.lib.dll
    # an array: a 5-byte key and a 10-byte length; an entry: 0a, length, 08 + shard, 12 + length; a member: 5
    assert dll.pz_wire_committees_bound(1, 0, 0) >= 15 and dll.pz_wire_committees_bound(0, 1, 0) >= 1 + 10 + 11 + 11
    assert dll.pz_wire_committees_bound(0, 0, 7) == 35
    assert dll.pz_wire_committees_scratch_bytes(3, 5, 1000) % 16 == 0
    head = dll.pz_crystallized_state_bound(0, 32, 0, 0, 0)
    assert head >= 8 * 11 + 2 + 64 and head % 16 == 0
    per_record = 1 + 1 + 11 + (2 + 32) + 11
    assert dll.pz_crystallized_state_bound(1024, 32, 0, 0, 0) >= head + 1024 * per_record
    assert dll.pz_crystallized_state_bound(0, 32, 10, 3, 7) == head + dll.pz_wire_validators_bound(10, 3) + 7
    counts = (ctypes.c_uint64 * 7)(3, 10, 20, 30, 2, 40, 5)
    assert dll.pz_active_state_bound(counts, 128) == dll.pz_wire_attestations_bound(3, 100, 2, 5) + 128 * 34
