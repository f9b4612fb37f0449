"""The block gate's C ABI (include/prysm_hip.h, prysm_amd/csrc/blockgate.hip): the header declares
its two entry points and cites the reference lines, the binding has them, the built library exports
them (and no pz_debug_* entry beside them), pz_block_gate_batch -- passed by pointer from ctypes,
with pz_att_check_batch embedded -- has the header's field order, offsets and size, and every
argument error is PZ_EINVAL before anything is launched or followed.  No GPU needed: the argument
checks come before the first HIP call, and only refused batches are sent."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from prysm_amd import _lib
from test_attdigest_abi import header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pz_dev_block_gate", "pz_block_gate")


def header():
    return open(os.path.join(ROOT, "include", "prysm_hip.h")).read()


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_points_resolve(name):
    src = header()
    assert re.search(r"\bint\s+%s\(" % name, src)
    assert name in _lib.SIGNATURES and _lib._RESTYPES.get(name, ctypes.c_int) is ctypes.c_int
    assert getattr(ctypes.CDLL(_lib.library_path), name) is not None
    m = re.search(r"\b%s\(([^;]*?)\);" % name, src, re.S)
    assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name])
    at = src.index(name + "(")
    assert re.search(r"\.go:\d+", src[src.rindex("/*", 0, at):at]), name


def test_product_library_exports_the_gate_and_no_debug_entry():
    out = subprocess.run(["nm", "-D", _lib.library_path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(ENTRIES) <= names
    assert not [n for n in names if n.startswith("pz_debug_") and "gate" in n]


def test_block_gate_batch_layout():
    fields = header_fields("pz_block_gate_batch")
    assert [f for _, f in fields] == [f for f, _ in _lib.BlockGateBatch._fields_]
    for (ctype, name), (_, t) in zip(fields, _lib.BlockGateBatch._fields_):
        if "*" in ctype:
            assert t is _lib.vp, name
        elif ctype == "uint64_t":
            assert t is _lib.u64, name
        else:  # the embedded batch: every member of it is a pointer or a uint64_t too, so no padding
            assert ctype == "pz_att_check_batch" and t is _lib.AttCheckBatch and name == "chk"
    chk = header_fields("pz_att_check_batch")
    assert [f for _, f in chk] == [f for f, _ in _lib.AttCheckBatch._fields_]
    assert ctypes.sizeof(_lib.AttCheckBatch) == 8 * len(chk) == 160
    assert len(fields) == 10 and ctypes.sizeof(_lib.BlockGateBatch) == 8 * 9 + 160 == 232
    offs = {f: getattr(_lib.BlockGateBatch, f).offset for f, _ in _lib.BlockGateBatch._fields_}
    assert (offs["nblocks"], offs["att_first"], offs["chk"], offs["report"], offs["flags"]) == (0, 8, 40, 200, 224)


def test_report_values_are_the_python_constants():
    from prysm_amd import blockchain as bc
    assert (bc.BLOCK_REJECTED, bc.BLOCK_TALLIED, bc.BLOCK_MIXED) == (0, 1, 2)
    src = open(os.path.join(ROOT, "prysm_amd", "csrc", "blockgate_dev.h")).read()
    assert re.search(r"kBgRejected = 0, kBgClean = 1, kBgMixed = 2", src)


def test_argument_errors_are_einval():
    """Each batch is refused before any launch: ``p`` points at host zeros in both forms and is
    never followed."""
    host = np.zeros(4096, np.uint8)
    p = host.ctypes.data
    dll = _lib.lib.dll
    forms = {"pz_dev_block_gate": lambda b: dll.pz_dev_block_gate(b, None), "pz_block_gate": lambda b: dll.pz_block_gate(b)}
    for form, call in forms.items():
        def run(chk=None, **kw):
            c = dict(natt=1, slot=p, shard_id=p, n_oblique=p, block_slot=p, n_recent=128, narr=1, arr_offs=p, arr_shard=p,
                     arr_comm=p, status=p, committee=p, parents_start=p)
            c.update(chk or {})
            f = dict(nblocks=1, att_first=p, block_status=p, report=p, vote_status=p, flags=p, chk=_lib.AttCheckBatch(**c))
            f.update(kw)
            return call(ctypes.byref(_lib.BlockGateBatch(**f)))

        assert call(None) == _lib.PZ_EINVAL, form
        for name in ("att_first", "block_status", "report", "vote_status", "flags"):
            assert run(**{name: None}) == _lib.PZ_EINVAL, (form, name)
        for name in ("committee", "parents_start"):  # optional for the checks, completed in place here
            assert run(chk={name: None}) == _lib.PZ_EINVAL, (form, name)
            assert run(chk={name: None, "natt": 0, "narr": 0}) == _lib.PZ_EINVAL, (form, name)
        for name in ("status", "slot", "block_slot", "n_oblique", "shard_id"):
            assert run(chk={name: None}) == _lib.PZ_EINVAL, (form, name)
        for name in ("arr_offs", "arr_shard", "arr_comm"):
            assert run(chk={name: None}) == _lib.PZ_EINVAL, (form, name)
        assert run(nblocks=1 << 31) == _lib.PZ_EINVAL and run(nblocks=(1 << 64) - 1) == _lib.PZ_EINVAL, form
        # an empty batch launches nothing, whatever else it holds
        assert call(ctypes.byref(_lib.BlockGateBatch())) == _lib.PZ_OK, form
        assert run(nblocks=0, att_first=None, flags=None) == _lib.PZ_OK, form
    assert not host.any()


def test_python_face_exists():
    from prysm_amd import blockchain
    assert list(inspect.signature(blockchain.gate_blocks).parameters) == ["d", "candidate"]
    sig = inspect.signature(blockchain.tally_serialized_blocks)
    assert sig.parameters["tally_mixed"].default is False and list(sig.parameters)[-1] == "tally_mixed"
