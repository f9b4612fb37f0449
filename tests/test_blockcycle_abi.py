"""The C ABI of the run across a cycle transition (include/prysm_hip.h, prysm_amd/csrc/blockcycle.hip):
the header declares the entry points and cites the reference lines, the binding has them, the built
library exports them (and no pz_debug_* entry beside them), pz_block_cycle_batch -- passed by pointer
from ctypes -- has the header's field order and size, the result record's words are the header's, and
every argument error is PZ_EINVAL before anything is launched or followed.  No GPU needed: the
argument checks come before the first HIP call, and only refused calls are sent."""
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
ENTRIES = ("pz_block_cycle_scratch_bytes", "pz_dev_block_cycle", "pz_block_cycle")
RESTYPES = {"pz_block_cycle_scratch_bytes": _lib.u64}


def header():
    return open(os.path.join(ROOT, "include", "prysm_hip.h")).read()


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_points_resolve(name):
    src = header()
    decl = re.search(r"^(int|void|uint64_t)\s+%s\(" % name, src, re.M)
    assert decl
    assert name in _lib.SIGNATURES and _lib._RESTYPES.get(name, ctypes.c_int) is RESTYPES.get(name, ctypes.c_int)
    assert getattr(ctypes.CDLL(_lib.library_path), name) is not None
    m = re.compile(r"\b%s\(([^;]*?)\);" % name, re.S).search(src, decl.start())
    assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == len(_lib.SIGNATURES[name])
    at = decl.start()  # every declaration cites its reference lines (or says it has none)
    assert re.search(r"\.go:\d+|no reference counterpart", src[src.rindex("/*", 0, at):at]), name


def test_product_library_exports_the_cycle_and_no_debug_entry():
    out = subprocess.run(["nm", "-D", _lib.library_path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(ENTRIES) <= names
    assert not [n for n in names if n.startswith("pz_debug_") and "cycle" in n]


def test_block_cycle_batch_layout():
    fields = header_fields("pz_block_cycle_batch")
    assert [f for _, f in fields] == [f for f, _ in _lib.BlockCycleBatch._fields_]
    for (ctype, name), (_, t) in zip(fields, _lib.BlockCycleBatch._fields_):
        assert t is (_lib.vp if "*" in ctype else _lib.u64), name
        assert "*" in ctype or ctype == "uint64_t", name
    assert len(fields) == 22 and ctypes.sizeof(_lib.BlockCycleBatch) == 8 * 22
    offs = {f: getattr(_lib.BlockCycleBatch, f).offset for f, _ in _lib.BlockCycleBatch._fields_}
    assert (offs["nblocks"], offs["has_candidate"], offs["lag"], offs["natt"], offs["vote0"], offs["take1"], offs["walk"],
            offs["flags"]) == (0, 32, 56, 64, 104, 128, 136, 168)
    # the members the walk's batch has come in the walk's order, so a caller fills both alike
    walk = [f for f, _ in _lib.BlockWalkBatch._fields_]
    assert [f for f, _ in _lib.BlockCycleBatch._fields_ if f in walk] == walk


def test_the_record_and_the_codes_are_the_walks():
    """The first four result words and the four walk codes are blockwalk_dev.h's: no new code value,
    so pz_dev_block_set_insert_walked takes the codes unchanged."""
    src = open(os.path.join(ROOT, "prysm_amd", "csrc", "blockcycle_dev.h")).read()
    assert re.search(r"enum \{ kBcTIndex = kBwResultWords, kBcTRank, kBcTSlot, kBcLagOut, kBcResultWords \}", src)
    assert '#include "blockwalk_dev.h"' in src and not re.search(r"kBw(Off|Saved|Candidate|Deferred)\s*=", src)
    assert "hip_runtime" not in src  # no HIP types: the CPU check compiles it with plain g++
    from prysm_amd import blockchain as bc
    assert bc._NO_T == (1 << 64) - 1


def test_scratch_bytes():
    dll = _lib.lib.dll
    assert dll.pz_block_cycle_scratch_bytes(0, 0) == 129 * 32
    assert dll.pz_block_cycle_scratch_bytes(1024, 5) == (129 + 1024) * 32


def test_argument_errors_are_einval():
    """Each call is refused before any launch or device call: ``p`` points at host zeros in both
    forms and is never followed; ``ring`` is not a handle and is never followed either."""
    host = np.zeros(4096, np.uint8)
    aligned = host.ctypes.data + (-host.ctypes.data) % 16
    dll = _lib.lib.dll
    ring = ctypes.c_void_p(aligned)  # never followed: every call below fails its checks first
    forms = {"pz_dev_block_cycle": lambda r, b: dll.pz_dev_block_cycle(r, b, None), "pz_block_cycle": lambda r, b: dll.pz_block_cycle(r, b)}
    rows = ("att_block", "vote_status", "parents_start", "vote0", "vote1", "take0", "take1")
    for form, call in forms.items():
        def run(r=ring, **kw):
            f = dict(nblocks=1, slot_number=aligned, report=aligned, block_hash=aligned, natt=1, walk=aligned, base=aligned,
                     result=aligned, log=aligned, **{k: aligned for k in rows})
            f.update(kw)
            return call(r, ctypes.byref(_lib.BlockCycleBatch(**f)))

        assert call(ring, None) == _lib.PZ_EINVAL and run(r=None) == _lib.PZ_EINVAL, form
        for name in ("slot_number", "report", "block_hash", "walk", "base", "result") + rows:
            assert run(**{name: None}) == _lib.PZ_EINVAL, (form, name)
        assert run(lag=2) == _lib.PZ_EINVAL and run(lag=(1 << 64) - 1) == _lib.PZ_EINVAL, form
        assert run(nblocks=1 << 31) == _lib.PZ_EINVAL and run(nblocks=(1 << 64) - 1) == _lib.PZ_EINVAL, form
        assert run(nblocks=0, lag=2) == _lib.PZ_EINVAL, form
    blocks = dict(nblocks=1, slot_number=aligned, report=aligned, block_hash=aligned, walk=aligned, base=aligned, result=aligned)
    assert dll.pz_dev_block_cycle(ring, ctypes.byref(_lib.BlockCycleBatch(**blocks)), None) == _lib.PZ_EINVAL  # no log
    for name in ("block_hash", "log"):  # the device form wants both 16-byte aligned
        f = dict(blocks, log=aligned)
        f[name] = aligned + 8
        assert dll.pz_dev_block_cycle(ring, ctypes.byref(_lib.BlockCycleBatch(**f)), None) == _lib.PZ_EINVAL, name
    # an empty run launches nothing and touches no ring, whatever else the batch holds
    assert dll.pz_dev_block_cycle(ring, ctypes.byref(_lib.BlockCycleBatch()), None) == _lib.PZ_OK
    for lag in (0, 1):
        res = np.full(8, 99, np.uint64)
        b = _lib.BlockCycleBatch(has_candidate=1, candidate_slot=7, lag=lag, result=res.ctypes.data)
        assert dll.pz_block_cycle(ring, ctypes.byref(b)) == _lib.PZ_OK
        assert list(res) == [0, 0, 1, 7, (1 << 64) - 1, 0, 0, lag]
    assert not host.any()


def check_resident_chain_init(RC):
    """ResidentChain's constructor as callers know it: the seven positional arguments in their order,
    ``device`` defaulting to 0, then exactly the two policies, keyword-only and "fixed" by default,
    on a plain class."""
    params = list(inspect.signature(RC.__init__).parameters.values())
    assert [p.name for p in params[:8]] == ["self", "cache", "pool", "ring", "saved", "state", "shard_and_committees", "device"]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params[:8])
    assert [p.default for p in params[:8]] == [inspect.Parameter.empty] * 7 + [0]
    assert [(p.name, p.kind, p.default) for p in params[8:]] == [("cache_policy", inspect.Parameter.KEYWORD_ONLY, "fixed"),
                                                                 ("pool_policy", inspect.Parameter.KEYWORD_ONLY, "fixed")]
    assert type(RC) is type


def test_python_face_exists():
    from prysm_amd import blockchain
    sig = inspect.signature(blockchain.ResidentChain.process_serialized)
    assert list(sig.parameters) == ["self", "data", "offsets", "eligible", "want_digests"]
    assert list(inspect.signature(blockchain.ResidentChain.process_all).parameters) == ["self", "data", "offsets", "eligible",
                                                                                        "want_digests"]
    check_resident_chain_init(blockchain.ResidentChain)
    # the walk's entry points keep their pinned parameter lists
    assert list(inspect.signature(blockchain.walk_serialized_blocks).parameters)[:4] == ["cache", "pool", "ring", "data"]
