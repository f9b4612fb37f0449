"""The C ABI of the resident RecentBlockHashes and the block walk (include/prysm_hip.h,
prysm_amd/csrc/blockwalk.hip): the header declares the entry points and cites the reference lines, the
binding has them, the built library exports them (and no pz_debug_* entry beside them),
pz_block_walk_batch -- passed by pointer from ctypes -- has the header's field order and size, and
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
ENTRIES = ("pz_recent_hashes_new", "pz_recent_hashes_free", "pz_recent_hashes_view", "pz_recent_hashes_read",
           "pz_dev_recent_hashes_append", "pz_recent_hashes_append", "pz_block_walk_scratch_bytes", "pz_dev_block_walk",
           "pz_block_walk")
RESTYPES = {"pz_recent_hashes_free": None, "pz_block_walk_scratch_bytes": _lib.u64}


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
    if name != "pz_recent_hashes_free":  # every other declaration cites its reference lines (or says it has none)
        at = decl.start()
        assert re.search(r"\.go:\d+|no reference counterpart", src[src.rindex("/*", 0, at):at]), name


def test_product_library_exports_the_walk_and_no_debug_entry():
    out = subprocess.run(["nm", "-D", _lib.library_path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(ENTRIES) <= names
    assert not [n for n in names if n.startswith("pz_debug_") and "walk" in n]


def test_block_walk_batch_layout():
    fields = header_fields("pz_block_walk_batch")
    assert [f for _, f in fields] == [f for f, _ in _lib.BlockWalkBatch._fields_]
    for (ctype, name), (_, t) in zip(fields, _lib.BlockWalkBatch._fields_):
        assert t is (_lib.vp if "*" in ctype else _lib.u64), name
        assert "*" in ctype or ctype == "uint64_t", name
    assert len(fields) == 18 and ctypes.sizeof(_lib.BlockWalkBatch) == 8 * 18
    offs = {f: getattr(_lib.BlockWalkBatch, f).offset for f, _ in _lib.BlockWalkBatch._fields_}
    assert (offs["nblocks"], offs["has_candidate"], offs["lag"], offs["natt"], offs["walk"], offs["flags"]) == (0, 32, 56, 64, 104, 136)


def test_codes_are_the_python_constants():
    from prysm_amd import blockchain as bc
    assert (bc.WALK_OFF, bc.WALK_SAVED, bc.WALK_CANDIDATE, bc.WALK_DEFERRED) == (0, 1, 2, 3)
    src = open(os.path.join(ROOT, "prysm_amd", "csrc", "blockwalk_dev.h")).read()
    assert re.search(r"kBwOff = 0, kBwSaved = 1, kBwCandidate = 2, kBwDeferred = 3", src)
    assert re.search(r"enum \{ kBwStop = 0, kBwNcand, kBwHasCandidate, kBwCandidateSlot, kBwResultWords \}", src)


def test_scratch_bytes():
    dll = _lib.lib.dll
    assert dll.pz_block_walk_scratch_bytes(0, 0) == 129 * 32
    assert dll.pz_block_walk_scratch_bytes(1024, 5) == (129 + 1024) * 32


def test_argument_errors_are_einval():
    """Each call is refused before any launch or device call: ``p`` points at host zeros in both
    forms and is never followed; ``ring`` is not a handle and is never followed either."""
    host = np.zeros(4096, np.uint8)
    aligned = host.ctypes.data + (-host.ctypes.data) % 16
    dll = _lib.lib.dll
    ring = ctypes.c_void_p(aligned)  # never followed: every call below fails its checks first
    forms = {"pz_dev_block_walk": lambda r, b: dll.pz_dev_block_walk(r, b, None), "pz_block_walk": lambda r, b: dll.pz_block_walk(r, b)}
    for form, call in forms.items():
        def run(r=ring, **kw):
            f = dict(nblocks=1, slot_number=aligned, report=aligned, block_hash=aligned, natt=1, att_block=aligned,
                     vote_status=aligned, parents_start=aligned, walk=aligned, base=aligned, result=aligned, log=aligned)
            f.update(kw)
            return call(r, ctypes.byref(_lib.BlockWalkBatch(**f)))

        assert call(ring, None) == _lib.PZ_EINVAL and run(r=None) == _lib.PZ_EINVAL, form
        for name in ("slot_number", "report", "block_hash", "walk", "base", "result"):
            assert run(**{name: None}) == _lib.PZ_EINVAL, (form, name)
        for name in ("att_block", "vote_status", "parents_start"):
            assert run(**{name: None}) == _lib.PZ_EINVAL, (form, name)
        assert run(lag=2) == _lib.PZ_EINVAL and run(lag=(1 << 64) - 1) == _lib.PZ_EINVAL, form
        assert run(nblocks=1 << 31) == _lib.PZ_EINVAL and run(nblocks=(1 << 64) - 1) == _lib.PZ_EINVAL, form
        assert run(nblocks=0, lag=2) == _lib.PZ_EINVAL, form
    assert dll.pz_dev_block_walk(ring, ctypes.byref(_lib.BlockWalkBatch(nblocks=1, slot_number=aligned, report=aligned,
                                 block_hash=aligned, walk=aligned, base=aligned, result=aligned)), None) == _lib.PZ_EINVAL  # no log
    for name in ("block_hash", "log"):  # the device form wants both 16-byte aligned
        f = dict(nblocks=1, slot_number=aligned, report=aligned, block_hash=aligned, walk=aligned, base=aligned, result=aligned,
                 log=aligned)
        f[name] = aligned + 8
        assert dll.pz_dev_block_walk(ring, ctypes.byref(_lib.BlockWalkBatch(**f)), None) == _lib.PZ_EINVAL, name
    # an empty run launches nothing and touches no ring, whatever else the batch holds
    assert dll.pz_dev_block_walk(ring, ctypes.byref(_lib.BlockWalkBatch()), None) == _lib.PZ_OK
    res = np.full(4, 99, np.uint64)
    assert dll.pz_block_walk(ring, ctypes.byref(_lib.BlockWalkBatch(has_candidate=1, candidate_slot=7, result=res.ctypes.data))) == _lib.PZ_OK
    assert list(res) == [0, 0, 1, 7]

    # the ring
    out = ctypes.c_void_p(1)
    assert dll.pz_recent_hashes_new(aligned, aligned, 127, 0, ctypes.byref(out)) == _lib.PZ_EINVAL and out.value is None
    assert dll.pz_recent_hashes_new(aligned, aligned, 129, 0, ctypes.byref(out)) == _lib.PZ_EINVAL
    assert dll.pz_recent_hashes_new(aligned, aligned, 0, 0, ctypes.byref(out)) == _lib.PZ_EINVAL
    assert dll.pz_recent_hashes_new(None, None, 128, 0, ctypes.byref(out)) == _lib.PZ_EINVAL
    assert dll.pz_recent_hashes_new(aligned, aligned, 128, 0, None) == _lib.PZ_EINVAL
    assert dll.pz_recent_hashes_view(None, None, None) == _lib.PZ_EINVAL
    assert dll.pz_recent_hashes_read(None, None, None) == _lib.PZ_EINVAL
    for call in (lambda r, h, n: dll.pz_dev_recent_hashes_append(r, h, None, n, None),
                 lambda r, h, n: dll.pz_recent_hashes_append(r, h, None, n)):
        assert call(None, aligned, 1) == _lib.PZ_EINVAL and call(ring, None, 1) == _lib.PZ_EINVAL
        assert call(ring, aligned, 1 << 31) == _lib.PZ_EINVAL
        assert call(ring, None, 0) == _lib.PZ_OK  # nothing to append: nothing is launched
    assert dll.pz_dev_recent_hashes_append(ring, aligned + 8, None, 1, None) == _lib.PZ_EINVAL
    assert not host.any()
    dll.pz_recent_hashes_free(None)


def test_python_face_exists():
    from prysm_amd import blockchain, pending
    sig = inspect.signature(blockchain.walk_serialized_blocks)
    assert list(sig.parameters) == ["cache", "pool", "ring", "data", "offsets", "last_justified_slot", "last_state_recalc",
                                    "shard_and_committees", "balance", "eligible", "has_candidate", "candidate_slot", "lag",
                                    "want_digests", "device"]
    assert {"view", "read", "append"} <= set(dir(pending.DeviceRecentHashes))
    assert "DeviceRecentHashes" in pending.__all__
