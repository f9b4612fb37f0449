"""The C ABI of the resident saved-block set and the parent check (include/prysm_hip.h,
prysm_amd/csrc/blockparents.hip): the header declares the entry points and cites the reference lines,
the binding has them, the built library exports them (and no pz_debug_* entry beside them),
pz_block_parents_batch -- passed by pointer from ctypes -- has the header's field order and size, and
every argument error is PZ_EINVAL before anything is launched or followed.  No GPU needed: the
argument checks come before the first HIP call, and only refused or empty calls are sent."""
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
ENTRIES = ("pz_block_set_new", "pz_block_set_free", "pz_block_set_count", "pz_block_set_read", "pz_dev_block_set_contains",
           "pz_block_set_contains", "pz_dev_block_set_insert", "pz_block_set_insert", "pz_dev_block_set_reserve",
           "pz_block_set_reserve", "pz_block_parents_scratch_bytes", "pz_dev_block_parents", "pz_block_parents",
           "pz_dev_block_set_insert_walked")
RESTYPES = {"pz_block_set_free": None, "pz_block_parents_scratch_bytes": _lib.u64}


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
    if name != "pz_block_set_free":  # every other declaration cites its reference lines (or says it has none)
        at = decl.start()
        assert re.search(r"\.go:\d+|no reference counterpart", src[src.rindex("/*", 0, at):at]), name


def test_product_library_exports_the_entries_and_no_debug_entry():
    out = subprocess.run(["nm", "-D", _lib.library_path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(ENTRIES) <= names
    assert not [n for n in names if n.startswith("pz_debug_") and ("parents" in n or "block_set" in n)]


def test_block_parents_batch_layout():
    fields = header_fields("pz_block_parents_batch")
    assert [f for _, f in fields] == [f for f, _ in _lib.BlockParentsBatch._fields_]
    for (ctype, name), (_, t) in zip(fields, _lib.BlockParentsBatch._fields_):
        assert t is (_lib.vp if "*" in ctype else _lib.u64), name
        assert "*" in ctype or ctype == "uint64_t", name
    assert len(fields) == 15 and ctypes.sizeof(_lib.BlockParentsBatch) == 8 * 15
    offs = {f: getattr(_lib.BlockParentsBatch, f).offset for f, _ in _lib.BlockParentsBatch._fields_}
    assert (offs["nblocks"], offs["nbytes"], offs["block_hash"], offs["natt"], offs["block_status_out"]) == (0, 16, 48, 88, 112)


def test_rule_constants():
    src = open(os.path.join(ROOT, "prysm_amd", "csrc", "blockparents_dev.h")).read()
    assert re.search(r"kBpTrue = 0xFFFFFFFFu, kBpFalse = 0xFFFFFFFEu", src)
    assert re.search(r"kBsEmpty = 0xFFFFFFFFu, kBsFull = 0;", src) and re.search(r"kBsMinCells = 8", src)
    assert "bg_span_ok" in src and "bg_report" in src and "vc_bytes_to_hash" in src  # the gate's and the cache's own inlines
    assert _lib.PZ_ENOTFOUND == -5  # block_status_out where the parent is not saved


def test_scratch_bytes():
    dll = _lib.lib.dll
    r16 = lambda x: (x + 15) & ~15  # noqa: E731
    for n, cells in ((0, 2), (1, 2), (2, 4), (63, 128), (1024, 2048), (1025, 4096)):
        assert dll.pz_block_parents_scratch_bytes(n) == r16(4 * cells) + 3 * r16(4 * n) + r16(n), n


def test_argument_errors_are_einval():
    """Each call is refused before any launch or device call: ``p`` points at host zeros in both
    forms and is never followed; ``hset`` is not a handle and is never followed either."""
    host = np.zeros(4096, np.uint8)
    aligned = host.ctypes.data + (-host.ctypes.data) % 16
    dll = _lib.lib.dll
    E = _lib.PZ_EINVAL
    hset = ctypes.c_void_p(aligned)
    forms = {"pz_dev_block_parents": lambda s, b: dll.pz_dev_block_parents(s, b, aligned, None),
             "pz_block_parents": lambda s, b: dll.pz_block_parents(s, b)}
    pointers = ("bytes_beg", "bytes_len", "slot_number", "block_hash", "att_first", "block_status", "parent_ok", "saved0",
                "block_status_out")
    for form, call in forms.items():
        def run(s=hset, **kw):
            f = dict(nblocks=1, bytes=aligned, nbytes=8, natt=1, att_status=aligned, rec_status=aligned,
                     **{k: aligned for k in pointers})
            f.update(kw)
            return call(s, ctypes.byref(_lib.BlockParentsBatch(**f)))

        assert call(hset, None) == E and run(s=None) == E, form
        for name in pointers:
            assert run(**{name: None}) == E, (form, name)
        assert run(bytes=None) == E and run(att_status=None) == E, form
        assert run(nblocks=1 << 31) == E and run(nblocks=(1 << 64) - 1) == E, form
        # an empty run launches nothing and follows nothing, whatever else the batch holds
        assert call(hset, ctypes.byref(_lib.BlockParentsBatch())) == _lib.PZ_OK, form
    ok = dict(nblocks=1, bytes=aligned, nbytes=8, natt=0, **{k: aligned for k in pointers})
    assert dll.pz_dev_block_parents(hset, ctypes.byref(_lib.BlockParentsBatch(**ok)), None, None) == E  # no scratch
    assert dll.pz_dev_block_parents(hset, ctypes.byref(_lib.BlockParentsBatch(**ok)), aligned + 8, None) == E
    ok["block_hash"] = aligned + 8  # the device form wants it 16-byte aligned
    assert dll.pz_dev_block_parents(hset, ctypes.byref(_lib.BlockParentsBatch(**ok)), aligned, None) == E

    # the set
    out = ctypes.c_void_p(1)
    assert dll.pz_block_set_new(None, 1, 0, 0, ctypes.byref(out)) == E and out.value is None
    assert dll.pz_block_set_new(aligned, 0, 0, 0, None) == E
    assert dll.pz_block_set_new(aligned, (1 << 30) + 1, 0, 0, ctypes.byref(out)) == E
    assert dll.pz_block_set_new(None, 0, (1 << 30) + 1, 0, ctypes.byref(out)) == E
    n64 = ctypes.c_uint64(7)
    assert dll.pz_block_set_count(None, ctypes.byref(n64)) == E and dll.pz_block_set_count(hset, None) == E
    assert dll.pz_block_set_read(None, aligned, 1, ctypes.byref(n64)) == E and dll.pz_block_set_read(hset, aligned, 1, None) == E
    for call in (lambda s, h, n: dll.pz_dev_block_set_contains(s, h, n, aligned, None),
                 lambda s, h, n: dll.pz_block_set_contains(s, h, n, aligned),
                 lambda s, h, n: dll.pz_dev_block_set_insert(s, h, None, n, None),
                 lambda s, h, n: dll.pz_block_set_insert(s, h, None, n),
                 lambda s, h, n: dll.pz_dev_block_set_insert_walked(s, h, aligned, None, n, None, None)):
        assert call(None, aligned, 1) == E and call(hset, None, 1) == E
        assert call(hset, aligned, 1 << 31) == E and call(hset, aligned, (1 << 64) - 1) == E
        assert call(hset, None, 0) == _lib.PZ_OK  # nothing to do: nothing is launched
    assert dll.pz_dev_block_set_contains(hset, aligned, 1, None, None) == E
    assert dll.pz_block_set_contains(hset, aligned, 1, None) == E
    assert dll.pz_dev_block_set_contains(hset, aligned + 8, 1, aligned, None) == E
    assert dll.pz_dev_block_set_insert(hset, aligned + 8, None, 1, None) == E
    assert dll.pz_dev_block_set_insert_walked(hset, aligned + 8, aligned, None, 1, None, None) == E
    assert dll.pz_dev_block_set_insert_walked(hset, aligned, None, None, 1, None, None) == E  # no walk
    assert dll.pz_dev_block_set_reserve(None, 1, None) == E and dll.pz_block_set_reserve(None, 1) == E
    assert dll.pz_dev_block_set_reserve(hset, (1 << 30) + 1, None) == E and dll.pz_block_set_reserve(hset, (1 << 30) + 1) == E
    assert not host.any() and n64.value == 7
    dll.pz_block_set_free(None)


def test_python_face_exists():
    from prysm_amd import blockchain, pending
    sig = inspect.signature(blockchain.walk_serialized_blocks_saved)
    assert list(sig.parameters) == ["cache", "pool", "ring", "saved", "data", "offsets", "last_justified_slot",
                                    "last_state_recalc", "shard_and_committees", "balance", "eligible", "has_candidate",
                                    "candidate_slot", "lag", "want_digests", "device"]
    assert {"contains", "insert", "count", "hashes", "reserve"} <= set(dir(pending.DeviceSavedBlocks))
    assert "DeviceSavedBlocks" in pending.__all__
    assert list(inspect.signature(pending.DeviceSavedBlocks.__init__).parameters) == ["self", "hashes", "min_keys", "device"]
