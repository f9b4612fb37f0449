"""The C ABI of the attestation store batch (include/prysm_hip.h, prysm_amd/csrc/blockstore.hip): the
header declares the entry points and cites the reference lines, the binding has them, the built
library exports them (and no pz_debug_* entry beside them), pz_block_store_batch -- passed by pointer
from ctypes -- has the header's field order and size, every argument error is PZ_EINVAL before
anything is launched or followed, the zero-size calls launch nothing, and ResidentChain's switch is
a plain attribute that is off by default.  No GPU needed: the argument checks come before the first
HIP call, and only refused or empty calls are sent."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from prysm_amd import _lib
from test_attdigest_abi import header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pz_block_store_scratch_bytes", "pz_dev_block_store_select", "pz_dev_block_store_digests", "pz_block_store_select",
           "pz_block_store_digests")
RESTYPES = {"pz_block_store_scratch_bytes": _lib.u64}
SELECT_PTRS = ("att_first", "block_status", "parent_ok", "att_block", "att_status", "att_beg", "att_end", "rows", "span", "first", "count")
DIGEST_PTRS = ("bytes", "rows", "span", "key", "hash", "lists")


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


def test_product_library_exports_the_store_and_no_debug_entry():
    out = subprocess.run(["nm", "-D", _lib.library_path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(ENTRIES) <= names
    assert not [n for n in names if n.startswith("pz_debug_") and "store" in n]


def test_block_store_batch_layout():
    fields = header_fields("pz_block_store_batch")
    assert [f for _, f in fields] == [f for f, _ in _lib.BlockStoreBatch._fields_]
    for (ctype, name), (_, t) in zip(fields, _lib.BlockStoreBatch._fields_):
        assert t is (_lib.vp if "*" in ctype else _lib.u64), name
        assert "*" in ctype or ctype == "uint64_t", name  # every member a pointer or a uint64_t
    assert len(fields) == 20 and ctypes.sizeof(_lib.BlockStoreBatch) == 8 * 20
    offs = {f: getattr(_lib.BlockStoreBatch, f).offset for f, _ in _lib.BlockStoreBatch._fields_}
    assert (offs["nblocks"], offs["stop"], offs["natt"], offs["rows"], offs["count"], offs["bytes"], offs["nbytes"], offs["lists"]) == \
        (0, 32, 40, 88, 112, 120, 128, 152)


def test_scratch_bytes():
    dll = _lib.lib.dll
    tiles = lambda n: (n + 255) // 256  # noqa: E731
    pad = lambda x: (x + 255) & ~255  # noqa: E731
    for nb, n in ((0, 0), (3, 1), (10, 256), (10, 257), (1024, 65536)):
        assert dll.pz_block_store_scratch_bytes(nb, n) == pad(8 * (tiles(n) + 1) + 4 * (n + 1)), (nb, n)


def test_select_argument_errors_are_einval():
    """Each call is refused before any launch or device call: every pointer is an address inside host
    zeros in both forms and is never followed."""
    host = np.zeros(4096, np.uint8)
    aligned = host.ctypes.data + (-host.ctypes.data) % 16
    dll = _lib.lib.dll
    forms = {"dev": lambda b: dll.pz_dev_block_store_select(b, aligned, None), "host": lambda b: dll.pz_block_store_select(b)}
    for form, call in forms.items():
        def run(**kw):
            f = dict(nblocks=1, natt=1, stop=aligned, rec_status=aligned, **{k: aligned for k in SELECT_PTRS})
            f.update(kw)
            return call(ctypes.byref(_lib.BlockStoreBatch(**f)))

        assert call(None) == _lib.PZ_EINVAL, form
        for name in SELECT_PTRS:
            assert run(**{name: None}) == _lib.PZ_EINVAL, (form, name)
        assert run(nblocks=1 << 31) == _lib.PZ_EINVAL and run(nblocks=(1 << 64) - 1) == _lib.PZ_EINVAL, form
        assert run(natt=1 << 32) == _lib.PZ_EINVAL and run(natt=(1 << 64) - 1) == _lib.PZ_EINVAL, form
        assert run(nblocks=0, natt=1 << 32) == _lib.PZ_EINVAL, form  # the sizes are checked before the empty call returns
    # the device form: scratch, then every pointer aligned to its element (span: 16 bytes)
    ok = dict(nblocks=1, natt=1, stop=aligned, rec_status=aligned, **{k: aligned for k in SELECT_PTRS})
    b = _lib.BlockStoreBatch(**ok)
    assert dll.pz_dev_block_store_select(ctypes.byref(b), None, None) == _lib.PZ_EINVAL
    assert dll.pz_dev_block_store_select(ctypes.byref(b), aligned + 8, None) == _lib.PZ_EINVAL
    for name, off in [("span", 8), ("att_first", 4), ("att_beg", 4), ("att_end", 4), ("stop", 4), ("first", 4), ("count", 4),
                      ("block_status", 2), ("att_block", 2), ("att_status", 2), ("rec_status", 2), ("rows", 2)]:
        f = dict(ok)
        f[name] = aligned + off
        assert dll.pz_dev_block_store_select(ctypes.byref(_lib.BlockStoreBatch(**f)), aligned, None) == _lib.PZ_EINVAL, name
    assert not host.any()


def test_digests_argument_errors_are_einval():
    host = np.zeros(4096, np.uint8)
    aligned = host.ctypes.data + (-host.ctypes.data) % 16
    dll = _lib.lib.dll
    cols = _lib.AttestationCols(slot=aligned, shard_id=aligned)
    forms = {"dev": lambda b, a, m: dll.pz_dev_block_store_digests(b, a, m, None), "host": lambda b, a, m: dll.pz_block_store_digests(b, a, m)}
    for form, call in forms.items():
        def run(a=cols, m=1, **kw):
            f = dict(natt=2, nbytes=64, **{k: aligned for k in DIGEST_PTRS})
            f.update(kw)
            return call(ctypes.byref(_lib.BlockStoreBatch(**f)), None if a is None else ctypes.byref(a), m)

        assert call(None, ctypes.byref(cols), 1) == _lib.PZ_EINVAL and run(a=None) == _lib.PZ_EINVAL, form
        for name in DIGEST_PTRS:
            assert run(**{name: None}) == _lib.PZ_EINVAL, (form, name)
        assert run(m=3) == _lib.PZ_EINVAL and run(m=(1 << 64) - 1) == _lib.PZ_EINVAL, form  # more rows than there are
        assert run(natt=1 << 32, m=1) == _lib.PZ_EINVAL, form
        for bad in (_lib.AttestationCols(shard_block_hash_offs=aligned), _lib.AttestationCols(oblique_first=aligned),
                    _lib.AttestationCols(oblique_first=aligned, oblique_offs=aligned)):  # offsets without their data column
            assert run(a=bad) == _lib.PZ_EINVAL, form
    for name, off in [("span", 8), ("key", 8), ("hash", 8), ("rows", 2), ("lists", 2)]:
        f = dict(natt=2, nbytes=64, **{k: aligned for k in DIGEST_PTRS})
        f[name] = aligned + off
        assert dll.pz_dev_block_store_digests(ctypes.byref(_lib.BlockStoreBatch(**f)), ctypes.byref(cols), 1, None) == _lib.PZ_EINVAL, name
    # the host form reads what the device form takes on trust: a row past natt, a span that leaves the bytes
    rows, span = np.array([2], np.uint32), np.array([0, 8], np.uint64)
    f = dict(natt=2, nbytes=64, **{k: aligned for k in DIGEST_PTRS})
    f.update(rows=rows.ctypes.data, span=span.ctypes.data)
    assert dll.pz_block_store_digests(ctypes.byref(_lib.BlockStoreBatch(**f)), ctypes.byref(cols), 1) == _lib.PZ_EINVAL
    rows[0] = 1
    for lo, hi in ((9, 8), (0, 65)):
        span[:] = (lo, hi)
        assert dll.pz_block_store_digests(ctypes.byref(_lib.BlockStoreBatch(**f)), ctypes.byref(cols), 1) == _lib.PZ_EINVAL, (lo, hi)
    assert not host.any()


def test_zero_size_calls_launch_nothing():
    """nblocks == 0, natt == 0 and m == 0 return PZ_OK without following a pointer: the addresses are
    not device memory, and the host form's only writes are the zero count and ranks."""
    host = np.zeros(256, np.uint8)
    aligned = host.ctypes.data + (-host.ctypes.data) % 16
    dll = _lib.lib.dll
    every = {k: aligned for k in SELECT_PTRS + DIGEST_PTRS}
    for sizes in (dict(nblocks=0, natt=0), dict(nblocks=0, natt=5), dict(nblocks=5, natt=0)):
        b = _lib.BlockStoreBatch(**sizes, **every)
        assert dll.pz_dev_block_store_select(ctypes.byref(b), aligned, None) == _lib.PZ_OK, sizes
        assert dll.pz_dev_block_store_select(ctypes.byref(_lib.BlockStoreBatch(**sizes)), None, None) == _lib.PZ_OK, sizes
        first, count = np.full(sizes["nblocks"] + 1 + 2, 77, np.uint64), np.full(1, 77, np.uint64)
        b = _lib.BlockStoreBatch(**sizes, first=first.ctypes.data, count=count.ctypes.data)
        assert dll.pz_block_store_select(ctypes.byref(b)) == _lib.PZ_OK, sizes
        assert list(first) == [0] * (sizes["nblocks"] + 1) + [77, 77] and count[0] == 0, sizes
    cols = _lib.AttestationCols()
    for b in (_lib.BlockStoreBatch(natt=4, **every), _lib.BlockStoreBatch(natt=4), _lib.BlockStoreBatch()):
        assert dll.pz_dev_block_store_digests(ctypes.byref(b), ctypes.byref(cols), 0, None) == _lib.PZ_OK
        assert dll.pz_block_store_digests(ctypes.byref(b), None, 0) == _lib.PZ_OK
    assert not host.any()


def test_the_store_switch_is_a_plain_attribute_off_by_default():
    from prysm_amd import blockchain
    from test_blockcycle_abi import check_resident_chain_init, test_python_face_exists

    RC = blockchain.ResidentChain
    assert RC.store is False and "store" in vars(RC) and not isinstance(vars(RC)["store"], property)
    rc = RC.__new__(RC)
    assert rc.store is False
    rc.store = True  # set per object: the class keeps its default
    assert rc.store is True and RC.store is False
    check_resident_chain_init(RC)  # the pinned parameter lists stay as they are
    test_python_face_exists()
    assert callable(blockchain.store_writes)
