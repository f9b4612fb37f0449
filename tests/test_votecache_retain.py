"""The vote cache's growth and retirement without a GPU:

1. the rules of prysm_amd/csrc/votecache_dev.h (keep, renumber, the move's row split, the rehash insert
   -- the inlines the kernels of votecache.hip compile too) on the CPU under ASan+UBSan, driven lane by
   lane by the stand-alone program prysm_amd/csrc/tests/votecache_retain_san.cpp against a std::map
   filtered by the keep list.  Built by ``make -C prysm_amd/csrc san_votecache_retain`` and run
   directly; no GPU code is involved and nothing is loaded into Python;
2. the C ABI: the header declares the entry points, the binding has them, the library exports them,
   and a NULL cache is refused before any device call;
3. the Python face."""
import ctypes
import os
import re
import subprocess

import pytest

from prysm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"pz_vote_cache_capacity": "int", "pz_dev_vote_cache_reserve": "int", "pz_vote_cache_reserve": "int",
           "pz_vote_cache_retain_scratch_bytes": "uint64_t", "pz_dev_vote_cache_retain": "int", "pz_vote_cache_retain": "int"}


def test_rules_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_votecache_retain"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_votecache_retain")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) caches retained twice and reserved", r.stdout)
    assert m and int(m.group(1)) > 500, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_points_resolve(name):
    src = open(os.path.join(ROOT, "include", "prysm_hip.h")).read()
    assert re.search(r"\b%s\s+%s\(" % (ENTRIES[name], name), src)
    assert name in _lib.SIGNATURES
    dll = ctypes.CDLL(_lib.library_path)
    assert getattr(dll, name) is not None
    want = {"int": ctypes.c_int, "uint64_t": _lib.u64}[ENTRIES[name]]
    assert _lib._RESTYPES.get(name, ctypes.c_int) is want


def test_every_entry_cites_the_reference_or_says_it_has_no_counterpart():
    src = open(os.path.join(ROOT, "include", "prysm_hip.h")).read()
    for name in ENTRIES:
        at = src.index(name + "(")
        comment = src[src.rindex("/*", 0, at):at]
        assert re.search(r"no reference counterpart|\w+\.go:\d+", comment), name


def test_a_null_cache_is_refused_before_any_device_call():
    dll = _lib.lib.dll
    cap = ctypes.c_uint32(7)
    E = _lib.PZ_EINVAL
    assert dll.pz_vote_cache_capacity(None, ctypes.byref(cap)) == E and cap.value == 7
    assert dll.pz_dev_vote_cache_reserve(None, 1, None) == E and dll.pz_vote_cache_reserve(None, 1) == E
    assert dll.pz_dev_vote_cache_retain(None, None, 0, None, None) == E and dll.pz_vote_cache_retain(None, None, 0) == E


def test_scratch_bytes():
    f = _lib.lib.dll.pz_vote_cache_retain_scratch_bytes
    for cap in (1, 4, 5, 512, 2500):
        assert f(cap, 0) == f(cap, 1000) >= 3 * 4 * cap and f(cap, 0) % 16 == 0


def test_python_face_exists():
    from prysm_amd import blockchain, votes
    assert callable(votes.DeviceVoteCache.reserve) and callable(votes.DeviceVoteCache.retain)
    assert blockchain.ResidentChain.CACHE_POLICIES == ("fixed", "grow", "retire")
