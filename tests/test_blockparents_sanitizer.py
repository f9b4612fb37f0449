"""The parent check's rules and the saved-block set's table on the CPU under ASan+UBSan:
prysm_amd/csrc/blockparents_dev.h (the inlines the kernels of blockparents.hip compile too) driven by
the stand-alone program prysm_amd/csrc/tests/blockparents_san.cpp through a sequential form of the
three launches of pz_dev_block_parents (open, link, the double-buffered pointer-jumping rounds), of the
insert (lanes of a tile in a shuffled order), the rehash and the lookup, against a block-by-block
restatement of blockchain/service.go:261-269 + :324 over a std::set that only grows -- nblocks in {0,
1, 2, 63, 64, 65, 1023, 1024, 1025, 2049}: linear chains (the deepest jump), a chain with a block
removed, a child before its parent, a block delivered twice with its child between and after, copies
whose caller masks differ in both orders, closed parents, slots 0 and 1, parent spans of 0, 31, 32 and
33 bytes, the zero hash as a key, 8-cell tables whose keys share a home cell, a full table, a reserve
from 8 to 4,096 cells, and 4,000 random runs, over arrays of exactly their sizes; the gate's report
over block_status_out is non-zero exactly where saved0 holds.  Built by ``make -C prysm_amd/csrc
san_blockparents`` and run directly; no GPU code is involved and nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_parents_rules_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_blockparents"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_blockparents")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) runs, (\d+) blocks, (\d+) saved, (\d+) refused, (\d+) closed, (\d+) linked, (\d+) in-set, (\d+) free, "
                 r"(\d+) copies, (\d+) inserted, (\d+) rehashes, (\d+) capacity, (\d+) wraps, (\d+) lookups, (\d+) rounds", r.stdout)
    assert m, r.stdout
    runs, blocks, saved, refused, closed, linked, in_set, free, copies, inserted, rehashes, capacity, wraps, lookups, rounds = \
        (int(x) for x in m.groups())
    assert runs > 4000 and blocks > 100000 and saved > 10000 and refused > 10000 and closed > 1000, r.stdout  # no class is empty
    assert linked > 10000 and in_set > 1000 and free > 1000 and copies >= 40 and inserted > 10000, r.stdout
    assert rehashes > 100 and capacity == 1 and wraps > 100 and lookups > 100000 and rounds == 12, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
