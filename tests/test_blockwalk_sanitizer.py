"""The block walk's rules on the CPU under ASan+UBSan: prysm_amd/csrc/blockwalk_dev.h (the inlines
the kernels of blockwalk.hip compile too) driven by the stand-alone program
prysm_amd/csrc/tests/blockwalk_san.cpp through a sequential form of the scan kernel (tiles of 1,024
lanes in waves of 64, with the carry) and of the rows, roll and append kernels, against a restatement
of blockchain/service.go:320-333 that walks block by block with a pending-candidate variable and a
list that only grows -- nblocks in {0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049}, all / none /
alternating blocks going on, siblings, decreasing slots, slots 0 and 1 with and without a carried
candidate, a carried candidate above every slot, a transition candidate first, in the middle, last
and just past a tile edge, lag 1 with its first candidate at 0, at 1024 and absent, and 3,000 random
runs, over arrays of exactly their sizes.  Built by ``make -C prysm_amd/csrc san_blockwalk`` and run
directly; no GPU code is involved and nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_walk_rules_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_blockwalk"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_blockwalk")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) runs, (\d+) blocks, (\d+) deferred, (\d+) saved-not-candidate, (\d+) candidates, (\d+) rows, "
                 r"(\d+) appends", r.stdout)
    assert m, r.stdout
    runs, blocks, deferred, saved, cands, rows, appends = (int(x) for x in m.groups())
    assert runs > 1000 and deferred > 1000 and saved > 1000, r.stdout  # no class is silently empty
    assert cands > 1000 and rows > 100000 and appends >= 15, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
