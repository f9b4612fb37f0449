"""The rules of a run across a cycle transition on the CPU under ASan+UBSan:
prysm_amd/csrc/blockcycle_dev.h (the inlines the kernels of blockcycle.hip compile too) driven by the
stand-alone program prysm_amd/csrc/tests/blockcycle_san.cpp through a sequential form of the scan
kernel (tiles of 1,024 lanes in waves of 64, the carry, the ballot words) and of the rows and roll
kernels, against a restatement of blockchain/service.go:320-363 that walks block by block with a
pending-candidate variable, a "the candidate's states are not promoted yet" flag, a
last_state_recalc that advances at the transition block and a list that only grows -- nblocks in
{0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049}; no transition block; one first, in the middle, last and
at lanes 1,022, 1,023 and 1,024 with the promoting block in the next tile; siblings and closed blocks
between the two; the promoting block a transition itself (deferred); the run ending before it; lag 1
with its first candidate plain and a transition; slots 0 and 1; last_state_recalc near 2^64; and
4,000 random runs, over arrays of exactly their sizes.  On every run without a transition block
(among them runs of {1, 64, 65, 1023, 1024, 1025, 2049} blocks with lag 0 and 1 against a
last_state_recalc no slot reaches) the cycle's form is also held against the walk's.  Built by ``make -C prysm_amd/csrc
san_blockcycle`` and run directly; no GPU code is involved and nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_cycle_rules_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_blockcycle"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_blockcycle")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) runs, (\d+) blocks, (\d+) deferred, (\d+) saved-not-candidate, (\d+) candidates, (\d+) rows, "
                 r"(\d+) with T, (\d+) with L deferred, (\d+) with T under lag, (\d+) rows after T", r.stdout)
    assert m, r.stdout
    runs, blocks, deferred, saved, cands, rows, with_t, l_deferred, lag_t, after = (int(x) for x in m.groups())
    assert runs > 1000 and deferred > 1000 and saved > 1000 and cands > 1000 and rows > 100000, r.stdout
    assert with_t > 1000 and l_deferred > 100 and lag_t > 100 and after > 10000, r.stdout  # no class is silently empty
    # the runs without a transition block, on which the cycle's form must equal the walk's
    w = re.search(r"^the walk's runs: (\d+), (\d+) under lag, (\d+) stopped early$", r.stdout, re.M)
    assert w, r.stdout
    walks, walks_lag, walks_early = (int(x) for x in w.groups())
    assert walks > 1000 and walks_lag > 100 and walks_early > 100, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
