"""The block gate's rule on the CPU under ASan+UBSan: prysm_amd/csrc/blockgate_dev.h (the inlines
pz_block_gate_kernel compiles too) driven by the stand-alone program
prysm_amd/csrc/tests/blockgate_san.cpp through a sequential form of the kernel's two passes, against
a restatement of blockchain/service.go:281-318 and core.go:300-374 that derives every row's parents
and committee on its own -- every check status in an open, a closed and an unaccepted block, the
wrap cases of start / end / idx, m in {0, 1, 63, 64, 65}, att_first pairs that are inverted or run
past the rows, blocks of 0..130 rows and random batches, over arrays of exactly their sizes.  Built
by ``make -C prysm_amd/csrc san_blockgate`` and run directly; no GPU code is involved and nothing is
loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_gate_rule_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_blockgate"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_blockgate")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) batches, (\d+) blocks, (\d+) rows, (\d+) re-derived, (\d+) panics", r.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(3)) > 100000, r.stdout
    assert int(m.group(4)) > 1000 and int(m.group(5)) > 1000, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
