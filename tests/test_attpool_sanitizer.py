"""The pending-attestation pool's selection rules on the CPU under ASan+UBSan:
prysm_amd/csrc/attpool_dev.h (the inlines the kernels of attpool.hip compile too) driven by the
stand-alone program prysm_amd/csrc/tests/attpool_san.cpp -- a sequential form of the size, scan,
commit and write phases against a std::vector-of-records model, over random batches, appends at a
non-zero base, prunes, each of the seven capacities hit alone with the rollback, and the
inverted-range rule.  Built by ``make -C prysm_amd/csrc san_attpool`` and run directly; no GPU code
is involved and nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_selection_rules_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_attpool"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_attpool")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) calls landed, (\d+) rolled back, (\d+) prunes", r.stdout)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) >= 7 * 20 and int(m.group(3)) > 20, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
