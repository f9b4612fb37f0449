"""The vote cache's table rules on the CPU under ASan+UBSan: prysm_amd/csrc/votecache_dev.h (the
inlines the kernels of votecache.hip compile too) driven by the stand-alone program
prysm_amd/csrc/tests/votecache_san.cpp -- a sequential form of the mark, intern and commit phases
against a std::map model, over random batches, tables of 2-8 cells in which every hash has the same
home cell, and the rollback of a call that does not fit.  Built by ``make -C prysm_amd/csrc
san_votecache`` and run directly; no GPU code is involved and nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_logic_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_votecache"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_votecache")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) calls landed, (\d+) rolled back", r.stdout)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) > 0, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
