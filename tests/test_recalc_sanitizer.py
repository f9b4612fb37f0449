"""The resident transition's pure rules on the CPU under ASan+UBSan: votecache_dev.h's vc_probe and
prysm_amd/csrc/recalc_dev.h (the inlines pz_vc_lookup_kernel and the kernels of recalc.hip compile
too) driven by the stand-alone program prysm_amd/csrc/tests/recalc_san.cpp -- the probe against a
std::map over tables of 2-8 cells in which every hash has the same home cell (the wrap, a full table,
cells holding a claim or an id the cache never gave out), the justification loop against a
restatement of the Go loop that works from totals (single-failure, all-pass, all-fail, alternating
and random masks; streaks, lastStateRecalc values and deposits whose arithmetic wraps), and the
commit's panic decision and clamps.  Built by ``make -C prysm_amd/csrc san_recalc`` and run directly;
no GPU code is involved and nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_recalc_rules_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_recalc"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_recalc")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) probes, (\d+) masks, (\d+) commit decisions", r.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 3 * 4 * 4 * 68 and int(m.group(3)) > 1000, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
