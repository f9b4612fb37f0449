"""The attestation column table and the one staging rule on the CPU under ASan+UBSan:
prysm_amd/csrc/att_cols.h (the text the host-pointer entry points compile) driven by the stand-alone
program prysm_amd/csrc/tests/att_cols_san.cpp through a memcpy uploader -- for every row the bytes
seen through the staged (data, offsets) are the bytes seen through the caller's: monotone offsets
from 0 and from a non-zero base, an inverted range among valid ones, empty columns, every NULL
combination the entry points allow, n = 0, the two-level oblique column with zero, one and several
elements, and random column sets; and the table's widths, lengths and order against the two
structs.  Built by ``make -C prysm_amd/csrc san_attcols`` and run directly; no GPU code is involved
and nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_staging_rule_and_table_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_attcols"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_attcols")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) cases", r.stdout)
    # 2 x (4 subsets + 256 NULL combinations), 12 inverted, 1 + 256 + 8 empty, and 2 or 3 a random set
    # of 240 (3 when it has two rows or more: the program's seed is fixed, so the count is)
    assert m and int(m.group(1)) == 2 * 260 + 12 + 265 + 2 * 240 + 176, r.stdout
    assert r.stderr == "", r.stderr
