"""The two states' encoding rules on the CPU under ASan+UBSan: prysm_amd/csrc/wire_state_dev.h (the
inlines the kernels of wire_state.hip compile too) driven by the stand-alone program
prysm_amd/csrc/tests/wire_state_san.cpp through a sequential form of the kernels' phases into buffers
of exactly the encoded size -- the varint length and put, the nested lengths of an entry and an
array, the head's scalar and record sizes right-aligned at the head bound, the tail placement and the
recent hashes -- against a byte-by-byte scalar encoder, over tests/state_wire_cases.py's list written
out in C and a few thousand random tables, heads and hash lists.  Built by
``make -C prysm_amd/csrc san_wirestate`` and run directly; no GPU code is involved and nothing is
loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_wire_rules_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_wirestate"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_wirestate")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) tables, (\d+) heads, (\d+) hash lists", r.stdout)
    assert m and int(m.group(1)) > 3000 and int(m.group(2)) > 2000 and int(m.group(3)) > 2000, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
