"""The pending-attestation pool's growth rules without a GPU: prysm_amd/csrc/attpool_dev.h -- a
column's live length, a reserve's capacities, a lane's share of the move and what an append would
add, the inlines pz_att_pool_move_kernel and pz_att_pool_need_kernel compile too -- on the CPU under
ASan+UBSan, driven by the stand-alone program prysm_amd/csrc/tests/attpool_reserve_san.cpp through a
sequential form of the move over buffers of exactly the old and new sizes, against a
vector-of-records model.  Built by ``make -C prysm_amd/csrc san_attpool_reserve`` and run directly;
no GPU code is involved and nothing is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_growth_rules_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_attpool_reserve"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_attpool_reserve")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) reserves, (\d+) no-ops, (\d+) columns moved, (\d+) bytes moved, (\d+) appends, (\d+) prunes, "
                 r"(\d+) need batches", r.stdout)
    assert m, r.stdout
    reserves, noops, cols, nbytes, appends, prunes, needs = (int(x) for x in m.groups())
    # 6 lengths x 4 row counts x (7 alone + all) x 3 grids of the length table alone
    assert reserves >= 6 * 4 * 8 * 3 + 120 and noops >= 2 * 6 * 4 * 8 * 3
    assert cols == 16 * reserves and nbytes > 100000
    assert appends > 500 and prunes >= 120
    assert needs == 6 * 4  # 0, 1, 255, 256, 257, 513 rows x no take / take / take of zeros / inverted rows
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_san_list_builds_the_program():
    mk = open(os.path.join(ROOT, "prysm_amd", "csrc", "Makefile")).read()
    san = [ln for ln in mk.splitlines() if ln.startswith("san:")][0]
    assert "../../build/san_attpool_reserve" in san.split()
    rule = mk[mk.index("../../build/san_attpool_reserve:"):]
    rule = rule[:rule.index("\n\n")]
    assert "$(CXX)" in rule and "-fsanitize=address,undefined" in rule and "hipcc" not in rule.lower()
