"""The attestation store's rule without a GPU: prysm_amd/csrc/blockstore_dev.h -- which rows of a run
blockProcessing saves (service.go:281-301) and the dwords of the appended list entries, the inlines
the kernels of blockstore.hip compile too -- on the CPU under ASan+UBSan, driven by the stand-alone
program prysm_amd/csrc/tests/blockstore_san.cpp through a sequential form of select and of the dword
writer over buffers of exactly the stated sizes, against a vector-of-records model.  Built by
``make -C prysm_amd/csrc san_blockstore`` and run directly; no GPU code is involved and nothing is
loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_store_rule_clean_and_consistent_under_sanitizer():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_blockstore"], check=True)
    r = subprocess.run([os.path.join(ROOT, "build", "san_blockstore")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok: (\d+) selects, (\d+) rows saved, (\d+) list entries", r.stdout)
    assert m, r.stdout
    selects, saved, entries = (int(x) for x in m.groups())
    assert selects == 6 * 3 * 3 * 2  # 0, 1, 255, 256, 257, 513 rows x random / all / none x stop 0 / middle / nblocks x rec_status or NULL
    assert saved >= 2 * (1 + 255 + 256 + 257 + 513)  # the all-saved runs at stop == nblocks alone
    assert entries == 0 + 1 + 2 + 3 + 255 + 256 + 257 + 513
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr


def test_san_list_builds_the_program():
    mk = open(os.path.join(ROOT, "prysm_amd", "csrc", "Makefile")).read()
    san = [ln for ln in mk.splitlines() if ln.startswith("san:")][0]
    assert "../../build/san_blockstore" in san.split()
    rule = mk[mk.index("../../build/san_blockstore:"):]
    rule = rule[:rule.index("\n\n")]
    assert "$(CXX)" in rule and "-fsanitize=address,undefined" in rule and "hipcc" not in rule.lower()
    assert "blockstore.hip" in [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0].split()


def test_the_header_states_the_rule_for_plain_cxx():
    src = open(os.path.join(ROOT, "prysm_amd", "csrc", "blockstore_dev.h")).read()
    for cite in ("service.go:308", ":288-297", ":304", "service.go:261-269", "core.go:650-658", "core.go:745-760"):
        assert cite in src, cite
    assert "refused whole" in src
    kernels = open(os.path.join(ROOT, "prysm_amd", "csrc", "blockstore.hip")).read()
    assert '#include "blockstore_dev.h"' in kernels and '#include "tile_scan.h"' in kernels
    assert "bs_row_saved(" in kernels and "bs_list_dword(" in kernels and "bs_first(" in kernels
