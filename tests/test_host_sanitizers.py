"""Host code under sanitizers (SURVEY.md §5 race detection): the serial BLAKE2b hasher and its
thread pool (prysm_amd/csrc/serial_hash.cpp) built with ASan+UBSan and with TSan, and the
canonical-form rule's walks over both cursors (prysm_amd/csrc/proto3_canon.h) built with
ASan+UBSan, by ``make -C prysm_amd/csrc san``, run on the CPU.  No GPU code is involved."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def san_build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san"], check=True)
    return os.path.join(ROOT, "build")


@pytest.mark.parametrize("kind", ["asan", "tsan"])
def test_serial_hasher_clean_under_sanitizer(san_build, kind):
    prog = os.path.join(san_build, "san_" + kind)
    r = None
    if kind == "tsan" and shutil.which("setarch"):
        # TSan's runtime lays out its shadow memory around fixed address ranges before main();
        # on a kernel with more address-space randomisation bits than the runtime knows, the
        # program sometimes lands outside them and dies there ("unexpected memory mapping", or
        # a bare SIGSEGV).  Randomisation is switched off for this one child; the program and
        # what is asserted of it are unchanged.
        r = subprocess.run(["setarch", platform.machine(), "-R", prog], capture_output=True, text=True, timeout=300)
        if r.returncode != 0 and r.stderr.startswith("setarch:"):  # setarch itself was refused
            r = None
    if r is None:
        r = subprocess.run([prog], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok"), r.stdout
    assert "ERROR" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr, r.stderr


def test_canonical_walks_clean_and_consistent_under_sanitizer(san_build, tmp_path):
    """Both cursors over the whole corpus, each case with the protobuf runtime's verdict, and
    over the program's mutants of the canonical cases (prysm_amd/csrc/tests/proto3_canon_san.cpp)."""
    from canon_corpus import san_corpus_file

    corpus = tmp_path / "canon_corpus.bin"
    corpus.write_bytes(san_corpus_file())
    r = subprocess.run([os.path.join(san_build, "san_canon"), str(corpus)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok"), r.stdout
    assert "ERROR" not in r.stderr, r.stderr
