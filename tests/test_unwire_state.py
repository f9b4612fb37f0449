"""The host side of the stored CrystallizedState's loader: pz_cstate_head (fields 1-10, host only)
against oracle.schema's parse (Google's runtime) of the same bytes, and the loader's rules
(prysm_amd/csrc/unwire_state_dev.h) on the CPU under ASan+UBSan through the stand-alone program
prysm_amd/csrc/tests/unwire_state_san.cpp over canonical states and the non-canonical corpus of
tests/unwire_state_cases.py.  No GPU, nothing loaded into Python but the product library's host call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import unwire_state_cases as uc
from oracle import ref
from prysm_amd import _lib, pb, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
HEAD_FIELDS = ("last_state_recalc", "justified_streak", "last_justified_slot", "last_finalized_slot", "current_dynasty",
               "crosslinking_start_shard", "total_deposits", "dynasty_seed", "dynasty_seed_last_reset")
FULL_HEAD = dict(zip(HEAD_FIELDS, (1 << 40, 3, 1 << 63, 127, 2, 1023, uc.FULL, b"\x07" * 32, 300)))


def check_head(raw):
    """pz_cstate_head's outputs against the parsed message; returns the head."""
    cs = uc.parse(raw)
    assert cs.SerializeToString() == raw
    h = wire.cstate_head(raw)
    s, r = h["scalars"], h["rest"]
    got = (int(s[0]), int(s[1]), int(s[2]), int(s[3]), int(s[4]), int(r.crosslinking_start_shard), int(s[5]),
           bytes(r.dynasty_seed)[:r.dynasty_seed_len], int(r.dynasty_seed_last_reset))
    assert got == tuple(getattr(cs, k) for k in HEAD_FIELDS)
    assert not s[6:].any()
    recs = cs.crosslink_records
    assert len(h["rec_dynasty"]) == len(recs)
    np.testing.assert_array_equal(h["rec_dynasty"], np.array([x.dynasty for x in recs], U64))
    np.testing.assert_array_equal(h["rec_slot"], np.array([x.slot for x in recs], U64))
    offs = h["rec_hash_offs"]
    assert [h["rec_hash"][int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(recs))] == [bytes(x.blockhash) for x in recs]
    # the first byte behind field 10: where the runtime's encoding of the head alone ends
    head_only = uc.parse(raw)
    del head_only.validators[:]
    del head_only.shard_and_committees_for_slots[:]
    assert h["body_beg"] == len(head_only.SerializeToString())
    return h


def test_head_of_the_genesis_state():
    _, cs = ref.new_genesis_states(1024)
    h = check_head(ref.marshal(cs))
    assert len(h["rec_dynasty"]) == 1024


def test_head_with_1024_records_of_every_hash_length():
    rng = np.random.default_rng(5)
    recs = [pb.CrosslinkRecord(int(rng.integers(0, 1 << 40)) * (i % 3 > 0), rng.bytes((0, 1, 32, 33)[i % 4]), int(rng.integers(0, 1 << 20)) * (i % 5 > 0))
            for i in range(1024)]
    h = check_head(uc.state(uc.mixed_validators(7), uc.arrays_of([[(1, [2, 3])]]), recs, **FULL_HEAD))
    assert {int(b - a) for a, b in zip(h["rec_hash_offs"], h["rec_hash_offs"][1:])} == {0, 1, 32, 33}


def test_head_without_records_and_an_empty_message():
    check_head(uc.state(uc.mixed_validators(3), **FULL_HEAD))
    h = check_head(b"")
    assert h["body_beg"] == 0 and not h["scalars"].any()


@pytest.mark.parametrize("absent", HEAD_FIELDS)
def test_head_with_each_field_zero(absent):
    kw = dict(FULL_HEAD)
    kw[absent] = b"" if absent == "dynasty_seed" else 0
    check_head(uc.state(uc.mixed_validators(2), records=[pb.CrosslinkRecord(1, b"h" * 32, 2)], **kw))


def test_head_with_rec_cap_one_short():
    ct = _lib.ctypes
    raw = np.frombuffer(uc.state(records=[pb.CrosslinkRecord(i + 1, b"x" * i, i) for i in range(5)]), np.uint8)
    scalars, rest = np.zeros(8, U64), _lib.CstateRest()
    dyn, slot, hashes, offs = np.zeros(5, U64), np.zeros(5, U64), np.zeros(raw.size, np.uint8), np.zeros(6, U64)
    nrec, body = ct.c_uint64(0), ct.c_uint64(0)
    call = lambda cap: _lib.lib.dll.pz_cstate_head(raw.ctypes.data, raw.size, scalars.ctypes.data, ct.byref(rest), dyn.ctypes.data,  # noqa: E731
                                                   slot.ctypes.data, hashes.ctypes.data, offs.ctypes.data, cap, ct.byref(nrec),
                                                   ct.byref(body))
    assert call(4) == _lib.PZ_ERANGE and nrec.value == 5
    assert call(5) == _lib.PZ_OK and nrec.value == 5 and list(dyn) == [1, 2, 3, 4, 5] and list(offs) == [0, 0, 1, 3, 6, 10]
    assert _lib.lib.dll.pz_cstate_head(raw.ctypes.data, raw.size, None, ct.byref(rest), None, None, None, None, 0, ct.byref(nrec),
                                       ct.byref(body)) == _lib.PZ_EINVAL
    assert _lib.lib.dll.pz_cstate_head(None, raw.size, scalars.ctypes.data, ct.byref(rest), None, None, None, None, 0, ct.byref(nrec),
                                       ct.byref(body)) == _lib.PZ_EINVAL


@pytest.mark.parametrize("raw, offset", [
    (b"\x08\x40\x10\x01\x18\x80\x00\x20\x01", 4),         # field 3 as 80 00: not minimal
    (b"\x08\x40\x18\x01\x10\x01", 4),                      # field 2 behind field 3
    (b"\x08\x00", 0),                                      # a zero scalar present
    (b"\x08\x40\x42\x00", 2),                              # an empty seed present
    (b"\x08\x40\x52\x02\x08\x00", 4),                      # a crosslink record with a zero dynasty present
    (b"\x08\x40\x52\x04\x18\x01\x08\x01", 6),              # a crosslink record's fields out of order
    (b"\x08\x40\x68\x01", 2),                              # an unknown field 13
    (b"\x08\x40\x42" + bytes([65]) + b"s" * 65, 2),        # a seed the state's struct cannot hold
])
def test_head_violations_name_their_offset(raw, offset):
    with pytest.raises(_lib.PzError) as e:
        wire.cstate_head(raw)
    assert e.value.code == _lib.PZ_EINVAL and e.value.offset == offset


def test_the_rules_clean_and_consistent_under_sanitizer(tmp_path):
    """The stand-alone program over canonical states (verdict PZ_OK with the parsed counts) and the
    corpus (PZ_EINVAL at each case's offset, PZ_ERANGE at the record over the limit), then over
    three mutants of every byte of every short entry, where only ASan and UBSan judge."""
    if shutil.which(os.environ.get("CXX", "g++")) is None:
        pytest.skip("no C++ compiler: the sanitizer program cannot be built here")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "prysm_amd", "csrc"), "san_unwire_state"], check=True)
    _, genesis = ref.new_genesis_states(1024)
    tab = [[(0, []), (5, [1, 127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, (1 << 32) - 1])], [], [(7, [9])]]
    good = [ref.marshal(genesis), b"", uc.state(uc.mixed_validators(300, 1), uc.arrays_of(tab), **FULL_HEAD),
            uc.state(uc.mixed_validators(200, 2, uc.decoy_blob)), uc.state(uc.full_validators(40)),
            uc.state(pb.Validators(1, withdrawal_address=[b"a" * (_lib.CSTATE_RECORD_LIMIT - 4)]))]
    entries = [(0, None, g) for g in good]
    entries += [(_lib.PZ_EINVAL, off, raw) for _, raw, off in uc.corpus()]
    over = uc.HEAD + uc.REC + uc.R(b"\x1a" + wire.varint(_lib.CSTATE_RECORD_LIMIT - 3) + b"a" * (_lib.CSTATE_RECORD_LIMIT - 3))
    entries.append((_lib.PZ_ERANGE, len(uc.HEAD + uc.REC), over))
    path, verdicts = str(tmp_path / "corpus.bin"), str(tmp_path / "verdicts.txt")
    uc.corpus_file(path, entries)
    r = subprocess.run([os.path.join(ROOT, "build", "san_unwire_state"), path, verdicts], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout.startswith("ok: %d cases, " % len(entries)), r.stdout
    lines = [[int(x) for x in ln.split()] for ln in open(verdicts)]
    for raw, (status, _, nval, narr, nent, nmem) in zip(good, lines):
        want = uc.truth(raw)
        assert uc.canonical(raw)
        assert (status, nval, narr, nent, nmem) == (0, want["nval"], want["narr"], len(want["arr_shard"]), len(want["members"]))
