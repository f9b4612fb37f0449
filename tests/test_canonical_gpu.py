"""The block engine accepts exactly the canonical proto3 encodings: the
reference hashes proto.Marshal of the DECODED block (types/block.go:69), so an input that is
not the canonical encoding of its own decoding would hash differently from its bytes; the
engine rejects it with PZ_EINVAL instead of guessing.  Each case (tests/canon_corpus.py) is a
decodable BeaconBlock whose re-encoding differs from its bytes (or, for the accepted cases, does
not), decided here independently by Google's protobuf runtime over the oracle schema."""
import numpy as np
import pytest

from canon_corpus import CANONICAL, NONCANONICAL, UNKNOWN_FIELD_BLOCK
from oracle import schema as opb
from prysm_amd import _lib
from prysm_amd.blockchain import BeaconChain

pytestmark = pytest.mark.gpu


def canonical_by_runtime(raw):
    m = opb.BeaconBlock()
    m.ParseFromString(raw)
    return m.SerializeToString() == raw


def run(raw):
    data = np.frombuffer(raw + bytes(16), dtype=np.uint8)
    offs = np.array([0, len(raw)], dtype=np.uint64)
    BeaconChain(1024).process_serialized(data, offs)


@pytest.mark.parametrize("name", [k for k, v in NONCANONICAL.items() if v is not None])
def test_noncanonical_rejected(name):
    raw = NONCANONICAL[name]
    assert not canonical_by_runtime(raw), name  # the case really is non-canonical
    with pytest.raises(_lib.PzError) as e:
        run(raw)
    assert e.value.code == _lib.PZ_EINVAL


@pytest.mark.parametrize("name", list(CANONICAL))
def test_canonical_accepted(name):
    raw = CANONICAL[name]
    assert canonical_by_runtime(raw), name
    run(raw)


def test_unknown_fields_rejected():
    """Deliberately stricter than the reference: golang/protobuf keeps an unknown field in
    XXX_unrecognized and re-emits it at the end, so Marshal(decode(x)) == x there; the engine
    does not model unrecognized fields and rejects the block (PZ_EINVAL) rather than hash
    bytes it does not understand."""
    raw = UNKNOWN_FIELD_BLOCK
    assert canonical_by_runtime(raw)
    with pytest.raises(_lib.PzError) as e:
        run(raw)
    assert e.value.code == _lib.PZ_EINVAL
