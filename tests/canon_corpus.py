"""The canonical-form corpus: serialized AttestationRecords and BeaconBlocks
that are, or are not, the encoding of their own decoding.  One set of tables for the GPU tests
of the decoder (test_unwire_gpu.py) and of the engine (test_canonical_gpu.py) and for the CPU
sanitizer run of the shared walks (test_host_sanitizers.py).

Import-light on purpose: the canonical encodings come from Google's protobuf runtime over the
oracle schema, the rest is bytes written out by hand; nothing of the product is imported."""
import struct

from google.protobuf import unknown_fields
from google.protobuf.message import DecodeError

from oracle import schema as opb


def varint(x):
    out = bytearray()
    while x >= 0x80:
        out.append((x & 0x7F) | 0x80)
        x >>= 7
    out.append(x)
    return bytes(out)


def frame(num, body):
    """``body`` as the length-delimited field ``num``."""
    return varint((num << 3) | 2) + varint(len(body)) + body


# ---- what "canonical" means: the protobuf runtime's verdict -------------------------------------
def has_unknown(m):
    return bool(len(unknown_fields.UnknownFieldSet(m))) or any(has_unknown(a) for a in getattr(m, "attestations", ()))


def canonical(raw, cls=opb.AttestationRecord):
    m = cls()
    try:
        m.ParseFromString(raw)
    except DecodeError:
        return False
    return not has_unknown(m) and m.SerializeToString() == raw


# ---- records (tests/test_unwire_gpu.py) ---------------------------------------------------------
A = opb.AttestationRecord(slot=5, shard_id=300, justified_slot=1 << 40, justified_block_hash=b"\x11" * 32,
                          shard_block_hash=b"\x22" * 32, attester_bitfield=b"\xff\x80",
                          oblique_parent_hashes=[b"\x33" * 32, b""],
                          aggregate_sig=[5, (1 << 64) - 1]).SerializeToString()
CORPUS = {
    "as encoded": A,
    "10-byte varint ending 0x01": b"\x08" + b"\xff" * 9 + b"\x01",
    "the empty record": b"",
    "empty field-7 element": b"\x3a\x00",
    "truncated by one byte": A[:-1],
    "10-byte varint ending 0x02": b"\x08" + b"\xff" * 9 + b"\x02",
    "11-byte varint": b"\x08" + b"\xff" * 10 + b"\x01",
    "08 85 00": b"\x08\x85\x00",
    "08 00": b"\x08\x00",
    "field 9 appended": A + b"\x48\x01",
    "field 1 with wire type 2": b"\x0a\x01\x00",
    "field 8 unpacked": b"\x40\x05",
    "2a 05 01 (length past the end)": b"\x2a\x05\x01",
    "a length of 2^63": b"\x2a" + varint(1 << 63) + b"\x01\x02",
    "field number 0": b"\x00\x01",
    "42 01 80 (packed varint cut)": b"\x42\x01\x80",
    "10 01 08 01 (order)": b"\x10\x01\x08\x01",
    "08 01 08 02 (repeat)": b"\x08\x01\x08\x02",
    "2a 00": b"\x2a\x00",
    "field-7 run broken by field 8 and resumed": b"\x3a\x01\xaa\x42\x01\x05\x3a\x01\xbb",
}
CANONICAL_CASES = {"as encoded", "10-byte varint ending 0x01", "the empty record", "empty field-7 element"}
FRAMED = {name: frame(8, c) for name, c in CORPUS.items()}
FRAMED.update({
    "non-minimal frame length": b"\x42\x82\x00\x08\x01",
    "frame length one short of the span": b"\x42\x01\x08\x01",
    "frame length one long of the span": b"\x42\x03\x08\x01",
})

# ---- blocks (tests/test_canonical_gpu.py) -------------------------------------------------------
ATT = dict(slot=0, shard_id=3, justified_slot=0, shard_block_hash=b"\x11" * 32, attester_bitfield=b"\xff\x00",
           oblique_parent_hashes=[b"\x22" * 32], aggregate_sig=[5, 7])


def block(atts=(ATT,), ts=(8, 0)):
    """The block of the tables with these attestations and this (seconds, nanos) timestamp: a set
    Timestamp message is emitted even when both are zero."""
    m = opb.BeaconBlock(parent_hash=b"\x01" * 32, slot_number=1, attestations=[opb.AttestationRecord(**a) for a in atts])
    m.timestamp.SetInParent()
    m.timestamp.seconds, m.timestamp.nanos = ts
    return m.SerializeToString()


E = block()
HEAD = E[:E.index(b"\x42")]  # everything before the attestation field
ATT_BYTES = opb.AttestationRecord(**ATT).SerializeToString()

NONCANONICAL = {
    "slot field repeated at the end": E + b"\x10\x01",
    "non-minimal varint (slot)": E.replace(b"\x10\x01", b"\x10\x81\x00", 1),
    "fields out of order": E.replace(b"\x10\x01", b"", 1) + b"\x10\x01",
    "explicit empty bytes (randao_reveal)": E.replace(b"\x10\x01", b"\x10\x01\x1a\x00", 1),
    "explicit zero scalar in the timestamp": E.replace(b"\x3a\x02\x08\x08", b"\x3a\x04\x08\x08\x10\x00", 1),
    "timestamp nanos beyond int32 (Marshal re-encodes the truncated int32)":
        E.replace(b"\x3a\x02\x08\x08", b"\x3a\x08\x08\x08\x10" + varint((1 << 32) + 5), 1),
    "attestation: explicit zero slot": HEAD + frame(8, b"\x08\x00" + ATT_BYTES),
    "attestation: field 7 run broken by field 8 then 7 again": HEAD + frame(8, ATT_BYTES + frame(7, b"\x33" * 32)),
    "attestation: empty packed signature": HEAD + frame(8, ATT_BYTES + b"\x42\x00"),
    "attestation: non-minimal length prefix": HEAD + b"\x42" + bytes([0x80 | len(ATT_BYTES), 0x00]) + ATT_BYTES
    if len(ATT_BYTES) < 128 else None,
}
CANONICAL = {
    "as encoded": E,
    "empty oblique element (every element is emitted)": block([{**ATT, "oblique_parent_hashes": [b""]}]),
    "empty timestamp message (a set message is emitted)": block(ts=(0, 0)),
    "no attestations": block(atts=()),
    "negative timestamp seconds (10-byte varint)": block(ts=(-5, 0)),
    "negative nanos (sign-extended 10-byte varint)": block(ts=(1, -3)),
}
# golang/protobuf re-emits an unknown field, so the runtime calls this one canonical; the engine
# does not model unrecognized fields and rejects it (test_canonical_gpu.test_unknown_fields_rejected)
UNKNOWN_FIELD_BLOCK = E + b"\x48\x01"


# ---- the file prysm_amd/csrc/tests/proto3_canon_san.cpp reads -----------------------------------
def san_corpus_file():
    """Every case, with the runtime's verdict: bare records, records framed as field 8 (walked as
    blocks whose record spans are walked as records) and whole blocks.  Entries of {kind u8 (0
    record, 1 block), verdict u8, length u32 little-endian, bytes}."""
    cases = [(0, c) for c in CORPUS.values()] + [(1, c) for c in FRAMED.values()]
    cases += [(1, c) for c in list(NONCANONICAL.values()) + list(CANONICAL.values()) + [UNKNOWN_FIELD_BLOCK] if c is not None]
    cls = (opb.AttestationRecord, opb.BeaconBlock)
    return b"".join(struct.pack("<BBI", kind, canonical(c, cls[kind]), len(c)) + c for kind, c in cases)
