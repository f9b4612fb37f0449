"""Stored CrystallizedStates for the loader's tests (tests/test_unwire_state.py on the CPU,
tests/test_unwire_state_gpu.py on the device): canonical states built with ``prysm_amd.wire`` from
synthetic validators and committee arrays, the non-canonical corpus with the offset of each
violation worked out from how the bytes were put together, and the ground truth -- ``oracle.schema``'s
parse (Google's runtime) of the same bytes, as columns."""
import numpy as np

from oracle import schema
from prysm_amd import pb, wire

U64 = np.uint64
FULL = (1 << 64) - 1  # a 10-byte varint


def parse(raw):
    cs = schema.CrystallizedState()
    cs.ParseFromString(bytes(raw))
    return cs


def canonical(raw):
    """Acceptance: parse-then-SerializeToString reproduces the input."""
    return parse(raw).SerializeToString() == bytes(raw)


def truth(raw):
    """The parsed message as the loader's columns: what ``wire.unwire_crystallized_state`` must return."""
    cs = parse(raw)
    vs = cs.validators
    out = {k: np.array([getattr(v, k) for v in vs], U64)
           for k in ("public_key", "withdrawal_shard", "balance", "start_dynasty", "end_dynasty")}
    for k in ("withdrawal_address", "randao_commitment"):
        blobs = [bytes(getattr(v, k)) for v in vs]
        offs = np.zeros(len(vs) + 1, U64)
        offs[1:] = np.cumsum([len(b) for b in blobs], dtype=U64)
        out[k], out[k + "_offs"] = np.frombuffer(b"".join(blobs), np.uint8), offs
    tab = [[(e.shard_id, list(e.committee)) for e in a.array_shard_and_committee] for a in cs.shard_and_committees_for_slots]
    out.update(wire.committee_table(tab))
    out["nval"], out["narr"] = len(vs), len(tab)
    return out


def same_columns(got, want):
    assert got["nval"] == want["nval"] and got["narr"] == want["narr"]
    for k in wire.VALIDATOR_COLS + wire.TABLE_COLS:
        np.testing.assert_array_equal(got[k], want[k], k)


# ---- canonical states ------------------------------------------------------------------------------------
def state(vals=None, arrays=(), records=(), **head):
    kw = dict(last_state_recalc=64, current_dynasty=1, total_deposits=77)
    kw.update(head)
    return wire.crystallized_state(pb.CrystallizedState(crosslink_records=list(records), validators=vals or pb.Validators(),
                                                        shard_and_committees_for_slots=list(arrays), **kw))


def arrays_of(tab):
    return [pb.ShardAndCommitteeArray([pb.ShardAndCommittee(s, np.asarray(c, np.uint32)) for s, c in arr]) for arr in tab]


def full_validators(n, seed=0):
    """Every field at its longest: five 10-byte varints, a 20-byte address and a 32-byte commitment."""
    rng = np.random.default_rng(seed)
    big = lambda: rng.integers(1 << 63, FULL, size=n, dtype=U64, endpoint=True)  # noqa: E731
    return pb.Validators(n, big(), big(), [rng.bytes(20) for _ in range(n)], [rng.bytes(32) for _ in range(n)], big(), big(), big())


def fixed_validators(n, framed, seed=0):
    """n records whose framing (key, length, body) takes exactly ``framed`` bytes: 5 (a 2-byte
    balance), 37 (that and a 30-byte commitment) or 113 (full records)."""
    rng = np.random.default_rng(seed)
    if framed == 113:
        return full_validators(n, seed)
    bal = rng.integers(128, 1 << 14, size=n, dtype=U64)
    if framed == 5:
        return pb.Validators(n, balance=bal)
    assert framed == 37
    return pb.Validators(n, balance=bal, randao_commitment=[rng.bytes(30) for _ in range(n)])


def mixed_validators(n, seed=0, blobs=None):
    """Records of every length from 2 (all fields zero) to full: each field present or not, every
    varint length; ``blobs(rng, i, k)`` supplies the bytes fields (None: random ones up to 20 / 32 bytes)."""
    rng = np.random.default_rng(seed)

    def scalar():
        bits = rng.integers(0, 65, size=n)
        x = rng.integers(0, FULL, size=n, dtype=U64, endpoint=True) >> (64 - bits).astype(U64)
        return np.where((bits == 0) | (rng.random(n) < 0.3), U64(0), x).astype(U64)

    def blob(k, cap):
        if blobs is not None:
            return [blobs(rng, i, k) for i in range(n)]
        return [rng.bytes(int(rng.integers(0, cap + 1))) if rng.random() < 0.6 else b"" for _ in range(n)]

    v = pb.Validators(n, scalar(), scalar(), blob(0, 20), blob(1, 32), scalar(), scalar(), scalar())
    for col in (v.public_key, v.withdrawal_shard, v.balance, v.start_dynasty, v.end_dynasty):
        col[0] = 0  # record 0: 5a 00 unless a bytes field says otherwise
        if n > 1:
            col[1] = FULL  # record 1: full
    if blobs is None:
        v.withdrawal_address[0] = v.randao_commitment[0] = b""
        if n > 1:
            v.withdrawal_address[1], v.randao_commitment[1] = rng.bytes(20), rng.bytes(32)
    return v


def record_lengths(raw):
    """The body length of every ValidatorRecord of a canonical state."""
    return [v.ByteSize() for v in parse(raw).validators]


# bytes that look like headers, for addresses and commitments: an empty record, a short one, an array
# header, and records whose length points past any tile
DECOYS = (b"\x5a\x00", b"\x5a\x05\x28\x01\x30\x01\x38", b"\x62\x01\x0a", b"\x5a\xff\x1f", b"\x5a\xfd\x03", b"\x5a\x7f",
          b"\x5a\x00\x5a\x00\x5a\x00", b"\x5a\x02\x28\x05")


def decoy_blob(rng, i, k):
    parts = [DECOYS[int(j)] for j in rng.integers(0, len(DECOYS), size=int(rng.integers(1, 4)))]
    return b"".join(parts)[:20 if k == 0 else 32]


# ---- the non-canonical corpus ------------------------------------------------------------------------------
HEAD = b"\x08\x40"  # last_state_recalc 64


def R(body):
    return b"\x5a" + wire.varint(len(body)) + body


def A(body):
    return b"\x62" + wire.varint(len(body)) + body


def E(body):
    return b"\x0a" + wire.varint(len(body)) + body


REC = R(b"\x28\x05")                               # balance 5
ARR = A(E(b"\x08\x03\x12\x03\x01\xac\x02"))        # shard 3, members 1 and 300


def corpus():
    """``[(name, bytes, offset)]``: each input is PZ_EINVAL at ``offset``, the key byte of the first
    field that breaks the rule (for a run that ends where no header stands: that position)."""
    pre = HEAD + REC
    at = len(pre)
    cases = [
        ("a non-minimal length in a record header", pre + b"\x5a\x82\x00\x28\x05" + REC, at),
        ("a record length past the end", pre + b"\x5a\x10\x28\x05", at),
        ("a last record truncated", pre + R(b"\x28\x85\x01")[:-1], at),
        ("fields 6 and 7 swapped", pre + R(b"\x38\x01\x30\x01") + REC, at + 4),
        ("a zero scalar present", pre + R(b"\x28\x00") + REC, at + 2),
        ("an empty bytes field present", pre + R(b"\x1a\x00") + REC, at + 2),
        ("an unknown field 8 in a record", pre + R(b"\x28\x05\x40\x01") + REC, at + 4),
        ("field 12 before field 11", HEAD + ARR + REC, len(HEAD + ARR)),
        ("a second run of field 11 after field 12", pre + ARR + REC, len(pre + ARR)),
        ("unpacked members", pre + A(E(b"\x08\x03\x10\x01\x10\x02")), at + 6),
        ("a member varint cut by the field's end", pre + ARR + A(E(b"\x12\x02\x01\x81")), len(pre + ARR) + 4),
        ("a 6-byte member", pre + A(E(b"\x12\x08\x01\x80\x80\x80\x80\x80\x01\x02")), at + 7),
        ("trailing bytes after the message", pre + ARR + b"\x00", len(pre + ARR)),
        ("a 5-byte member above 2^32 - 1", pre + A(E(b"\x12\x06\x07\xff\xff\xff\xff\x1f")), at + 7),
        ("a member with a zero last byte", pre + A(E(b"\x12\x03\x07\x81\x00")), at + 7),
        ("an array with an unknown field", pre + A(b"\x12\x00"), at + 2),
        ("a zero shard present", pre + A(E(b"\x08\x00")), at + 4),
        ("an empty packed field present", pre + A(E(b"\x12\x00")), at + 4),
    ]
    for name, raw, _ in cases:  # (the runtime keeps an unknown field and emits it again: Marshal of the reference's struct cannot)
        assert "unknown" in name or not canonical_or_error(raw), name
    return cases


def canonical_or_error(raw):
    try:
        return canonical(raw)
    except Exception:  # (the runtime refuses what does not parse at all)
        return False


def corpus_file(path, entries):
    """The sanitizer program's input: ``entries`` of ``(status, offset or None, bytes)``."""
    with open(path, "wb") as f:
        for status, off, raw in entries:
            f.write(int(status).to_bytes(1, "little", signed=True))
            f.write(((1 << 64) - 1 if off is None else int(off)).to_bytes(8, "little"))
            f.write(len(raw).to_bytes(4, "little"))
            f.write(bytes(raw))
