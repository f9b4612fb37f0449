"""Cases of the attestation store batch (prysm_amd/csrc/blockstore_dev.h; ResidentChain.store), shared
by the CPU test (test_blockstore_cases.py) and the GPU tests (test_blockstore_gpu.py):

* ``ModelDB``: the reference's database as a dict, driven by the oracle's records exactly as
  blockchain/service.go:281-301 writes through core.go:650-658 (saveAttestation: db.Put under
  ``attestation-`` + Key(), a key written twice keeps the later value) and core.go:745-760
  (saveAttestationHash: the list under ``attestationHashes-`` + the block's hash read, appended to
  and put back);
* ``case_chain()``: blocks 0..69 of the 130-block chain (the transition block is index 63 of them),
  with the blocks the store's rule is about placed among them as siblings of chain blocks, so that
  the chain itself goes on undisturbed, and ``five_cycles()``: synth.chain_blocks(1024, 330) as it is;
* ``oracle_records()``: oracle.replay.Chain stepped block by block.  The oracle has no
  CanProcessBlock, so an ineligible block's record comes from a ``copy.deepcopy`` of the chain: the
  reference processes its attestations and saves them (service.go:281-301), then drops the block at
  :308 without touching any state."""
import copy
import functools

import numpy as np

from oracle import ref
from oracle import replay as oreplay
from prysm_amd import pb
from test_blockparents_gpu import chain130

NVAL = 1024
ATT_PREFIX, LIST_PREFIX = b"attestation-", b"attestationHashes-"  # blockchain/schema.go:31-34


class ModelDB:
    """The attestation part of the reference's key-value store."""

    def __init__(self):
        self.data = {}

    def save_attestation(self, key, value):
        self.data[ATT_PREFIX + bytes(key)] = bytes(value)  # core.go:650-658

    def save_attestation_hash(self, block_hash, att_hash):
        k = LIST_PREFIX + bytes(block_hash)  # core.go:745-760: proto.Marshal(AttestationHashes{append(list, hash)})
        self.data[k] = self.data.get(k, b"") + b"\x0a\x20" + bytes(att_hash)

    def apply_record(self, rec, block):
        """What the loop of service.go:281-301 writes for one block, from the oracle's record of it."""
        atts = oreplay.to_pb_block(block).attestations
        assert len(rec["atts"]) in (0, len(atts))  # (no_parent: the loop is never reached)
        for a, r in zip(atts, rec["atts"]):
            if "key" in r:
                self.save_attestation(r["key"], ref.marshal(a))
                self.save_attestation_hash(rec["hash"], r["hash"])

    def apply_writes(self, writes):
        """``blockchain.store_writes``'s triples."""
        for key, value, append in writes:
            self.data[key] = (self.data.get(key, b"") if append else b"") + value


def _sibling(block, **changes):
    """A copy of ``block`` with other contents: same parent and slot, another hash."""
    b = copy.deepcopy(block)
    b.randao_reveal = bytes(x ^ 0x5A for x in bytes(b.randao_reveal))
    for k, v in changes.items():
        setattr(b, k, v)
    return b


def _refused(a):
    """``a`` as processAttestation refuses it without a panic later on: another justified slot
    (core.go:255-259); calculateBlockVoteCache derives its parents and committee all the same."""
    b = copy.deepcopy(a)
    b.justified_slot = a.justified_slot + 7
    return b


@functools.lru_cache(maxsize=None)
def _case_chain():
    base = chain130()[:70]
    blocks, eligible, at = [], [], {}

    def put(name, block, el=1):
        at[name] = len(blocks)
        blocks.append(block)
        eligible.append(el)

    for k, b in enumerate(base):
        put("chain %d" % k, b)
        good = b.attestations[0]
        if k == 10:  # its parent was never saved: nothing of it is written (service.go:261-269)
            put("orphan", _sibling(b, parent_hash=b"\xEE" * 32))
        if k == 12:  # accepted rows, then the last one fails: the block is dropped at :304, after the saves
            put("last fails", _sibling(b, attestations=[copy.deepcopy(good), copy.deepcopy(good), _refused(good)]))
        if k == 14:  # the first fails, the last passes: the block goes on, the passed rows are saved
            put("first fails", _sibling(b, attestations=[_refused(good), copy.deepcopy(good)]))
        if k == 16:  # CanProcessBlock fails: tested at :308, after the saves
            put("ineligible", _sibling(b), el=0)
        if k == 18:  # the same bytes again, in the same run: its list grows
            put("twice", copy.deepcopy(b))
        if k == 20:  # two accepted attestations with equal Key (the signature is not part of it): the later value stays
            other = copy.deepcopy(good)
            other.aggregate_sig = [int(x) + 1 for x in good.aggregate_sig]
            put("equal key", _sibling(b, attestations=[copy.deepcopy(good), other]))
        if k == 22:
            put("no attestations", _sibling(b, attestations=[]))
    put("again later", copy.deepcopy(base[64]))  # received again in a later run: behind the deferred blocks
    return blocks, np.array(eligible, np.uint8), at


def case_chain():
    """``(blocks, eligible, at)``: the blocks, CanProcessBlock's answer per block, and where each case sits."""
    blocks, eligible, at = _case_chain()
    return copy.deepcopy(blocks), eligible.copy(), dict(at)


def five_cycles():
    from prysm_amd import synth

    return synth.chain_blocks(NVAL, 330, seed=4)


def oracle_records(blocks, eligible=None, chain=None):
    """``(records, chain)``: the oracle's record of every block and the chain behind the last one.  An
    ineligible block is processed on a copy of the chain, which is then thrown away."""
    chain = oreplay.Chain(NVAL) if chain is None else chain
    recs = []
    for j, b in enumerate(blocks):
        if eligible is not None and not eligible[j]:
            recs.append(copy.deepcopy(chain).process_block(oreplay.to_pb_block(b)))
        else:
            recs.append(chain.process_block(oreplay.to_pb_block(b)))
    return recs, chain


def model_db(blocks, recs):
    db = ModelDB()
    for b, r in zip(blocks, recs):
        db.apply_record(r, b)
    return db


def saved_rows(recs):
    """Per block, how many rows the reference saves."""
    return [sum("key" in a for a in r["atts"]) for r in recs]


__all__ = ["ModelDB", "NVAL", "case_chain", "five_cycles", "model_db", "oracle_records", "saved_rows", "pb"]
