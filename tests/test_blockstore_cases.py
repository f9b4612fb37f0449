"""The attestation store's cases on the CPU, from the oracle's records alone (blockstore_cases.py): each
of the seven cases the rule is about occurs in the case chain, a block past a transition is deferred,
and ``blockchain.store_writes`` on hand-made dicts gives the reference's writes in its order."""
import numpy as np

from oracle import ref
from oracle import replay as oreplay
from prysm_amd import blockchain as bc
from blockstore_cases import ATT_PREFIX, LIST_PREFIX, ModelDB, case_chain, model_db, oracle_records, saved_rows


def test_each_case_occurs_in_the_case_chain():
    blocks, eligible, at = case_chain()
    recs, chain = oracle_records(blocks, eligible)
    saved = saved_rows(recs)
    status = lambda name: recs[at[name]]["status"]  # noqa: E731
    ok = lambda name: ["key" in a for a in recs[at[name]]["atts"]]  # noqa: E731
    # a block whose parent was never saved: the loop is never reached
    assert status("orphan") == "no_parent" and recs[at["orphan"]]["atts"] == [] and len(blocks[at["orphan"]].attestations) == 1
    # the last attestation fails after accepted ones: the block is dropped, the accepted rows are saved
    assert status("last fails") == "attestations_rejected" and ok("last fails") == [True, True, False]
    # the first fails, the last passes: the block goes on
    assert status("first fails") in ("processed", "saved_not_candidate") and ok("first fails") == [False, True]
    # an ineligible block: the chain never saw it, its record (from a copy) saves its row
    assert eligible[at["ineligible"]] == 0 and eligible.sum() == len(blocks) - 1
    assert ok("ineligible") == [True] and recs[at["ineligible"]]["hash"] not in chain.saved
    # a block received twice in one run, and one received again in a later run
    assert recs[at["twice"]]["hash"] == recs[at["chain 18"]]["hash"] and at["twice"] == at["chain 18"] + 1
    assert ok("twice") == [True] and ok("chain 18") == [True]
    assert recs[at["again later"]]["hash"] == recs[at["chain 64"]]["hash"] and ok("again later") == ok("chain 64") == [True]
    # two accepted attestations with equal Key and different bytes
    a, b = recs[at["equal key"]]["atts"]
    assert a["key"] == b["key"] and a["hash"] != b["hash"]
    # a block with no attestations
    assert blocks[at["no attestations"]].attestations == [] and status("no attestations") == "attestations_rejected"
    # the chain itself goes on undisturbed, through its transition block
    assert [recs[at["chain %d" % k]]["status"] for k in range(70)] == ["processed"] * 70
    trans = [j for j, r in enumerate(recs) if r["transition"] and eligible[j]]
    assert trans == [at["chain 63"]]
    # a run handed all the blocks stops behind the block that promotes the transition block's states:
    # every block past it is deferred, rows to save among them
    stop = at["chain 64"] + 1
    assert stop < len(blocks) and sum(saved[stop:]) >= 5 and at["again later"] >= stop
    # the model database: a key is overwritten, a list is appended to
    db = model_db(blocks, recs).data
    assert len([k for k in db if k.startswith(ATT_PREFIX)]) == len({a["key"] for r in recs for a in r["atts"] if "key" in a})
    assert len({a["key"] for r in recs for a in r["atts"] if "key" in a}) < sum(saved)
    lists = {k[len(LIST_PREFIX):]: v for k, v in db.items() if k.startswith(LIST_PREFIX)}
    assert len(lists[recs[at["twice"]]["hash"]]) == 2 * 34 and len(lists[recs[at["chain 64"]]["hash"]]) == 2 * 34
    assert len(lists[recs[at["last fails"]]["hash"]]) == 2 * 34 and len(lists[recs[at["equal key"]]["hash"]]) == 2 * 34
    assert recs[at["orphan"]]["hash"] not in lists and recs[at["no attestations"]]["hash"] not in lists
    assert sum(len(v) for v in lists.values()) == 34 * sum(saved)
    # the later value stays under the equal key: the second record's bytes
    second = oreplay.to_pb_block(blocks[at["equal key"]]).attestations[1]
    assert db[ATT_PREFIX + b["key"]] == ref.marshal(second)


def hand_made(first, nrec=None):
    """A dict as ResidentChain returns it, made by hand: record i of ``data`` is 3 + i bytes long."""
    m = int(first[-1]) if nrec is None else nrec
    ends = np.cumsum([3 + i for i in range(m)]).astype(np.uint64)
    span = np.stack([ends - (3 + np.arange(m, dtype=np.uint64)), ends], axis=1) if m else np.zeros((0, 2), np.uint64)
    key = (np.arange(32 * m) % 251).astype(np.uint8).reshape(m, 32)
    hash_ = (np.arange(32 * m) % 241 + 1).astype(np.uint8).reshape(m, 32)
    lists = np.concatenate([np.concatenate([np.array([0x0a, 0x20], np.uint8), h]) for h in hash_] + [np.zeros(0, np.uint8)])
    n = len(first) - 1
    out = {"block_hash": (np.arange(32 * n) % 239).astype(np.uint8).reshape(n, 32),
           "store": {"rows": np.arange(m, dtype=np.uint32), "first": np.array(first, np.uint64), "span": span, "key": key, "hash": hash_,
                     "lists": lists}}
    data = np.arange(int(ends[-1]) if m else 0, dtype=np.int64).astype(np.uint8)
    return out, data


def test_store_writes_on_hand_made_dicts():
    # three blocks: two rows, none, one row
    out, data = hand_made([0, 2, 2, 3])
    st, bh = out["store"], out["block_hash"]
    rec = lambda i: data[int(st["span"][i, 0]):int(st["span"][i, 1])].tobytes()  # noqa: E731
    entry = lambda i: b"\x0a\x20" + st["hash"][i].tobytes()  # noqa: E731
    w = list(bc.store_writes(out, data))
    assert w == [(b"attestation-" + st["key"][0].tobytes(), rec(0), False), (b"attestation-" + st["key"][1].tobytes(), rec(1), False),
                 (b"attestationHashes-" + bh[0].tobytes(), entry(0) + entry(1), True),
                 (b"attestation-" + st["key"][2].tobytes(), rec(2), False),
                 (b"attestationHashes-" + bh[2].tobytes(), entry(2), True)]
    assert [len(v) for _, v, _ in w] == [3, 4, 68, 5, 34]
    # bytes objects and arrays alike
    assert list(bc.store_writes(out, data.tobytes())) == w
    # applied twice the lists grow and the keys stay: a block received twice
    db = ModelDB()
    db.apply_writes(w)
    db.apply_writes(bc.store_writes(out, data))
    assert db.data[b"attestationHashes-" + bh[0].tobytes()] == 2 * (entry(0) + entry(1))
    assert db.data[b"attestation-" + st["key"][1].tobytes()] == rec(1) and len(db.data) == 5


def test_store_writes_of_an_empty_batch():
    for first in ([0], [0, 0], [0, 0, 0, 0]):  # no block; blocks that saved nothing (m == 0)
        out, data = hand_made(first)
        assert out["store"]["lists"].size == 0 and list(bc.store_writes(out, data)) == []
