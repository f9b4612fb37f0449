"""Times the two attestation-digest kernels (attdigest.hip: Attestation.Key and the
processAttestation message digest from device columns) on N = 1,048,576 attestations with HIP
events, in two shapes: synth.attestation_columns_512 (ShardBlockHash 32 B, 11 oblique hashes:
Key 394 B) and the replay's (32 B, none: Key 42 B); the message is 2,154 B in both.

Beside each, the yardstick: pz_dev_blake2b512_batch (one lane per message, the same
compressions, no gather) over the same messages assembled on the host into a CSR buffer.  The
two digests are compared, so the probe is also a check at full size.  Per launch one event
pair; 3 warm-up launches, then the median of REPS (default 20).

    python tools/attdigest_probe.py [--n N] [--reps REPS] [--out DIR]   # DIR/probe.json"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from prysm_amd import _lib, blockchain, synth, types  # noqa: E402

if os.environ.get("PZ_PROBE_LIB"):
    _lib.library_path = os.environ["PZ_PROBE_LIB"]

N_RECENT = 128


def hdr10(first, shard):
    """(n, 10) uint8: PutUvarint(first) at offset 0, then PutUvarint(shard) at offset 0 over it."""
    def put(buf, x):
        more = np.ones(len(x), dtype=bool)
        for k in range(10):
            rest = x >> np.uint64(7 * k)
            b = (rest & np.uint64(0x7F)).astype(np.uint8)
            nxt = (rest >> np.uint64(7)) != 0 if k < 9 else np.zeros(len(x), dtype=bool)
            b[nxt] |= 0x80
            buf[more, k] = b[more]
            more &= nxt
    buf = np.zeros((len(first), 10), dtype=np.uint8)
    put(buf, first)
    put(buf, shard)
    return buf


def shape_columns(n, m, seed=2):
    """attestation_columns_512's columns with m oblique hashes per record."""
    c = synth.attestation_columns_512(n, seed)
    obl = c["oblique_parent_hashes"].reshape(n, synth.N_OBLIQUE, 32)[:, :m]
    c["oblique_parent_hashes"] = np.ascontiguousarray(obl).reshape(-1)
    c["oblique_offs"] = np.arange(n * m + 1, dtype=np.uint64) * np.uint64(32)
    c["oblique_first"] = np.arange(n + 1, dtype=np.uint64) * np.uint64(m)
    return c


def key_messages(c, n, m):
    sbh = c["shard_block_hash"].reshape(n, 32)
    obl = c["oblique_parent_hashes"].reshape(n, 32 * m)
    return np.concatenate([hdr10(c["slot"], c["shard_id"]), sbh, obl], axis=1)


def att_messages(c, n, m, pstart, recent):
    idx = pstart[:, None].astype(np.int64) + np.arange(64 - m)[None, :]
    parents = np.concatenate([recent[idx], c["oblique_parent_hashes"].reshape(n, m, 32)], axis=1)
    signed = np.concatenate([parents, np.full((n, 64, 1), 0x20, np.uint8)], axis=2).reshape(n, 64 * 33)
    return np.concatenate([hdr10(c["slot"] % np.uint64(64), c["shard_id"]), signed,
                           c["shard_block_hash"].reshape(n, 32)], axis=1)


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.n
    dev = torch.device("cuda", 0)
    sh = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def up(a, pad=0):
        a = np.ascontiguousarray(a)
        a = a.view(np.int64) if a.dtype == np.uint64 else a
        t = torch.zeros(a.size + pad, dtype=torch.from_numpy(a[:1]).dtype, device=dev)
        t[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
        return t

    def csr_time(msgs, out_bytes):
        """The yardstick over (n, L) messages; returns its timing and digests."""
        length = msgs.shape[1]
        d_msgs = up(msgs, pad=16)
        d_offs = up(np.arange(n + 1, dtype=np.uint64) * np.uint64(length))
        out = torch.empty((n, out_bytes), dtype=torch.uint8, device=dev)
        t = median_ms(lambda: _lib.lib.call("pz_dev_blake2b512_batch", d_msgs.data_ptr(), d_offs.data_ptr(), n,
                                            out.data_ptr(), out_bytes, sh), args.reps)
        return t, out

    rng = np.random.default_rng(5)
    recent = rng.integers(0, 256, size=(N_RECENT, 32), dtype=np.uint8)
    d_recent = up(recent).view(N_RECENT, 32)
    results = {"n": n, "reps": args.reps, "shapes": {}}
    for name, m in (("columns_512", synth.N_OBLIQUE), ("replay", 0)):
        c = shape_columns(n, m)
        d = {k: up(c[k], pad=4 if c[k].dtype == np.uint8 else 0)
             for k in ("slot", "shard_id", "shard_block_hash", "shard_block_hash_offs", "oblique_parent_hashes",
                       "oblique_offs", "oblique_first")}
        pstart = rng.integers(0, N_RECENT - 64 + 1, size=n).astype(np.uint64)
        d_status = torch.zeros(n, dtype=torch.int32, device=dev)  # PZ_ATT_PROCESSED
        d_pstart = up(pstart)
        row = {}
        keys = [None]

        def run_keys():
            keys[0] = types.attestation_keys_device(d, n, out_bytes=32)
        t_fused = median_ms(run_keys, args.reps)
        kmsgs = key_messages(c, n, m)
        t_csr, want = csr_time(kmsgs, 32)
        assert torch.equal(keys[0], want), "Key digests differ from the CSR hash of the same messages"
        row["key"] = {"msg_bytes": int(kmsgs.shape[1]), "fused_ms": t_fused[0], "fused_min_max": t_fused[1:],
                      "csr_ms": t_csr[0], "csr_min_max": t_csr[1:], "ratio": t_fused[0] / t_csr[0]}
        del kmsgs, want
        msgs = [None]

        def run_msgs():
            msgs[0] = blockchain.attestation_messages_device(d, n, d_status, d_pstart, d_recent, N_RECENT)
        t_fused = median_ms(run_msgs, args.reps)
        amsgs = att_messages(c, n, m, pstart, recent)
        t_csr, want = csr_time(amsgs, 64)
        assert torch.equal(msgs[0][0], want), "message digests differ from the CSR hash of the same messages"
        assert int(msgs[0][1].min().item()) == amsgs.shape[1] == int(msgs[0][1].max().item())
        row["message"] = {"msg_bytes": int(amsgs.shape[1]), "fused_ms": t_fused[0], "fused_min_max": t_fused[1:],
                          "csr_ms": t_csr[0], "csr_min_max": t_csr[1:], "ratio": t_fused[0] / t_csr[0]}
        del amsgs, want
        results["shapes"][name] = row
        for what in ("key", "message"):
            r = row[what]
            print("%-12s %-8s %5d B  fused %8.4f ms  csr %8.4f ms  ratio %.2f  (digests equal)"
                  % (name, what, r["msg_bytes"], r["fused_ms"], r["csr_ms"], r["ratio"]), flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "probe.json"), "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
