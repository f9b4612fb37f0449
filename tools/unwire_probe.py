"""Times the device decoder (prysm_amd/csrc/unwire.hip) with HIP events, 200 warm-up launches
and `reps` timed repetitions:

  records  pz_dev_unwire_attestations on the 1,048,576 x 512-B records of
           synth.attestation_records_512, alternating in the same process with
           pz_dev_wire_attestations on the same records' columns (the same bytes moved the other
           way), with the decoded columns checked against synth.attestation_columns_512;
  blocks   pz_dev_unwire_blocks + pz_dev_unwire_attestations on the 10,000-block configs[4]
           chain, against the engine's host parse of the same bytes (pz_debug_parse, as
           tools/parse_probe.py runs it; needs PZ_PROBE_LIB=build/ab/libprysm_hip.so).

Usage: unwire_probe.py [reps] [n] [records|blocks|all]"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from prysm_amd import _lib, synth, wire  # noqa: E402

if os.environ.get("PZ_PROBE_LIB"):
    _lib.library_path = os.environ["PZ_PROBE_LIB"]

PEAK = 8e12  # HBM bytes/s
WARMUP = 200


def dev(a):
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def timed(fns, reps):
    """Per-launch ms of each function: warmed up, then timed one launch at a time in turn."""
    for _ in range(WARMUP):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
          for _ in fns]
    for r in range(reps):
        for k, f in enumerate(fns):
            ev[k][r][0].record()
            f()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    return [np.array([a.elapsed_time(b) for a, b in e]) for e in ev]


def report(name, ms, count, unit, alg_bytes):
    med = float(np.median(ms))
    line = "%-30s %8.3f ms median  (min %.3f, max %.3f, %d launches)  %8.1f M %s/s" % (
        name, med, ms.min(), ms.max(), len(ms), count / med / 1e3, unit)
    if alg_bytes:
        line += "  %.1f MB algorithmic, %.1f%% of 8 TB/s" % (alg_bytes / 1e6, 100 * alg_bytes / (med * 1e-3) / PEAK)
    print(line, flush=True)


def decoder(d_bytes, d_begs, d_ends, n, nbytes=None):
    """One decode into columns allocated once; returns (launch, columns)."""
    out = wire.unwire_attestations_device(d_bytes, d_begs, d_ends, n, 0, nbytes)
    c = _lib.AttestationColsOut(*[out[k].data_ptr() for k in wire.ATT_OUT_COLS])
    scr = torch.empty(int(_lib.lib.dll.pz_unwire_attestations_scratch_bytes(n)), dtype=torch.uint8, device="cuda")
    sh = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        _lib.lib.call("pz_dev_unwire_attestations", d_bytes.data_ptr(), d_begs.data_ptr(), d_ends.data_ptr(), n, 0,
                      ctypes.byref(c), out["totals"].data_ptr(), scr.data_ptr(), sh)

    return run, out


def records(reps, n):
    cols = synth.attestation_columns_512(n, seed=2)
    recs = synth.attestation_records_512(n, seed=2)
    d_bytes = torch.zeros(n * 512 + 16, dtype=torch.uint8, device="cuda")
    d_bytes[:n * 512] = torch.from_numpy(recs.reshape(-1)).cuda()
    d_offs = dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(512))
    decode, out = decoder(d_bytes, d_offs[:-1], d_offs[1:], n, n * 512)

    t = {k: dev(cols[k]) for k in wire.ATT_COLS}
    ec = _lib.AttestationCols(*[t[k].data_ptr() for k in wire.ATT_COLS])
    ne, ns = int(cols["oblique_first"][-1]), int(cols["aggregate_sig_first"][-1])
    nb = sum(int(cols[k][-1]) for k in ("justified_block_hash_offs", "shard_block_hash_offs", "attester_bitfield_offs",
                                        "oblique_offs"))
    e_out = torch.zeros(int(_lib.lib.dll.pz_wire_attestations_bound(n, nb, ne, ns)) + 16, dtype=torch.uint8,
                        device="cuda")
    e_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    e_scr = torch.empty(int(_lib.lib.dll.pz_wire_attestations_scratch_bytes(n)), dtype=torch.uint8, device="cuda")
    sh = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def encode():
        _lib.lib.call("pz_dev_wire_attestations", ctypes.byref(ec), n, 0, e_out.data_ptr(), e_offs.data_ptr(),
                      e_scr.data_ptr(), sh)

    d_ms, e_ms = timed([decode, encode], reps)
    # algorithmic bytes from shapes: the records and their spans read once, every column written once
    col_bytes = sum(int(cols[k].nbytes) for k in wire.ATT_COLS)
    d_alg = n * 512 + 2 * n * 8 + col_bytes + n * (8 + 1 + 4)  # + n_oblique, last_byte, status
    e_alg = col_bytes + n * 512 + (n + 1) * 8
    report("decode (pz_dev_unwire_att.)", d_ms, n, "records", d_alg)
    report("encode (pz_dev_wire_att.)", e_ms, n, "records", e_alg)
    print("decode / encode: %.2fx" % (np.median(d_ms) / np.median(e_ms)), flush=True)
    totals = out["totals"].cpu().numpy()
    got = wire._att_trim({k: out[k] for k in wire.ATT_COLS}, n, totals)
    ok = totals[6] == 0 and all(np.array_equal(got[k].cpu().numpy().view(cols[k].dtype), cols[k])
                                for k in wire.ATT_COLS)
    ok = ok and bool(np.array_equal(e_out[:n * 512].cpu().numpy(), recs.reshape(-1)))
    print("parity=%s" % ok, flush=True)
    return ok


def blocks(reps):
    from prysm_amd.blockchain import serialize_blocks
    t0 = time.perf_counter()
    data, offs = serialize_blocks(synth.chain_blocks(65536, 10000, seed=6))
    data = np.array(data)
    n = len(offs) - 1
    print("configs[4] chain: %d blocks, %.1f MB (built in %.1f s)" % (n, offs[-1] / 1e6, time.perf_counter() - t0),
          flush=True)
    d_bytes, d_offs = torch.from_numpy(data).cuda(), dev(offs)
    blk = wire.unwire_blocks_device(d_bytes, d_offs, n)
    natt = int(blk["natt"].item())
    bc = _lib.BlockColsOut(*[blk[k].data_ptr() for k in wire.BLOCK_COLS])
    cap = blk["att_beg"].numel()
    scr = torch.empty(int(_lib.lib.dll.pz_unwire_blocks_scratch_bytes(n)), dtype=torch.uint8, device="cuda")
    sh = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def split():
        _lib.lib.call("pz_dev_unwire_blocks", d_bytes.data_ptr(), d_offs.data_ptr(), n, cap, ctypes.byref(bc),
                      blk["natt"].data_ptr(), scr.data_ptr(), sh)

    decode, out = decoder(d_bytes, blk["att_beg"], blk["att_end"], natt)

    def both():
        split()
        decode()

    s_ms, d_ms, b_ms = timed([split, decode, both], reps)
    nbytes = int(offs[-1])
    report("split (pz_dev_unwire_blocks)", s_ms, n, "blocks", 0)
    report("decode (%d attestations)" % natt, d_ms, natt, "records", 0)
    report("split + decode", b_ms, n, "blocks", nbytes)
    bad = int(blk["status"].count_nonzero().item()) + int(out["status"][:natt].count_nonzero().item())
    print("attestations %d, bad blocks + records %d" % (natt, bad), flush=True)
    # the same bytes from host memory: one H2D, then the two decodes (host clock, synchronised)
    best = 1e9
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d_bytes.copy_(torch.from_numpy(data), non_blocking=False)
        both()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    print("H2D + split + decode: %.3f ms (best of 10, host clock, pageable source)" % (best * 1e3), flush=True)
    fn = getattr(_lib.lib.dll, "pz_debug_parse", None) if os.environ.get("PZ_PROBE_LIB") else None
    if fn is None:
        print("host parse: not measured (pz_debug_parse is in the A/B library: set PZ_PROBE_LIB)", flush=True)
    else:
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                       ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
        for th in (1, 16):
            sec, cs = ctypes.c_double(), ctypes.c_uint64()
            rc = fn(data.ctypes.data, offs.ctypes.data, n, th, 20, ctypes.byref(sec), ctypes.byref(cs))
            print("host parse, %2d threads: %.3f ms (best of 20), rc %d" % (th, sec.value * 1e3, rc), flush=True)
    return bad == 0


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
    what = sys.argv[3] if len(sys.argv) > 3 else "all"
    ok = True
    if what in ("records", "all"):
        ok = records(reps, n) and ok
    if what in ("blocks", "all"):
        ok = blocks(reps) and ok
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
