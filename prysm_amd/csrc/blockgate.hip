// The block gate, for gfx950: which received blocks blockProcessing goes on with, which of their
// attestations reach the vote cache and which the pending pool.
//
// blockchain/service.go:281-306 keeps a block iff its LAST attestation passed processAttestation,
// then service.go:313-318 runs calculateBlockVoteCache (core.go:300-345) over EVERY attestation of
// it, the refused ones included, re-deriving their parents and committee.  The rule is
// blockgate_dev.h's; this file is its kernel and its two entry points.
//
// One wave per block, lanes striding over the block's rows (a block of more than 64 rows loops):
//   pass 1  __ballot / popcount over the rows: any bad record status, the PROCESSED count, a row
//           on which processAttestation itself panicked; with the last row's status that gives
//           the block's report and whether it is open.
//   pass 2  a lane per row writes vote_status and pend_take, and, for a row whose parents and
//           committee are re-derived, completes committee / parents_start in place.
// No LDS, no wait on another wave, no look-back; results leave by plain vector stores; the only
// atomic is the OR of the panic bit into the caller's flag word, one per wave that has one.
// The kernel streams ~30 bytes a row (five 8-byte columns only on the re-derived rows) and walks
// the committee table only for those: at the sizes a received batch has it is a launch floor.
#include <hip/hip_runtime.h>

#include "blockgate_dev.h"
#include "resident.h"

namespace pz {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;

extern "C" __global__ void __launch_bounds__(kThreads) pz_block_gate_kernel(pz_block_gate_batch g) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t b = (uint64_t)blockIdx.x * kWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (b >= g.nblocks) return;  // (wave-uniform, as everything below up to the lanes' rows)
  const uint64_t f0 = g.att_first[b], f1 = g.att_first[b + 1];
  if (!bg_span_ok(f0, f1, g.chk.natt)) {
    if (lane == 0) g.report[b] = kBgRejected;
    return;
  }
  const uint64_t n = f1 - f0;
  // ---- pass 1 ----
  uint64_t nproc = 0, bad = 0, panicked = 0;
  for (uint64_t base = 0; base < n; base += 64) {
    const bool in = base + lane < n;
    const uint64_t i = f0 + base + lane;
    const int32_t st = in ? g.chk.status[i] : -1;
    const int32_t rs = in && g.rec_status ? g.rec_status[i] : PZ_OK;
    bad |= __ballot(rs != PZ_OK);
    nproc += (uint64_t)__builtin_popcountll(__ballot(in && st == PZ_ATT_PROCESSED));
    panicked |= __ballot(in && bg_check_panicked(st));
  }
  const bool accepted = g.block_status[b] == PZ_OK && bad == 0;
  const uint8_t report = bg_report(accepted, n, nproc, n ? g.chk.status[f1 - 1] : -1);
  const bool open = report != kBgRejected;
  bool panic = accepted && panicked != 0;
  // ---- pass 2 ----
  for (uint64_t base = 0; base < n; base += 64) {
    if (base + lane >= n) continue;
    const uint64_t i = f0 + base + lane;
    const BgRow r = bg_row(g.chk, i, open);
    panic = panic || r.panic;
    g.vote_status[i] = r.vote_status;
    if (g.pend_take) g.pend_take[i] = bg_pend_take(g.chk.status[i], open, g.candidate, b) ? 1 : 0;
    if (r.rederived) {
      g.chk.committee[i] = r.committee;
      g.chk.parents_start[i] = r.parents_start;
    }
  }
  const uint64_t any_panic = __ballot(panic);
  if (lane == 0) {
    g.report[b] = report;
    if (any_panic) atomicOr(g.flags, kBgPanic);
  }
}

int check_args(const pz_block_gate_batch* b) {
  if (!b) return fail(PZ_EINVAL, "batch is null");
  if (b->nblocks >= (1ull << 31)) return fail(PZ_EINVAL, "nblocks %llu: 2^31 blocks or more", (unsigned long long)b->nblocks);
  if (b->nblocks == 0) return 1;
  if (!b->att_first || !b->block_status || !b->report || !b->vote_status || !b->flags)
    return fail(PZ_EINVAL, "block gate: null att_first / block_status / report / vote_status / flags");
  if (!b->chk.committee || !b->chk.parents_start)
    return fail(PZ_EINVAL, "block gate: chk.committee and chk.parents_start are completed in place and cannot be null");
  const pz_att_check_batch& c = b->chk;
  if (c.natt && (!c.status || !c.slot || !c.block_slot || !c.n_oblique || !c.shard_id))
    return fail(PZ_EINVAL, "block gate: null chk.status / slot / block_slot / n_oblique / shard_id");
  if (c.narr && (!c.arr_offs || !c.arr_shard || !c.arr_comm)) return fail(PZ_EINVAL, "null committee table");
  return PZ_OK;
}

hipError_t launch(const pz_block_gate_batch& b, hipStream_t s) {
  hipLaunchKernelGGL(pz_block_gate_kernel, dim3((uint32_t)((b.nblocks + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, b);
  return hipGetLastError();
}

}  // namespace
}  // namespace pz

using namespace pz;

extern "C" {

int pz_dev_block_gate(const pz_block_gate_batch* b, void* stream) {
  int rc = check_args(b);
  if (rc) return rc < 0 ? rc : PZ_OK;
  hipError_t e = launch(*b, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_block_gate_kernel");
}

int pz_block_gate(const pz_block_gate_batch* hb) {
  int rc = check_args(hb);
  if (rc) return rc < 0 ? rc : PZ_OK;
  const uint64_t nb = hb->nblocks, n = hb->chk.natt, narr = hb->chk.narr;
  if (narr && (rc = check_csr(hb->chk.arr_offs, narr, "committee table"))) return rc;
  HostForm f;  // (no handle: the current device's context)
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_block_gate_batch d = *hb;
  d.att_first = st.up(hb->att_first, nb + 1);
  d.block_status = st.up(hb->block_status, nb);
  if (hb->rec_status) d.rec_status = st.up(hb->rec_status, n);
  if (hb->candidate) d.candidate = st.up(hb->candidate, nb);
  d.chk.status = st.up(hb->chk.status, n);
  d.chk.slot = st.up(hb->chk.slot, n);
  d.chk.block_slot = st.up(hb->chk.block_slot, n);
  d.chk.n_oblique = st.up(hb->chk.n_oblique, n);
  d.chk.shard_id = st.up(hb->chk.shard_id, n);
  if (narr) {
    const uint64_t ne = hb->chk.arr_offs[narr];
    d.chk.arr_offs = st.up(hb->chk.arr_offs, narr + 1);
    d.chk.arr_shard = st.up(hb->chk.arr_shard, ne);
    d.chk.arr_comm = st.up(hb->chk.arr_comm, ne);
  }
  // what the kernel completes or leaves alone goes up first: a row no block names comes back as it was
  d.chk.committee = st.up(hb->chk.committee, n);
  d.chk.parents_start = st.up(hb->chk.parents_start, n);
  d.vote_status = st.up(hb->vote_status, n);
  if (hb->pend_take) d.pend_take = st.up(hb->pend_take, n);
  d.report = st.up<uint8_t>(nullptr, nb);
  d.flags = st.up(hb->flags, 1);
  if (st.rc) return st.rc;
  st.check(launch(d, st.s), "pz_block_gate_kernel");
  st.down(hb->report, d.report, nb);
  st.down(hb->vote_status, d.vote_status, n);
  if (hb->pend_take) st.down(hb->pend_take, d.pend_take, n);
  st.down(hb->chk.committee, d.chk.committee, n);
  st.down(hb->chk.parents_start, d.chk.parents_start, n);
  st.down(hb->flags, d.flags, 1);
  if ((rc = st.sync())) return rc;
  if (*hb->flags & kBgPanic)
    return fail(PZ_EINDEX, "the reference panics in this batch (processAttestation or calculateBlockVoteCache: "
                           "slice bounds, core.go:353, or committee index, core.go:367)");
  return PZ_OK;
}

}  // extern "C"
