// A run of blocks through a cycle transition, for gfx950: the block walk (blockwalk.hip) for a run
// that holds the transition block itself -- the candidate's and the chain's states side by side
// (blockchain/service.go:320-361, core.go:181-183, core.go:398-497).  The rules are
// blockcycle_dev.h's; this file is their kernels and entry points.
//
// pz_dev_block_cycle is three dependent launches on the caller's stream; no workgroup waits for
// another and the host reads nothing:
//   scan  ONE workgroup of 1,024 lanes, a lane per block, tiles of 1,024 blocks taken in sequence.
//         The walk's carry (BwCarry: pending, max slot, candidates so far) and the run's state (T,
//         L, stop, the lag to carry) in registers, identical in every lane.  Per tile the walk's
//         round 1 (blockscan_wave.h, the same text as the walk's scan compiles), then three ballot
//         words a wave in LDS (candidates, transitions under the chain's value, transitions under
//         the promoted one), from which every lane takes its rank (bw_rank) and the same T and L
//         (bc_tile).  The lanes of T and L leave their rank, slot and carry in LDS for the result
//         record.  It copies the ring into the head of the log, writes walk / base, the candidates'
//         hashes behind the ring and the zeroed tail.
//   rows  a lane per attestation row: parents_start made absolute, the gate's vote_status and
//         pend_take split into the phase before stateRecalc and the phase after it.
//   roll  the walk's own kernel and swap (recent_hashes_roll, blockwalk.hip): nothing rolls when
//         the gate's panic bit is set.
#include <hip/hip_runtime.h>

#include "blockcycle_dev.h"
#include "blockscan_wave.h"
#include "resident.h"

namespace pz {
namespace {

constexpr int kBcRowThreads = 256;

enum { kFinRank = 0, kFinPending, kFinBefore, kFinSlot, kFinTRank, kFinTSlot, kFinWords };

extern "C" __global__ void __launch_bounds__(kBwTile) pz_block_cycle_scan_kernel(pz_block_cycle_batch g, const uint8_t* ring) {
  __shared__ ScanWords s_r1;
  __shared__ uint64_t s_cb[kBwWaves], s_tb[kBwWaves], s_ta[kBwWaves], s_fin[kFinWords];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t n = g.nblocks, lag = g.lag, lsr = g.last_state_recalc, lsr_after = bc_lsr_after(lsr, lag);
  scan_ring_head(g.log, ring);
  if (tid < kFinWords) s_fin[tid] = 0;

  BwCarry c = bw_carry(g.has_candidate, g.candidate_slot);  // the same values in every lane
  BcState st = bc_start(lag);
  for (uint64_t t0 = 0; t0 < n; t0 += kBwTile) {
    const uint64_t j = t0 + tid;
    const bool in = j < n;
    if (st.stop != kBwNone) {  // past the stop: left for the caller to submit again
      if (in) g.walk[j] = kBwDeferred, g.base[j] = 0;
      continue;
    }
    const bool go = in && bw_go(g.report[j]);
    const uint64_t slot = in ? g.slot_number[j] : 0;
    // ---- round 1 (the walk's): the largest slot before me, and whether anything is pending before me ----
    const BwRound1 r = scan_round1(s_r1, c, t0, j, go, slot);
    // ---- round 2: the candidates before me; T, L and the stop from the tile's ballots ----
    const uint64_t cb = __ballot(r.cand), tb = __ballot(r.cand && bw_transition(slot, lsr)),
                   ta = __ballot(r.cand && bw_transition(slot, lsr_after));
    if (lane == 0) s_cb[w] = cb, s_tb[w] = tb, s_ta[w] = ta;
    __syncthreads();
    const BwRank k = bw_rank(c, s_cb, tid);
    bc_tile(st, t0, lag, s_cb, s_tb, s_ta);
    const bool deferred = bc_deferred(st, j);
    if (in) {
      g.walk[j] = bw_walk(go, r.cand, deferred);
      g.base[j] = bc_base(bc_lagged(st, lag, j), k.rank, deferred);
      if (r.cand && !deferred) scan_put_hash(g.log, k.rank, g.block_hash, j);
      if (j == st.t_index) s_fin[kFinTRank] = k.rank, s_fin[kFinTSlot] = slot;
      if (j == st.l_index) s_fin[kFinRank] = k.rank, s_fin[kFinPending] = r.pending, s_fin[kFinBefore] = r.before, s_fin[kFinSlot] = slot;
    }
    bw_advance(c, r, k.tile_cnt);
  }
  __syncthreads();
  // L met: the record is the state after L (included) or before it (deferred); else the carry
  const bool met = st.l_index != kBwNone, included = met && st.stop == st.l_index + 1;
  const uint64_t ncand = met ? s_fin[kFinRank] + (included ? 1 : 0) : c.cnt;
  if (tid == 0) {
    g.result[kBwStop] = st.stop == kBwNone ? n : st.stop;
    g.result[kBwNcand] = ncand;
    g.result[kBwHasCandidate] = included ? 1 : met ? s_fin[kFinPending] : (uint64_t)c.pending;
    g.result[kBwCandidateSlot] = included ? s_fin[kFinSlot] : met ? s_fin[kFinBefore] : c.max;
    g.result[kBcTIndex] = st.t_index;
    g.result[kBcTRank] = s_fin[kFinTRank];
    g.result[kBcTSlot] = s_fin[kFinTSlot];
    g.result[kBcLagOut] = st.lag_out;
  }
  scan_zero_tail(g.log, ncand, n);
}

extern "C" __global__ void __launch_bounds__(kBcRowThreads) pz_block_cycle_rows_kernel(pz_block_cycle_batch g) {
  const uint64_t i = (uint64_t)blockIdx.x * kBcRowThreads + threadIdx.x;
  if (i >= g.natt) return;
  const uint64_t b = g.att_block[i];
  const bool named = b < g.nblocks;  // a row no block of the run names keeps its parents_start and lands nowhere
  const BcRow r = bc_row(g.parents_start[i], g.pend_take ? g.pend_take[i] : 1, g.vote_status[i], named ? g.walk[b] : kBwDeferred,
                         named ? g.base[b] : 0, b, g.result[kBcTIndex]);
  g.parents_start[i] = r.parents_start;
  g.vote0[i] = r.vote0, g.vote1[i] = r.vote1;
  g.take0[i] = r.take0, g.take1[i] = r.take1;
}

// The shared checks, and the four columns that are the cycle's own.  1: nothing to launch.
int check_cycle(const pz_recent_hashes* h, const pz_block_cycle_batch* b, bool device_form) {
  const int rc = check_block_run(h, b, device_form, "block cycle");
  if (!rc && b->natt && (!b->vote0 || !b->vote1 || !b->take0 || !b->take1))
    return fail(PZ_EINVAL, "block cycle: null vote0 / vote1 / take0 / take1");
  return rc;
}

hipError_t launch_cycle(pz_recent_hashes* h, const pz_block_cycle_batch& b, hipStream_t s, Events* ev) {
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_block_cycle_scan_kernel, dim3(1), dim3(kBwTile), 0, s, b, recent_hashes_live(h));
  stamp(ev, 1, s);
  if (b.natt)
    hipLaunchKernelGGL(pz_block_cycle_rows_kernel, dim3((uint32_t)((b.natt + kBcRowThreads - 1) / kBcRowThreads)), dim3(kBcRowThreads), 0, s, b);
  stamp(ev, 2, s);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = recent_hashes_roll(h, b.log, b.result, b.flags, b.nblocks, s);
  stamp(ev, 3, s);
  return e;
}

}  // namespace
}  // namespace pz

using namespace pz;

extern "C" {

uint64_t pz_block_cycle_scratch_bytes(uint64_t nblocks, uint64_t natt) {
  (void)natt;  // (the rows' outputs are the caller's columns)
  return (kBwRing + nblocks) * 32;
}

int pz_dev_block_cycle(pz_recent_hashes* h, const pz_block_cycle_batch* b, void* stream) {
  return enqueue_block_run(check_cycle(h, b, true), h, b, stream, "pz_block_cycle kernels", launch_cycle);
}

int pz_block_cycle(pz_recent_hashes* h, const pz_block_cycle_batch* hb) {
  int rc = check_cycle(h, hb, false);
  if (rc < 0) return rc;
  if (rc) {  // an empty run: the record says so, the ring stays as it is
    if (hb->result) {
      uint64_t* r = hb->result;
      r[kBwStop] = 0, r[kBwNcand] = 0, r[kBwHasCandidate] = hb->has_candidate != 0;
      r[kBwCandidateSlot] = hb->has_candidate ? hb->candidate_slot : 0;
      r[kBcTIndex] = kBwNone, r[kBcTRank] = 0, r[kBcTSlot] = 0, r[kBcLagOut] = hb->lag;
    }
    return PZ_OK;
  }
  const uint64_t n = hb->natt, log_bytes = pz_block_cycle_scratch_bytes(hb->nblocks, n);
  HostForm f(resident_of(h), "block cycle");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_block_cycle_batch d;
  stage_block_run(st, hb, d, kBcResultWords, log_bytes);
  if (n) {
    d.vote0 = st.up<int32_t>(nullptr, n), d.vote1 = st.up<int32_t>(nullptr, n);
    d.take0 = st.up<uint8_t>(nullptr, n), d.take1 = st.up<uint8_t>(nullptr, n);
  }
  if (st.rc) return st.rc;
  st.check(launch_cycle(h, d, st.s, nullptr), "pz_block_cycle kernels");
  unstage_block_run(st, hb, d, kBcResultWords, log_bytes);
  st.down(hb->vote0, d.vote0, n), st.down(hb->vote1, d.vote1, n);
  st.down(hb->take0, d.take0, n), st.down(hb->take1, d.take1, n);
  return st.sync();
}

#ifdef PZ_AB_BUILD
int pz_debug_block_cycle_timed(pz_recent_hashes* h, const pz_block_cycle_batch* b, void* stream, float ms[3]) {
  return timed_block_run(check_cycle(h, b, true), h, b, stream, ms, "pz_block_cycle kernels", launch_cycle);
}
#endif

}  // extern "C"
