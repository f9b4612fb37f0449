// A run of blocks through a cycle transition, for gfx950: the block walk (blockwalk.hip) for a run
// that holds the transition block itself -- the candidate's and the chain's states side by side
// (blockchain/service.go:320-361, core.go:181-183, core.go:398-497).  The rules are
// blockcycle_dev.h's; this file is their kernels and entry points.
//
// pz_dev_block_cycle is three dependent launches on the caller's stream; no workgroup waits for
// another and the host reads nothing:
//   scan  ONE workgroup of 1,024 lanes, a lane per block, tiles of 1,024 blocks taken in sequence.
//         The walk's carry (pending, max slot, candidates so far) and the run's state (T, L, stop,
//         the lag to carry) in registers, identical in every lane.  Per tile the walk's two rounds;
//         the second leaves three ballot words a wave in LDS (candidates, transitions under the
//         chain's value, transitions under the promoted one), from which every lane takes the same
//         T and L (bc_tile).  The lanes of T and L leave their rank, slot and carry in LDS for the
//         result record.  It copies the ring into the head of the log, writes walk / base, the
//         candidates' hashes behind the ring and the zeroed tail.
//   rows  a lane per attestation row: parents_start made absolute, the gate's vote_status and
//         pend_take split into the phase before stateRecalc and the phase after it.
//   roll  the walk's own kernel and swap (recent_hashes_roll, blockwalk.hip): nothing rolls when
//         the gate's panic bit is set.
#include <hip/hip_runtime.h>

#include "blockcycle_dev.h"
#include "resident.h"

namespace pz {
namespace {

constexpr int kBcThreads = (int)kBcTile;
constexpr int kBcRowThreads = 256;
constexpr uint32_t kBcRingPieces = 2 * (uint32_t)kBwRing;  // the ring in 16-byte pieces

__device__ __forceinline__ void bc_copy32(uint8_t* dst, const uint8_t* src) {  // both 16-byte aligned
  const uint4 a = reinterpret_cast<const uint4*>(src)[0], b = reinterpret_cast<const uint4*>(src)[1];
  reinterpret_cast<uint4*>(dst)[0] = a;
  reinterpret_cast<uint4*>(dst)[1] = b;
}

// Inclusive max-scan over the wave.
__device__ __forceinline__ uint64_t bc_wmaxscan(uint64_t x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t y = __shfl_up(x, d, 64);
    if (lane >= d && y > x) x = y;
  }
  return x;
}

enum { kFinRank = 0, kFinPending, kFinBefore, kFinSlot, kFinTRank, kFinTSlot, kFinWords };

extern "C" __global__ void __launch_bounds__(kBcThreads) pz_block_cycle_scan_kernel(pz_block_cycle_batch g, const uint8_t* ring) {
  __shared__ uint64_t s_max[kBcWaves], s_fslot[kBcWaves], s_cb[kBcWaves], s_tb[kBcWaves], s_ta[kBcWaves], s_fin[kFinWords];
  __shared__ uint32_t s_fgo[kBcWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t n = g.nblocks, lag = g.lag, lsr = g.last_state_recalc, lsr_after = bc_lsr_after(lsr, lag);
  if (tid < kBcRingPieces) reinterpret_cast<uint4*>(g.log)[tid] = reinterpret_cast<const uint4*>(ring)[tid];
  if (tid < kFinWords) s_fin[tid] = 0;

  // the carry: the same values in every lane
  bool c_pending = g.has_candidate != 0;
  uint64_t c_max = c_pending ? g.candidate_slot : 0, c_cnt = 0;
  BcState st = bc_start(lag);
  for (uint64_t t0 = 0; t0 < n; t0 += kBcThreads) {
    const uint64_t j = t0 + tid;
    const bool in = j < n;
    if (st.stop != kBwNone) {  // past the stop: left for the caller to submit again
      if (in) g.walk[j] = kBwDeferred, g.base[j] = 0;
      continue;
    }
    const bool go = in && bw_go(g.report[j]);
    const uint64_t slot = in ? g.slot_number[j] : 0;
    // ---- round 1 (the walk's): the largest slot before me, and whether anything is pending before me ----
    const uint64_t inc = bc_wmaxscan(bw_scan_value(go, true, slot));
    uint64_t before = __shfl_up(inc, 1, 64);
    if (lane == 0) before = 0;
    const uint64_t gob = __ballot(go);
    const uint32_t fl = gob ? (uint32_t)__builtin_ctzll(gob) : 64;
    const uint64_t fs = __shfl(slot, (int)(fl & 63), 64);
    if (lane == 63) s_max[w] = inc;
    if (lane == 0) s_fgo[w] = fl, s_fslot[w] = fs;
    __syncthreads();
    uint64_t tile_max = c_max, first = kBwNone, fslot = 0;
    if (c_max > before) before = c_max;
    for (int k = 0; k < (int)kBcWaves; ++k) {
      const uint64_t m = s_max[k];
      if (k < (int)w && m > before) before = m;
      if (m > tile_max) tile_max = m;
      if (!c_pending && first == kBwNone && s_fgo[k] < 64) first = t0 + 64 * k + s_fgo[k], fslot = s_fslot[k];
    }
    // with nothing carried in, the first block that goes on is the candidate whatever its slot
    const bool pending = c_pending || first < j;  // (kBwNone < j never holds)
    if (first < j && fslot > before) before = fslot;
    if (first != kBwNone && bw_scan_value(true, false, fslot) > tile_max) tile_max = fslot;
    const bool cand = bw_candidate(go, pending, slot, before);
    // ---- round 2: the candidates before me; T, L and the stop from the tile's ballots ----
    const uint64_t cb = __ballot(cand), tb = __ballot(cand && bw_transition(slot, lsr)), ta = __ballot(cand && bw_transition(slot, lsr_after));
    if (lane == 0) s_cb[w] = cb, s_tb[w] = tb, s_ta[w] = ta;
    __syncthreads();
    uint64_t rank = c_cnt + (uint64_t)__builtin_popcountll(cb & ((1ull << lane) - 1));
    uint64_t tile_cnt = 0;
    for (int k = 0; k < (int)kBcWaves; ++k) {
      const uint64_t c = (uint64_t)__builtin_popcountll(s_cb[k]);
      if (k < (int)w) rank += c;
      tile_cnt += c;
    }
    bc_tile(st, t0, lag, s_cb, s_tb, s_ta);
    const bool deferred = bc_deferred(st, j);
    if (in) {
      g.walk[j] = bw_walk(go, cand, deferred);
      g.base[j] = bc_base(bc_lagged(st, lag, j), rank, deferred);
      if (cand && !deferred) bc_copy32(g.log + 32 * (kBwRing + rank), g.block_hash + 32 * j);
      if (j == st.t_index) s_fin[kFinTRank] = rank, s_fin[kFinTSlot] = slot;
      if (j == st.l_index) s_fin[kFinRank] = rank, s_fin[kFinPending] = pending, s_fin[kFinBefore] = before, s_fin[kFinSlot] = slot;
    }
    c_cnt += tile_cnt, c_max = tile_max, c_pending = c_pending || first != kBwNone;
  }
  __syncthreads();
  // L met: the record is the state after L (included) or before it (deferred); else the carry
  const bool met = st.l_index != kBwNone, included = met && st.stop == st.l_index + 1;
  const uint64_t ncand = met ? s_fin[kFinRank] + (included ? 1 : 0) : c_cnt;
  if (tid == 0) {
    g.result[kBwStop] = st.stop == kBwNone ? n : st.stop;
    g.result[kBwNcand] = ncand;
    g.result[kBwHasCandidate] = included ? 1 : met ? s_fin[kFinPending] : (uint64_t)c_pending;
    g.result[kBwCandidateSlot] = included ? s_fin[kFinSlot] : met ? s_fin[kFinBefore] : c_max;
    g.result[kBcTIndex] = st.t_index;
    g.result[kBcTRank] = s_fin[kFinTRank];
    g.result[kBcTSlot] = s_fin[kFinTSlot];
    g.result[kBcLagOut] = st.lag_out;
  }
  uint4* log16 = reinterpret_cast<uint4*>(g.log);
  for (uint64_t p = 2 * (kBwRing + ncand) + tid; p < 2 * (kBwRing + n); p += kBcThreads) log16[p] = make_uint4(0, 0, 0, 0);
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

// 1: nothing to launch.
int check_cycle(const pz_recent_hashes* h, const pz_block_cycle_batch* b, bool device_form) {
  if (!h || !b) return fail(PZ_EINVAL, "block cycle: null handle or batch");
  if (b->nblocks >= (1ull << 31)) return fail(PZ_EINVAL, "nblocks %llu: 2^31 blocks or more", (unsigned long long)b->nblocks);
  if (b->lag > 1) return fail(PZ_EINVAL, "lag %llu: 0 or 1", (unsigned long long)b->lag);
  if (b->nblocks == 0) return 1;
  if (!b->slot_number || !b->report || !b->block_hash || !b->walk || !b->base || !b->result)
    return fail(PZ_EINVAL, "block cycle: null slot_number / report / block_hash / walk / base / result");
  if (device_form && !b->log) return fail(PZ_EINVAL, "block cycle: null log");
  if (b->natt && (!b->att_block || !b->vote_status || !b->parents_start || !b->vote0 || !b->vote1 || !b->take0 || !b->take1))
    return fail(PZ_EINVAL, "block cycle: null att_block / vote_status / parents_start / vote0 / vote1 / take0 / take1");
  return PZ_OK;
}

hipError_t launch_cycle(pz_recent_hashes* h, const pz_block_cycle_batch& b, hipStream_t s, Events* ev = nullptr) {
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_block_cycle_scan_kernel, dim3(1), dim3(kBcThreads), 0, s, b, recent_hashes_live(h));
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
  int rc = check_cycle(h, b, true);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!aligned16(b->block_hash) || !aligned16(b->log))
    return fail(PZ_EINVAL, "block cycle: block_hash and log must be 16-B aligned device pointers");
  Resident* r = resident_of(h);
  if ((rc = r->use())) return rc;
  std::lock_guard<std::mutex> lk(r->mu);
  hipError_t e = launch_cycle(h, *b, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_block_cycle kernels");
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
  const uint64_t nb = hb->nblocks, n = hb->natt;
  HostForm f(resident_of(h), "block cycle");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_block_cycle_batch d = *hb;
  d.slot_number = st.up(hb->slot_number, nb);
  d.report = st.up(hb->report, nb);
  d.block_hash = st.up(hb->block_hash, nb * 32);
  if (n) {
    d.att_block = st.up(hb->att_block, n);
    d.vote_status = st.up(hb->vote_status, n);
    d.parents_start = st.up(hb->parents_start, n);
    if (hb->pend_take) d.pend_take = st.up(hb->pend_take, n);
    d.vote0 = st.up<int32_t>(nullptr, n), d.vote1 = st.up<int32_t>(nullptr, n);
    d.take0 = st.up<uint8_t>(nullptr, n), d.take1 = st.up<uint8_t>(nullptr, n);
  }
  d.walk = st.up<uint8_t>(nullptr, nb);
  d.base = st.up<uint64_t>(nullptr, nb);
  d.result = st.up<uint64_t>(nullptr, kBcResultWords);
  d.log = st.up<uint8_t>(nullptr, (kBwRing + nb) * 32);
  if (hb->flags) d.flags = st.up(hb->flags, 1);
  if (st.rc) return st.rc;
  st.check(launch_cycle(h, d, st.s), "pz_block_cycle kernels");
  st.down(hb->walk, d.walk, nb);
  st.down(hb->base, d.base, nb);
  st.down(hb->result, d.result, kBcResultWords);
  if (hb->log) st.down(hb->log, d.log, (kBwRing + nb) * 32);
  if (n) {
    st.down(hb->parents_start, d.parents_start, n);
    st.down(hb->vote0, d.vote0, n), st.down(hb->vote1, d.vote1, n);
    st.down(hb->take0, d.take0, n), st.down(hb->take1, d.take1, n);
  }
  return st.sync();
}

#ifdef PZ_AB_BUILD
// (tools/blockcycle_probe.py) pz_dev_block_cycle with one event pair on each of its three launches;
// synchronises and returns the milliseconds of scan, rows and roll in ms[0..3).
int pz_debug_block_cycle_timed(pz_recent_hashes* h, const pz_block_cycle_batch* b, void* stream, float ms[3]) {
  int rc = check_cycle(h, b, true);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!ms || !aligned16(b->block_hash) || !aligned16(b->log)) return fail(PZ_EINVAL, "null ms or misaligned pointers");
  Resident* r = resident_of(h);
  if ((rc = r->use())) return rc;
  std::lock_guard<std::mutex> lk(r->mu);
  Events ev;
  if ((rc = ev.create(4))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = launch_cycle(h, *b, s, &ev);
  return ev.elapsed(e == hipSuccess ? PZ_OK : hip_fail(e, "pz_block_cycle kernels"), ms, nullptr, 3, s, "timed block cycle");
}
#endif

}  // extern "C"
