// The block walk, for gfx950: the sequential decisions of blockProcessing over a run of received
// blocks (blockchain/service.go:320-333, core.go:181-183) as scans, and ActiveState.RecentBlockHashes
// resident on the device (pz_recent_hashes; computeNewActiveState, core.go:223-237), so that every
// block of the run is tallied and digested against its own window (getSignedParentHashes,
// core.go:348-360).  The rules are blockwalk_dev.h's; this file is their kernels and entry points
// (DESIGN.md §3).
//
// pz_dev_block_walk is three dependent launches on the caller's stream; no workgroup waits for
// another and the host reads nothing:
//   scan  ONE workgroup of 1,024 lanes, a lane per block, tiles of 1,024 blocks taken in sequence
//         with the carry (BwCarry: pending, max slot, candidates so far) and the stop in registers,
//         identical in every lane.  Per tile: the shared round 1 (blockscan_wave.h: a wave max-scan by
//         __shfl_up and a __ballot for "a block went on before me", the waves' words through LDS,
//         bw_round1), then two ballot words a wave in LDS -- the candidates, and the candidates
//         under bw_transition -- from which every lane takes its rank (bw_rank) and the tile's stop
//         (bw_tile_stop); two barriers a tile.  It copies the ring into the head of the log, writes
//         walk / base, the candidates' hashes behind the ring (two 16-byte loads and stores each),
//         zeroes the log's unused tail and leaves the result record.  The cycle's scan
//         (blockcycle.hip) is the same round with its own ballots, state rule and record.
//   rows  a lane per attestation row: parents_start made absolute, pend_take and vote_status
//         narrowed by the row's block.
//   roll  the ring's other buffer set = the last 129 entries of the log; ncand is read from the
//         result record on the device.  The host then swaps the sets: it need not know ncand.
// pz_dev_recent_hashes_append is one launch of one workgroup: count the taken, then place them.
#include <hip/hip_runtime.h>

#include <cstring>

#include "blockscan_wave.h"
#include "resident.h"

struct pz_recent_hashes : pz::Resident {
  pz::DevBuf hashes[2], lens[2];  // 129 x 32 bytes and 129 lengths a set (the lengths padded to 144)
  int live = 0;
  ~pz_recent_hashes() {
    drain();
    for (int k = 0; k < 2; ++k) hashes[k].release(), lens[k].release();
  }
};

namespace pz {
namespace {

constexpr int kRollThreads = 320;                    // >= 258: a lane per 16-byte piece of the ring
constexpr uint32_t kRingPieces = 2 * (uint32_t)kBwRing;
constexpr size_t kRingBytes = kBwRing * 32, kLenBytes = 144;
constexpr int kRowThreads = 256;

struct RingSet {
  uint8_t* hashes;
  uint8_t* lens;
};

extern "C" __global__ void __launch_bounds__(kBwTile) pz_block_walk_scan_kernel(pz_block_walk_batch g, RingSet ring) {
  __shared__ ScanWords s_r1;
  __shared__ uint64_t s_cb[kBwWaves], s_tb[kBwWaves], s_fin[3];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t n = g.nblocks, lag = g.lag;
  scan_ring_head(g.log, ring.hashes);

  BwCarry c = bw_carry(g.has_candidate, g.candidate_slot);  // the same values in every lane
  uint64_t c_stop = kBwNone;
  bool fin_in_lds = false;
  for (uint64_t t0 = 0; t0 < n; t0 += kBwTile) {
    const uint64_t j = t0 + tid;
    const bool in = j < n;
    if (c_stop != kBwNone) {  // past the stop: left for the caller to submit again
      if (in) g.walk[j] = kBwDeferred, g.base[j] = 0;
      continue;
    }
    const bool go = in && bw_go(g.report[j]);
    const uint64_t slot = in ? g.slot_number[j] : 0;
    // ---- round 1: the largest slot before me, and whether anything is pending before me ----
    const BwRound1 r = scan_round1(s_r1, c, t0, j, go, slot);
    // ---- round 2: the candidates before me, and the stop ----
    const uint64_t cb = __ballot(r.cand), tb = __ballot(r.cand && bw_transition(slot, g.last_state_recalc));
    if (lane == 0) s_cb[w] = cb, s_tb[w] = tb;
    __syncthreads();
    const BwRank k = bw_rank(c, s_cb, tid);
    const uint64_t stop = bw_tile_stop(c, t0, lag, n, s_cb, s_tb);
    const bool deferred = j >= stop;
    if (in) {
      g.walk[j] = bw_walk(go, r.cand, deferred);
      g.base[j] = bw_base(lag, k.rank, deferred);
      if (r.cand && !deferred) scan_put_hash(g.log, k.rank, g.block_hash, j);
    }
    if (in && j == stop) s_fin[0] = k.rank, s_fin[1] = r.pending, s_fin[2] = r.before;  // the state before the stop
    if (stop != kBwNone && stop < t0 + kBwTile) fin_in_lds = true;  // (one past lane 1,023: the carry is that state)
    c_stop = stop;
    bw_advance(c, r, k.tile_cnt);
  }
  __syncthreads();
  const uint64_t ncand = fin_in_lds ? s_fin[0] : c.cnt;
  if (tid == 0) {
    g.result[kBwStop] = c_stop == kBwNone ? n : c_stop;
    g.result[kBwNcand] = ncand;
    g.result[kBwHasCandidate] = fin_in_lds ? s_fin[1] : (uint64_t)c.pending;
    g.result[kBwCandidateSlot] = fin_in_lds ? s_fin[2] : c.max;
  }
  scan_zero_tail(g.log, ncand, n);
}

extern "C" __global__ void __launch_bounds__(kRowThreads) pz_block_walk_rows_kernel(pz_block_walk_batch g) {
  const uint64_t i = (uint64_t)blockIdx.x * kRowThreads + threadIdx.x;
  if (i >= g.natt) return;
  const uint64_t b = g.att_block[i];
  if (b >= g.nblocks) return;  // a row no block of the run names stays as it was
  const BwRow r = bw_row(g.parents_start[i], g.pend_take ? g.pend_take[i] : 0, g.vote_status[i], g.walk[b], g.base[b]);
  g.parents_start[i] = r.parents_start;
  if (g.pend_take) g.pend_take[i] = r.pend_take;
  g.vote_status[i] = r.vote_status;
}

extern "C" __global__ void __launch_bounds__(kRollThreads) pz_block_walk_roll_kernel(const uint8_t* log, const uint64_t* result,
                                                                                     const uint32_t* flags, uint64_t nblocks,
                                                                                     RingSet from, RingSet to) {
  const uint32_t p = threadIdx.x;
  if (p >= kRingPieces) return;
  uint64_t ncand = bw_roll_count(result[kBwNcand], flags ? *flags : 0);
  if (ncand > nblocks) ncand = nblocks;  // (the log holds 129 + nblocks hashes)
  const uint64_t k = p >> 1;
  reinterpret_cast<uint4*>(to.hashes)[p] = reinterpret_cast<const uint4*>(log)[2 * bw_roll_src(k, ncand) + (p & 1)];
  if (!(p & 1)) to.lens[k] = bw_roll_len(from.lens[k], ncand);
}

// computeNewActiveState's append (core.go:230-232) for n hashes of which take (NULL: all) chooses.
extern "C" __global__ void __launch_bounds__(kBwTile) pz_recent_append_kernel(const uint8_t* hashes, const uint8_t* take, uint64_t n,
                                                                                 RingSet from, RingSet to) {
  __shared__ uint64_t s_tot[kBwWaves];
  __shared__ uint32_t s_cnt[kBwWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint64_t mine = 0;  // this wave's taken
  for (uint64_t t0 = 0; t0 < n; t0 += kBwTile) {
    const uint64_t j = t0 + tid;
    mine += (uint64_t)__builtin_popcountll(__ballot(j < n && (!take || take[j])));
  }
  if (lane == 0) s_tot[w] = mine;
  __syncthreads();
  uint64_t total = 0;
  for (int k = 0; k < (int)kBwWaves; ++k) total += s_tot[k];
  if (tid < kRingPieces) {  // what stays of the old ring
    const uint64_t k = tid >> 1;
    if (k >= total) {
      reinterpret_cast<uint4*>(to.hashes)[tid - 2 * total] = reinterpret_cast<const uint4*>(from.hashes)[tid];
      if (!(tid & 1)) to.lens[k - total] = bw_roll_len(from.lens[k], total);
    }
  }
  uint64_t c = 0;
  for (uint64_t t0 = 0; t0 < n; t0 += kBwTile) {
    const uint64_t j = t0 + tid;
    const bool t = j < n && (!take || take[j]);
    const uint64_t tb = __ballot(t);
    if (lane == 0) s_cnt[w] = (uint32_t)__builtin_popcountll(tb);
    __syncthreads();
    uint64_t rank = c + (uint64_t)__builtin_popcountll(tb & ((1ull << lane) - 1));
    for (int k = 0; k < (int)kBwWaves; ++k) {
      if (k < (int)w) rank += s_cnt[k];
      c += s_cnt[k];
    }
    __syncthreads();
    const int64_t dst = bw_append_dst(rank, total);
    if (t && dst >= 0) {
      copy32(to.hashes + 32 * dst, hashes + 32 * j);
      to.lens[dst] = 32;
    }
  }
}

RingSet set_of(pz_recent_hashes* h, int which) {
  return RingSet{static_cast<uint8_t*>(h->hashes[which].ptr), static_cast<uint8_t*>(h->lens[which].ptr)};
}

int check_ring(const pz_recent_hashes* h) { return h ? PZ_OK : fail(PZ_EINVAL, "the recent-hashes handle is null"); }

hipError_t launch_walk(pz_recent_hashes* h, const pz_block_walk_batch& b, hipStream_t s, Events* ev) {
  const RingSet from = set_of(h, h->live);
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_block_walk_scan_kernel, dim3(1), dim3(kBwTile), 0, s, b, from);
  stamp(ev, 1, s);
  if (b.natt) hipLaunchKernelGGL(pz_block_walk_rows_kernel, dim3((uint32_t)((b.natt + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0, s, b);
  stamp(ev, 2, s);
  const hipError_t e = recent_hashes_roll(h, b.log, b.result, b.flags, b.nblocks, s);
  stamp(ev, 3, s);
  return e;
}

hipError_t launch_append(pz_recent_hashes* h, const uint8_t* d_hashes, const uint8_t* d_take, uint64_t n, hipStream_t s) {
  hipLaunchKernelGGL(pz_recent_append_kernel, dim3(1), dim3(kBwTile), 0, s, d_hashes, d_take, n, set_of(h, h->live),
                     set_of(h, h->live ^ 1));
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) h->live ^= 1, h->last = s;
  return e;
}

int check_append(const pz_recent_hashes* h, const uint8_t* hashes, uint64_t n) {
  if (!h) return fail(PZ_EINVAL, "the recent-hashes handle is null");
  if (n >= (1ull << 31)) return fail(PZ_EINVAL, "n %llu: 2^31 hashes or more", (unsigned long long)n);
  if (n && !hashes) return fail(PZ_EINVAL, "recent hashes append: null hashes");
  return n ? PZ_OK : 1;
}

}  // namespace

// What blockcycle.hip takes from the ring (resident.h): the live set to scan from, and the walk's
// own roll launch with its swap.  The caller holds the handle's lock.
Resident* resident_of(pz_recent_hashes* h) { return h; }
const uint8_t* recent_hashes_live(pz_recent_hashes* h) { return set_of(h, h->live).hashes; }
hipError_t recent_hashes_roll(pz_recent_hashes* h, const uint8_t* log, const uint64_t* result, const uint32_t* flags, uint64_t nblocks,
                              hipStream_t s) {
  hipLaunchKernelGGL(pz_block_walk_roll_kernel, dim3(1), dim3(kRollThreads), 0, s, log, result, flags, nblocks, set_of(h, h->live),
                     set_of(h, h->live ^ 1));
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) h->live ^= 1, h->last = s;
  return e;
}

}  // namespace pz

using namespace pz;

extern "C" {

int pz_recent_hashes_new(const uint8_t* hashes, const uint8_t* lens, uint64_t n, int device, pz_recent_hashes** out) {
  if (!out) return fail(PZ_EINVAL, "out is null");
  *out = nullptr;
  if (n != kBwWindow)
    return fail(PZ_EINVAL, "%llu recent hashes: the resident ring holds a chain from genesis, always 128 (types/state.go:45-49)",
                (unsigned long long)n);
  if (!hashes) return fail(PZ_EINVAL, "hashes is null");
  uint8_t hb[kRingBytes] = {}, lb[kLenBytes] = {};
  std::memcpy(hb + 32, hashes, kBwWindow * 32);
  for (uint64_t k = 0; k < kBwWindow; ++k) lb[1 + k] = lens ? (lens[k] > 32 ? 32 : lens[k]) : 32;
  int rc = Resident::open(device);
  if (rc) return rc;
  auto* h = new pz_recent_hashes();
  h->device = device;
  const char* what = "recent hashes init";
  hipError_t e;
  if ((rc = h->hashes[0].fill(kRingBytes, 0, what, hb, kRingBytes)) || (rc = h->lens[0].fill(kLenBytes, 0, what, lb, kLenBytes)) ||
      (rc = h->hashes[1].fill(kRingBytes, 0, what)) || (rc = h->lens[1].fill(kLenBytes, 0, what)) ||
      ((e = hipDeviceSynchronize()) != hipSuccess && (rc = hip_fail(e, what)))) {
    delete h;
    return rc;
  }
  *out = h;
  return PZ_OK;
}

void pz_recent_hashes_free(pz_recent_hashes* h) { delete h; }

int pz_recent_hashes_view(pz_recent_hashes* h, const uint8_t** d_hashes, const uint8_t** d_lens) {
  int rc = check_ring(h);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  const RingSet s = set_of(h, h->live);
  if (d_hashes) *d_hashes = s.hashes + 32;
  if (d_lens) *d_lens = s.lens + 1;
  return PZ_OK;
}

int pz_recent_hashes_read(pz_recent_hashes* h, uint8_t* hashes, uint8_t* lens) {
  int rc = check_ring(h);
  if (rc || (rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  const char* what = "recent hashes read";
  if ((rc = h->wait(what))) return rc;
  const RingSet s = set_of(h, h->live);
  if ((rc = down(hashes, s.hashes, kRingBytes, what))) return rc;
  return down(lens, s.lens, kBwRing, what);
}

int pz_dev_recent_hashes_append(pz_recent_hashes* h, const uint8_t* d_hashes, const uint8_t* d_take, uint64_t n, void* stream) {
  int rc = check_append(h, d_hashes, n);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!aligned16(d_hashes)) return fail(PZ_EINVAL, "recent hashes append: d_hashes must be a 16-B aligned device pointer");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  hipError_t e = launch_append(h, d_hashes, d_take, n, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_recent_append_kernel");
}

int pz_recent_hashes_append(pz_recent_hashes* h, const uint8_t* hashes, const uint8_t* take, uint64_t n) {
  int rc = check_append(h, hashes, n);
  if (rc) return rc < 0 ? rc : PZ_OK;
  HostForm f(h, "recent hashes append");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  const uint8_t* d_hashes = st.up(hashes, n * 32);
  const uint8_t* d_take = take ? st.up(take, n) : nullptr;
  if (st.rc) return st.rc;
  st.check(launch_append(h, d_hashes, d_take, n, st.s), "pz_recent_append_kernel");
  return st.sync();
}

uint64_t pz_block_walk_scratch_bytes(uint64_t nblocks, uint64_t natt) {
  (void)natt;  // (the rows are narrowed in place)
  return (kBwRing + nblocks) * 32;
}

int pz_dev_block_walk(pz_recent_hashes* h, const pz_block_walk_batch* b, void* stream) {
  return enqueue_block_run(check_block_run(h, b, true, "block walk"), h, b, stream, "pz_block_walk kernels", launch_walk);
}

int pz_block_walk(pz_recent_hashes* h, const pz_block_walk_batch* hb) {
  int rc = check_block_run(h, hb, false, "block walk");
  if (rc < 0) return rc;
  if (rc) {  // an empty run: the record says so, the ring stays as it is
    if (hb->result)
      hb->result[kBwStop] = 0, hb->result[kBwNcand] = 0, hb->result[kBwHasCandidate] = hb->has_candidate != 0,
      hb->result[kBwCandidateSlot] = hb->has_candidate ? hb->candidate_slot : 0;
    return PZ_OK;
  }
  const uint64_t n = hb->natt, log_bytes = pz_block_walk_scratch_bytes(hb->nblocks, n);
  HostForm f(h, "block walk");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_block_walk_batch d;
  stage_block_run(st, hb, d, kBwResultWords, log_bytes);
  if (st.rc) return st.rc;
  st.check(launch_walk(h, d, st.s, nullptr), "pz_block_walk kernels");
  unstage_block_run(st, hb, d, kBwResultWords, log_bytes);
  st.down(hb->vote_status, d.vote_status, n);  // (both narrowed in place)
  if (hb->pend_take) st.down(hb->pend_take, d.pend_take, n);
  return st.sync();
}

#ifdef PZ_AB_BUILD
int pz_debug_block_walk_timed(pz_recent_hashes* h, const pz_block_walk_batch* b, void* stream, float ms[3]) {
  return timed_block_run(check_block_run(h, b, true, "block walk"), h, b, stream, ms, "pz_block_walk kernels", launch_walk);
}
#endif

}  // extern "C"
