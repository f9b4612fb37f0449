// stateRecalc (blockchain/core.go:398-497) as one call over the resident objects, for gfx950.
//
// pz_recalc_state holds the CrystallizedState's side of the transition on one device: eight u64
// scalars (PZ_RS_*), the crosslink records as columns (dynasty, slot, hash at a fixed stride, hash
// length), the last call's winners and a sticky error word.  pz_dev_state_recalc advances it from
// the pending-attestation pool (attpool.hip) and the block vote cache (votecache.hip) where they
// lie; the validators and the committee CSR stay the caller's device arrays.
//
// One call, on the caller's stream.  No workgroup ever waits for another (no spin, no look-back,
// no polling): every cross-launch fact travels through a launch boundary.
//   1 fit      a lane per pending row (the grid from a host upper bound, the count read on the
//              device, as the prune): raises a flag if a ShardBlockHash is longer than the records'
//              stride; the first lanes copy the pool's seven counts and lastStateRecalc beside it.
//              The host then makes its one wait, for those words: natt and max_inst_bytes of
//              pz_epoch_batch and the prune's bound are host values.  Flag set: PZ_ERANGE, nothing
//              changed.
//   2 justify  one wave, lane i = RecentBlockHashes()[i]: vc_probe (votecache_dev.h), the slot's
//              total, 3 * total >= 2 * TotalDeposits; the ballot is the mask rs_justify
//              (recalc_dev.h, core.go:411-431) runs over on lane 0.  Results and a snapshot of
//              lastStateRecalc, CurrentDynasty and TotalDeposits go to scratch.
//   3 epoch    pz_dev_epoch_count then pz_dev_epoch_finish, one instance over the pool's view;
//              dynasty, total_deposit and rec_dynasty point into the handle.
//   4 commit   a lane per record: the panic decision (rs_panics) from scal; else the records with
//              a winner get {CurrentDynasty, block_slot, the winning row's ShardBlockHash}
//              (core.go:549-555, 16 bytes a store), the winners are kept, and lane 0 writes the
//              new scalars (core.go:467-478).  It reads the snapshot, never a scalar another lane
//              of this launch writes.
//   5 prune    pz_dev_att_pool_prune(lastStateRecalc) (core.go:444-450).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "recalc_dev.h"
#include "resident.h"

struct pz_recalc_state : pz::Resident {  // (last: read waits for it)
  uint32_t nrec = 0, stride = 0;
  pz::DevBuf words;            // scalars[PZ_RS_COUNT], then the sticky error word
  pz::DevBuf rec_dynasty, rec_slot, rec_hash, rec_hash_len, winner;  // max(nrec, 1) entries each
  ~pz_recalc_state() {
    drain();
    for (pz::DevBuf* b : {&words, &rec_dynasty, &rec_slot, &rec_hash, &rec_hash_len, &winner}) b->release();
  }
};

namespace pz {
namespace {

constexpr int kRsThreads = 256;

// scratch, in u64 words: the fit record, the justify record, then the epoch's outputs
enum { kFitFlag = 0, kFitCounts = 1, kFitLsr = 8, kFitWords = 10 };
enum { kJStreak = 0, kJJustified = 1, kJFinalized = 2, kJDynasty = 3, kJLsr = 4, kJDeposits = 5, kJMask = 6, kJWords = 8 };

struct RsLayout {
  uint64_t fit, just, scal, vote, total, act_mask, act_list, blk_cnt, winner, end;  // byte offsets
};

RsLayout layout(uint64_t nval, uint64_t rows_cap, uint32_t nrec) {
  RsLayout l;
  const uint64_t na = std::max<uint64_t>(rows_cap, 1);
  l.fit = 0;
  l.just = l.fit + 8 * kFitWords;
  l.scal = l.just + 8 * kJWords;
  l.vote = l.scal + 8 * PZ_SCAL_COUNT;
  l.total = l.vote + r16(8 * na);
  l.act_mask = l.total + r16(8 * na);
  l.act_list = l.act_mask + r16(8 * ((nval + 63) / 64));
  l.blk_cnt = l.act_list + r16(4 * std::max<uint64_t>(nval, 1));
  l.winner = l.blk_cnt + r16(4 * ((nval + 2047) / 2048 + 1));
  l.end = l.winner + r16(4 * std::max<uint32_t>(nrec, 1));
  return l;
}

struct RsArgs {
  // the handle
  uint64_t* scalars;  // [PZ_RS_COUNT], the error word at [PZ_RS_COUNT]
  uint64_t* rec_dynasty;
  uint64_t* rec_slot;
  uint8_t* rec_hash;
  uint32_t* rec_hash_len;
  uint32_t* winner_kept;
  uint32_t nrec, stride;
  // the pool
  const uint64_t* pool_counts;
  const uint8_t* sbh;
  const uint64_t* sbh_offs;
  uint64_t rows_ub;
  // the cache (table NULL: no entry)
  const uint32_t* table;
  const uint8_t* keys;
  const uint32_t* nslots;
  const uint64_t* totals;
  uint32_t slot_cap, cells;
  // the call
  const uint8_t* recent;
  uint64_t block_slot;
  // scratch
  uint64_t* fit;
  uint64_t* just;
  const uint64_t* scal;
  const uint32_t* winner;
};

// ---- 1: fit ------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kRsThreads) pz_rs_fit_kernel(RsArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kRsThreads + threadIdx.x;
  const uint64_t rows = a.pool_counts[0];
  if (i < 7) a.fit[kFitCounts + i] = a.pool_counts[i];
  if (i == 7) a.fit[kFitLsr] = a.scalars[PZ_RS_LAST_STATE_RECALC];
  if (i < rows && !rs_row_fits(a.sbh_offs[i], a.sbh_offs[i + 1], a.stride))
    atomicOr((unsigned long long*)(a.fit + kFitFlag), 1ull);
}

// ---- 2: justify (one wave) ----------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64) pz_rs_justify_kernel(RsArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint64_t deposits = a.scalars[PZ_RS_TOTAL_DEPOSITS];
  uint64_t total = 0;
  if (a.table) {
    const uint32_t ns = *a.nslots < a.slot_cap ? *a.nslots : a.slot_cap;
    const uint32_t slot = vc_probe(a.table, a.cells, a.keys, ns, vc_load_hash16(a.recent + 32 * lane));
    if (slot != kVcNone) total = a.totals[slot];
  }
  const uint64_t mask = __ballot(rs_slot_passes(total, deposits));
  if (lane != 0) return;
  const uint64_t lsr = a.scalars[PZ_RS_LAST_STATE_RECALC];
  const RsJustified j = rs_justify(mask, lsr,
                                   RsJustified{a.scalars[PZ_RS_JUSTIFIED_STREAK], a.scalars[PZ_RS_LAST_JUSTIFIED_SLOT],
                                               a.scalars[PZ_RS_LAST_FINALIZED_SLOT]});
  a.just[kJStreak] = j.streak;
  a.just[kJJustified] = j.justified;
  a.just[kJFinalized] = j.finalized;
  a.just[kJDynasty] = a.scalars[PZ_RS_CURRENT_DYNASTY];
  a.just[kJLsr] = lsr;
  a.just[kJDeposits] = deposits;
  a.just[kJMask] = mask;
}

// ---- 4: commit -----------------------------------------------------------------------------------
// The 16 bytes of piece k of a hash of len bytes at src (any alignment): bytes past len are zero,
// and nothing at or past src + len is read.
__device__ __forceinline__ uint4 hash_piece(const uint8_t* src, uint32_t len, uint32_t k) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (k + 16 <= len) {
    __builtin_memcpy(&v, src + k, 16);
  } else if (k < len) {
    uint64_t lo = 0, hi = 0;  // (two words, not an indexed array: no private memory)
    for (uint32_t j = 0; j < len - k; ++j) {
      const uint64_t byte = src[k + j];
      if (j < 8) lo |= byte << (8 * j);
      else hi |= byte << (8 * (j - 8));
    }
    v = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
  }
  return v;
}

extern "C" __global__ void __launch_bounds__(kRsThreads) pz_rs_commit_kernel(RsArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kRsThreads + threadIdx.x;
  uint64_t scal[PZ_SCAL_COUNT];
#pragma unroll
  for (int k = 0; k < PZ_SCAL_COUNT; ++k) scal[k] = a.scal[k];
  if (rs_panics(scal, a.just[kJDeposits])) {  // (grid-uniform)
    if (s == 0) atomicOr((unsigned long long*)(a.scalars + PZ_RS_COUNT), (unsigned long long)kRsErrPanic);
    return;
  }
  if (s < a.nrec) {
    const uint32_t row = a.winner[s];
    a.winner_kept[s] = row;
    if (rs_row_ok(row, a.pool_counts[0])) {
      const uint64_t lo = a.sbh_offs[row], hi = a.sbh_offs[row + 1];
      const uint32_t len = rs_hash_len(lo, hi, a.stride);
      a.rec_dynasty[s] = a.just[kJDynasty];
      a.rec_slot[s] = a.block_slot;
      a.rec_hash_len[s] = len;
      uint4* out = reinterpret_cast<uint4*>(a.rec_hash + s * a.stride);
      for (uint32_t k = 0; k < a.stride; k += 16) out[k >> 4] = hash_piece(a.sbh + lo, len, k);
    }
  }
  if (s == 0) {
    a.scalars[PZ_RS_LAST_STATE_RECALC] = a.just[kJLsr] + PZ_CYCLE_LENGTH;
    a.scalars[PZ_RS_JUSTIFIED_STREAK] = a.just[kJStreak];
    a.scalars[PZ_RS_LAST_JUSTIFIED_SLOT] = a.just[kJJustified];
    a.scalars[PZ_RS_LAST_FINALIZED_SLOT] = a.just[kJFinalized];
    a.scalars[PZ_RS_TOTAL_DEPOSITS] = scal[PZ_SCAL_NEXT_BAL];
    a.scalars[PZ_RS_CURRENT_DYNASTY] = 0;  // (the reference's new state leaves it unset)
  }
}

// ---- host side ---------------------------------------------------------------------------------
// The whole call on s.  ev (the A/B library's timed entry; null in the product): eight events,
// around the fit, justify, count, finish, commit and prune steps (ev[1] .. ev[2] is the host's wait).
int enqueue(pz_recalc_state* h, pz_att_pool* pool, pz_vote_cache* cache, const pz_recalc_batch& b, void* d_scratch,
            hipStream_t s, Events* ev = nullptr) {
  ApView pv;
  VcView cv;
  std::memset(&cv, 0, sizeof cv);
  int rc = att_pool_peek(pool, &pv, s);
  if (rc) return rc;
  if (cache && (rc = vote_cache_view(cache, &cv, s))) return rc;
  if (pv.device != h->device || (cache && cv.device != h->device))
    return fail(PZ_EINVAL, "the recalc state, the pool and the vote cache live on different devices");
  if (cache && cv.nval != b.nval)
    return fail(PZ_EINVAL, "nval %llu, the vote cache's %llu", (unsigned long long)b.nval, (unsigned long long)cv.nval);
  if (b.nval >= (1ull << 32)) return fail(PZ_EINVAL, "2^32 validators or more");

  const RsLayout l = layout(b.nval, pv.rows_cap, h->nrec);
  uint8_t* p = static_cast<uint8_t*>(d_scratch);
  RsArgs a;
  std::memset(&a, 0, sizeof a);
  a.scalars = static_cast<uint64_t*>(h->words.ptr);
  a.rec_dynasty = static_cast<uint64_t*>(h->rec_dynasty.ptr);
  a.rec_slot = static_cast<uint64_t*>(h->rec_slot.ptr);
  a.rec_hash = static_cast<uint8_t*>(h->rec_hash.ptr);
  a.rec_hash_len = static_cast<uint32_t*>(h->rec_hash_len.ptr);
  a.winner_kept = static_cast<uint32_t*>(h->winner.ptr);
  a.nrec = h->nrec, a.stride = h->stride;
  a.pool_counts = pv.counts;
  a.sbh = pv.cols.shard_block_hash, a.sbh_offs = pv.cols.shard_block_hash_offs;
  a.rows_ub = pv.rows_ub;
  if (cache) {
    a.table = cv.table, a.keys = cv.keys, a.nslots = cv.nslots, a.totals = cv.totals;
    a.slot_cap = cv.slot_cap, a.cells = cv.cells;
  }
  a.recent = b.recent;
  a.block_slot = b.block_slot;
  a.fit = reinterpret_cast<uint64_t*>(p + l.fit);
  a.just = reinterpret_cast<uint64_t*>(p + l.just);
  a.scal = reinterpret_cast<uint64_t*>(p + l.scal);
  a.winner = reinterpret_cast<uint32_t*>(p + l.winner);

  hipError_t e = hipMemsetAsync(p, 0, l.winner, s);
  if (e == hipSuccess) e = hipMemsetAsync(p + l.winner, 0xFF, l.end - l.winner, s);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
  h->last = s;

  // 1: fit, and the call's one wait
  stamp(ev, 0, s);
  const uint64_t rows_ub = std::min(pv.rows_ub, pv.rows_cap);
  hipLaunchKernelGGL(pz_rs_fit_kernel, dim3((uint32_t)std::max<uint64_t>((rows_ub + kRsThreads - 1) / kRsThreads, 1)),
                     dim3(kRsThreads), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_rs_fit_kernel");
  stamp(ev, 1, s);
  uint64_t fit[kFitWords];
  if ((e = hipMemcpyAsync(fit, a.fit, sizeof fit, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = hipStreamSynchronize(s)) != hipSuccess)
    return hip_fail(e, "recalc fit check");
  const uint64_t rows = fit[kFitCounts];
  if (rows > pv.rows_cap || rows >= (1ull << 32)) return fail(PZ_EINVAL, "the pool reports %llu rows", (unsigned long long)rows);
  att_pool_note_rows(pool, rows);
  if (fit[kFitFlag])
    return fail(PZ_ERANGE, "a pending ShardBlockHash is longer than the records' stride of %u bytes; nothing changed", h->stride);

  // 2: justify
  stamp(ev, 2, s);
  hipLaunchKernelGGL(pz_rs_justify_kernel, dim3(1), dim3(64), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_rs_justify_kernel");
  stamp(ev, 3, s);

  // 3: the epoch, one instance over the pool's view
  pz_epoch_batch eb;
  std::memset(&eb, 0, sizeof eb);
  eb.ninst = 1;
  eb.nval = eb.nval_global = b.nval;
  eb.kind = PZ_KIND_ACTIVE;
  eb.balance = b.balance, eb.start = b.start, eb.end = b.end;
  eb.dynasty = a.scalars + PZ_RS_CURRENT_DYNASTY;
  eb.total_deposit = a.scalars + PZ_RS_TOTAL_DEPOSITS;
  eb.natt = (uint32_t)rows;
  eb.bits = pv.cols.attester_bitfield, eb.boffs = pv.cols.attester_bitfield_offs;
  eb.max_inst_bytes = fit[kFitCounts + 3];
  eb.pop_rank = 0, eb.pop_world = 1;
  eb.committee = b.members, eb.coffs = b.coffs;
  eb.att_comm = pv.committee, eb.att_shard = pv.shard32;
  eb.nrec = h->nrec;
  eb.rec_dynasty = a.rec_dynasty;
  eb.winner = reinterpret_cast<uint32_t*>(p + l.winner);
  eb.vote = reinterpret_cast<uint64_t*>(p + l.vote);
  eb.total = reinterpret_cast<uint64_t*>(p + l.total);
  eb.scal = reinterpret_cast<uint64_t*>(p + l.scal);
  eb.act_mask = reinterpret_cast<uint64_t*>(p + l.act_mask);
  eb.blk_cnt = reinterpret_cast<uint32_t*>(p + l.blk_cnt);
  eb.act_list = reinterpret_cast<uint32_t*>(p + l.act_list);
  if ((rc = pz_dev_epoch_count(&eb, s))) return rc;
  stamp(ev, 4, s);
  if ((rc = pz_dev_epoch_finish(&eb, s))) return rc;
  stamp(ev, 5, s);

  // 4: commit
  hipLaunchKernelGGL(pz_rs_commit_kernel, dim3(std::max<uint32_t>((h->nrec + kRsThreads - 1) / kRsThreads, 1)),
                     dim3(kRsThreads), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_rs_commit_kernel");
  stamp(ev, 6, s);

  // 5: prune, by the lastStateRecalc the wait brought
  if ((rc = pz_dev_att_pool_prune(pool, fit[kFitLsr], s))) return rc;
  stamp(ev, 7, s);
  return PZ_OK;
}

}  // namespace

Resident* resident_of(pz_recalc_state* h) { return h; }

int recalc_state_view(pz_recalc_state* h, RsView* v, hipStream_t s, bool record) {
  if (!h || !v) return fail(PZ_EINVAL, "recalc state is null");
  std::lock_guard<std::mutex> lk(h->mu);
  v->device = h->device;
  v->nrec = h->nrec, v->stride = h->stride;
  v->words = static_cast<const uint64_t*>(h->words.ptr);
  v->rec_dynasty = static_cast<const uint64_t*>(h->rec_dynasty.ptr);
  v->rec_slot = static_cast<const uint64_t*>(h->rec_slot.ptr);
  v->rec_hash = static_cast<const uint8_t*>(h->rec_hash.ptr);
  v->rec_hash_len = static_cast<const uint32_t*>(h->rec_hash_len.ptr);
  if (record) h->last = s;
  return PZ_OK;
}

}  // namespace pz

using namespace pz;

namespace {

int check_call(const pz_recalc_state* h, const pz_att_pool* pool, const pz_recalc_batch* b, const void* d_scratch) {
  if (!h || !pool || !b || !d_scratch) return fail(PZ_EINVAL, "recalc: null state / pool / batch / scratch");
  if (!b->balance || !b->start || !b->end || !b->members || !b->coffs || !b->recent)
    return fail(PZ_EINVAL, "recalc batch: null balance / start / end / members / coffs / recent");
  if (!aligned16(b->recent) || !aligned16(d_scratch))
    return fail(PZ_EINVAL, "recalc: recent and d_scratch must be 16-B aligned device pointers");
  if (b->n_recent < PZ_CYCLE_LENGTH)
    return fail(PZ_EINDEX, "stateRecalc: RecentBlockHashes()[i], index out of range with %llu hashes (core.go:413)",
                (unsigned long long)b->n_recent);
  return PZ_OK;
}

}  // namespace

extern "C" {

int pz_recalc_state_new(uint32_t nrec, uint32_t hash_stride, const uint64_t scalars[PZ_RS_COUNT], const uint64_t* rec_dynasty,
                        const uint64_t* rec_slot, const uint8_t* rec_hash, const uint64_t* rec_hash_offs, int device,
                        pz_recalc_state** out) {
  if (!out) return fail(PZ_EINVAL, "out is null");
  *out = nullptr;
  if (!scalars) return fail(PZ_EINVAL, "scalars is null");
  if (!rs_stride_ok(hash_stride)) return fail(PZ_EINVAL, "hash_stride %u: not a multiple of 16 in [32, 256]", hash_stride);
  if (nrec && (!rec_dynasty || !rec_slot || !rec_hash_offs)) return fail(PZ_EINVAL, "null crosslink record columns");
  std::vector<uint8_t> hashes((size_t)std::max<uint32_t>(nrec, 1) * hash_stride, 0);
  std::vector<uint32_t> lens(std::max<uint32_t>(nrec, 1), 0);
  for (uint32_t r = 0; r < nrec; ++r) {
    const uint64_t lo = rec_hash_offs[r], hi = rec_hash_offs[r + 1];
    if (hi < lo) return fail(PZ_EINVAL, "crosslink record %u: inverted hash range", r);
    if (hi - lo > hash_stride)
      return fail(PZ_ERANGE, "crosslink record %u: a hash of %llu bytes, stride %u", r, (unsigned long long)(hi - lo), hash_stride);
    if (hi > lo && !rec_hash) return fail(PZ_EINVAL, "rec_hash is null");
    if (hi > lo) std::memcpy(hashes.data() + (size_t)r * hash_stride, rec_hash + lo, hi - lo);
    lens[r] = (uint32_t)(hi - lo);
  }
  int rc = Resident::open(device);
  if (rc) return rc;
  auto* h = new pz_recalc_state();
  h->device = device;
  h->nrec = nrec;
  h->stride = hash_stride;
  uint64_t words[PZ_RS_COUNT + 1] = {};
  std::memcpy(words, scalars, PZ_RS_COUNT * 8);
  const char* what = "recalc state init";
  const size_t n1 = std::max<uint32_t>(nrec, 1);
  hipError_t e;
  if ((rc = h->words.fill(sizeof words, 0, what, words, sizeof words)) ||
      (rc = h->rec_dynasty.fill(n1 * 8, 0, what, rec_dynasty, nrec * 8ull)) ||
      (rc = h->rec_slot.fill(n1 * 8, 0, what, rec_slot, nrec * 8ull)) ||
      (rc = h->rec_hash.fill(hashes.size(), 0, what, hashes.data(), hashes.size())) ||
      (rc = h->rec_hash_len.fill(n1 * 4, 0, what, lens.data(), n1 * 4)) || (rc = h->winner.fill(n1 * 4, 0xFF, what)) ||
      ((e = hipDeviceSynchronize()) != hipSuccess && (rc = hip_fail(e, what)))) {
    delete h;
    return rc;
  }
  *out = h;
  return PZ_OK;
}

void pz_recalc_state_free(pz_recalc_state* h) { delete h; }

int pz_recalc_state_read(pz_recalc_state* h, uint64_t scalars[PZ_RS_COUNT], uint64_t* rec_dynasty, uint64_t* rec_slot,
                         uint8_t* rec_hash, uint32_t* rec_hash_len, uint32_t* winner) {
  if (!h) return fail(PZ_EINVAL, "recalc state is null");
  int rc = h->use();
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  uint64_t w[PZ_RS_COUNT + 1] = {};
  if ((rc = h->settle(w, h->words, sizeof w, "recalc state read"))) return rc;
  if (scalars) std::memcpy(scalars, w, PZ_RS_COUNT * 8);
  const uint64_t n = h->nrec;
  const char* what = "recalc state read";
  if ((rc = down(rec_dynasty, h->rec_dynasty.ptr, n, what)) || (rc = down(rec_slot, h->rec_slot.ptr, n, what)) ||
      (rc = down(rec_hash, h->rec_hash.ptr, n * h->stride, what)) || (rc = down(rec_hash_len, h->rec_hash_len.ptr, n, what)) ||
      (rc = down(winner, h->winner.ptr, n, what)))
    return rc;
  if (w[PZ_RS_COUNT] & kRsErrPanic)
    return fail(PZ_EINDEX, "stateRecalc would panic (processCrosslinks' indices or CalculateRewards' CheckBit); the state is as before it");
  return PZ_OK;
}

uint64_t pz_state_recalc_scratch_bytes(uint64_t nval, uint64_t rows_cap, uint32_t nrec) { return layout(nval, rows_cap, nrec).end; }

int pz_dev_state_recalc(pz_recalc_state* h, pz_att_pool* pool, pz_vote_cache* cache, const pz_recalc_batch* b, void* d_scratch,
                        void* stream) {
  int rc = check_call(h, pool, b, d_scratch);
  if (rc) return rc;
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return enqueue(h, pool, cache, *b, d_scratch, s);
}

#ifdef PZ_AB_BUILD
// (tools/recalc_probe.py) pz_dev_state_recalc with one event pair per step; synchronises and
// returns the milliseconds of fit, justify, epoch count, epoch finish, commit and prune in ms[0..6).
int pz_debug_state_recalc_timed(pz_recalc_state* h, pz_att_pool* pool, pz_vote_cache* cache, const pz_recalc_batch* b,
                                void* d_scratch, void* stream, float ms[6]) {
  int rc = check_call(h, pool, b, d_scratch);
  if (rc) return rc;
  if (!ms) return fail(PZ_EINVAL, "null pointer");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  Events ev;
  if ((rc = ev.create(8))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  static const int kFrom[6] = {0, 2, 3, 4, 5, 6};
  return ev.elapsed(enqueue(h, pool, cache, *b, d_scratch, s, &ev), ms, kFrom, 6, s, "timed state recalc");
}
#endif

}  // extern "C"
