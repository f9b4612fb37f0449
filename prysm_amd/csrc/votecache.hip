// A device-resident block vote cache fed from decoded attestation columns, for gfx950.
//
// calculateBlockVoteCache (blockchain/core.go:300-345) over the columns pz_dev_unwire_attestations
// and pz_dev_check_attestations leave on the device: the handle owns the map from 32-byte hash to
// slot (an open-addressing table, votecache_dev.h) beside the per-slot voter bitmaps and totals
// (pz_vote_batch's layout, so votes_dev.h tally_item tallies into them unchanged).  No host work
// list, no host hash map, no readback between the checks and the tally.
//
// One call is four dependent launches on the caller's stream.  No workgroup ever waits for
// another (no spin, no look-back, no polling): every cross-workgroup fact travels through a
// launch boundary or through the value an atomic returns.
//   1 mark    a wave per attestation, lane r = signed parent r: the oblique skip rule, then
//             used[source] = 1 for every tallied parent and mask[att] = the tallied parents' bits.
//   2 intern  a lane per used source probes the table from its home cell.  A committed cell is
//             compared with keys[slot] (written by an earlier launch); a tentative one with the
//             bytes of the source that claimed it (launch inputs); an empty one is claimed by
//             atomicCAS, and a lost CAS re-examines the value it returned.  Equal sources
//             atomicMin the cell: it ends holding the smallest source index of its group.  Cells
//             are read with relaxed agent-scope atomic loads and written only with atomics;
//             during this launch a cell only ever goes empty -> claimed -> claimed lower, so
//             every lane of a group walks the same cells and stops at the same one.
//   3 commit  one workgroup numbers the new groups by ascending smallest source index (recent
//             positions, then oblique elements: slot ids do not depend on scheduling), writes
//             keys, turns the claims into slot ids, fills src_slot for every used source and
//             advances nslots -- or, if a probe ran out or the slots do not fit, puts every claim
//             back to empty, sets the sticky error word and marks the call void: a call lands
//             whole or not at all.
//   4 tally   a wave per (attestation, parent r): tally_item into the parent's slot.
//
// A lookup (the `if _, ok := blockVoteCache[blockHash]` of core.go:414-418) is one launch between
// calls: a lane per query walks the table with votecache_dev.h's vc_probe, plain loads only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "att_cols.h"
#include "resident.h"
#include "votecache_dev.h"
#include "votes_dev.h"

struct pz_vote_cache : pz::Resident {  // (last: read / voters / the host forms wait for it)
  uint64_t nval = 0, words = 0;
  uint32_t slot_cap = 0, cells = 0;
  pz::DevBuf bitmaps, totals, keys, table, words2;  // words2: nslots (u32) at 0, the error word (u64) at 8
  ~pz_vote_cache() {
    drain();
    for (pz::DevBuf* b : {&bitmaps, &totals, &keys, &table, &words2}) b->release();
  }
};

namespace pz {
namespace {

constexpr int kThreads = 256;
constexpr int kCommitThreads = 1024;
constexpr uint32_t kFlagOverflow = 0, kFlagVoid = 1, kFlagNew = 2;  // scratch flags (u32 x 4)

struct VcArgs {
  pz_vote_cols_batch b;
  uint32_t* bitmaps;
  uint64_t* totals;
  uint8_t* keys;
  uint32_t* table;
  uint32_t* nslots;
  uint64_t* err;
  uint64_t nval, words;
  uint32_t slot_cap, cells;
  uint64_t nsrc;  // n_recent + n_oblique_total
  // scratch
  uint32_t* flags;
  uint8_t* used;
  uint32_t* src_slot;
  uint32_t* src_cell;
  uint64_t* mask;
};

#define PZ_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ Hash32 source_hash(const VcArgs& a, uint64_t s) {
  if (s < a.b.n_recent) return vc_load_hash(a.b.recent + 32 * s);
  const uint64_t e = s - a.b.n_recent;
  return vc_bytes_to_hash(a.b.oblique_parent_hashes, a.b.oblique_offs[e], a.b.oblique_offs[e + 1]);
}

// ---- 1: mark -----------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kThreads) pz_vc_mark_kernel(VcArgs a) {
  const uint64_t i = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  if (i >= a.b.natt) return;  // (wave-uniform, as everything below up to the lanes' parents)
  bool ok = a.b.status[i] == PZ_ATT_PROCESSED && (!a.b.take || a.b.take[i] != 0);
  uint64_t m = 0, f0 = 0, ps = 0;
  if (ok) {
    ps = a.b.parents_start[i];
    if (a.b.oblique_first) {
      f0 = a.b.oblique_first[i];
      const uint64_t f1 = a.b.oblique_first[i + 1];
      m = f1 - f0;
      if (f1 < f0 || f1 > a.b.n_oblique_total) ok = false;
    }
    if (ok && a.b.n_oblique && a.b.n_oblique[i] != m) ok = false;  // (columns that disagree)
    if (ok && !vc_parents_in_range(m, ps, a.b.n_recent)) ok = false;
  }
  if (ok && a.b.committee[i] >= a.b.ncomm) {  // core.go:367's index: Go panics
    ok = false;
    if (lane == 0) atomicOr((unsigned long long*)a.err, (unsigned long long)kVcErrPanic);
  }
  uint64_t mask = 0;
  if (ok) {
    const uint64_t nrec = kVcParents - m;
    const uint64_t src = vc_parent_source(lane, m, ps, f0, a.b.n_recent);
    Hash32 h;
    uint64_t len = 0;
    if (lane < nrec) {
      h = vc_load_hash(a.b.recent + 32 * src);
    } else {
      const uint64_t e = src - a.b.n_recent, lo = a.b.oblique_offs[e], hi = a.b.oblique_offs[e + 1];
      len = hi > lo ? hi - lo : 0;
      h = vc_bytes_to_hash(a.b.oblique_parent_hashes, lo, hi);
    }
    // the record's raw 32-byte obliques are their lanes' own hashes: each goes wave-wide by
    // readlane and every lane compares its parent with it (its own position included)
    uint64_t raw = __ballot(len == 32);
    bool skip = false;
    while (raw) {  // (wave-uniform)
      const int q = __builtin_ctzll(raw);
      raw &= raw - 1;
      Hash32 e;
#pragma unroll
      for (int k = 0; k < 8; ++k) e.w[k] = (uint32_t)__builtin_amdgcn_readlane((int)h.w[k], q);
      skip = skip || vc_skipped_by(h, e, 32);
    }
    if (!skip) a.used[src] = 1;
    mask = __ballot(!skip);
  }
  if (lane == 0) a.mask[i] = mask;
}

// ---- 2: intern -----------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kThreads) pz_vc_intern_kernel(VcArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= a.nsrc || !a.used[s]) return;
  const Hash32 h = source_hash(a, s);
  const uint32_t mine = vc_claim((uint32_t)s);
  uint32_t slot = kVcNone, cell = kVcNone;
  uint32_t c = vc_home(h, a.cells);
  bool done = false;
  for (uint32_t step = 0; step < a.cells && !done; ++step, c = vc_next(c, a.cells)) {
    uint32_t v = __hip_atomic_load(&a.table[c], PZ_RLX_AGENT);
    if (vc_is_empty(v)) {
      v = atomicCAS(&a.table[c], kVcEmpty, mine);  // a lost CAS returns the winner's claim
      if (vc_is_empty(v)) {
        cell = c;
        done = true;
      }
    }
    if (done) break;
    if (vc_is_slot(v)) {
      if (vc_hash_eq(h, vc_load_hash(a.keys + 32ull * v))) {
        slot = v;
        done = true;
      }
    } else {
      const uint32_t t = vc_claim_source(v);
      if (t == (uint32_t)s || vc_hash_eq(h, source_hash(a, t))) {
        if (mine < v) atomicMin(&a.table[c], mine);
        cell = c;
        done = true;
      }
    }
  }
  if (!done) atomicOr(&a.flags[kFlagOverflow], 1u);  // every cell holds another hash
  a.src_slot[s] = slot;
  a.src_cell[s] = cell;
}

// ---- 3: commit (one workgroup) ---------------------------------------------------------------
// A source is a leader when the cell it remembered holds its own claim: the smallest index of a
// new group.  Pass a gives the leaders their slot ids in ascending source order; pass b writes
// the leaders' keys and gives every other source of a new group its leader's id; pass c turns
// the leaders' cells into slot ids.  src_slot words that another thread of the workgroup wrote are
// read with agent-scope loads.
extern "C" __global__ void __launch_bounds__(kCommitThreads) pz_vc_commit_kernel(VcArgs a) {
  __shared__ uint32_t wcount[kCommitThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t old = *a.nslots;
  auto claimed = [&](uint64_t s) { return s < a.nsrc && a.used[s] && a.src_cell[s] != kVcNone; };
  auto leads = [&](uint64_t s) {
    return claimed(s) && __hip_atomic_load(&a.table[a.src_cell[s]], PZ_RLX_AGENT) == vc_claim((uint32_t)s);
  };
  uint64_t base = 0;
  for (uint64_t s0 = 0; s0 < a.nsrc; s0 += kCommitThreads) {  // (block-uniform)
    const uint64_t s = s0 + tid;
    const bool lead = leads(s);
    const uint64_t bal = __ballot(lead);
    if (lane == 0) wcount[wv] = (uint32_t)__builtin_popcountll(bal);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < kCommitThreads / 64; ++w) {
      before += w < wv ? wcount[w] : 0;
      total += wcount[w];
    }
    if (lead) {
      const uint64_t rank = base + before + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1));
      __hip_atomic_store(&a.src_slot[s], (uint32_t)(old + rank), PZ_RLX_AGENT);
    }
    base += total;
    __syncthreads();
  }
  const bool is_void = a.flags[kFlagOverflow] != 0 || (uint64_t)old + base > a.slot_cap;
  if (is_void) {
    for (uint64_t s = tid; s < a.nsrc; s += kCommitThreads)
      if (leads(s)) atomicExch(&a.table[a.src_cell[s]], kVcEmpty);
    if (tid == 0) {
      atomicOr((unsigned long long*)a.err, (unsigned long long)kVcErrCapacity);
      a.flags[kFlagVoid] = 1;
    }
    return;
  }
  for (uint64_t s = tid; s < a.nsrc; s += kCommitThreads) {
    if (!claimed(s)) continue;
    const uint32_t v = __hip_atomic_load(&a.table[a.src_cell[s]], PZ_RLX_AGENT);
    const uint32_t t = vc_claim_source(v);
    const uint32_t slot = __hip_atomic_load(&a.src_slot[t], PZ_RLX_AGENT);
    if (t == (uint32_t)s) {
      const Hash32 h = source_hash(a, s);
      uint32_t* k = reinterpret_cast<uint32_t*>(a.keys + 32ull * slot);
#pragma unroll
      for (int j = 0; j < 8; ++j) k[j] = h.w[j];
    } else {
      a.src_slot[s] = slot;
    }
  }
  __syncthreads();  // every claim has been read: now they become slot ids
  for (uint64_t s = tid; s < a.nsrc; s += kCommitThreads)
    if (leads(s)) atomicExch(&a.table[a.src_cell[s]], __hip_atomic_load(&a.src_slot[s], PZ_RLX_AGENT));
  if (tid == 0) {
    *a.nslots = old + (uint32_t)base;
    a.flags[kFlagNew] = (uint32_t)base;
  }
}

// ---- 4: tally --------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kThreads) pz_vc_tally_kernel(VcArgs a) {
  const uint64_t w = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
  const uint64_t i = w >> 6;
  const uint32_t r = (uint32_t)(w & 63);
  if (i >= a.b.natt || a.flags[kFlagVoid]) return;  // (wave-uniform)
  if (!((a.mask[i] >> r) & 1)) return;
  uint64_t m = 0, f0 = 0;
  if (a.b.oblique_first) {
    f0 = a.b.oblique_first[i];
    m = a.b.oblique_first[i + 1] - f0;
  }
  const uint64_t src = vc_parent_source(r, m, a.b.parents_start[i], f0, a.b.n_recent);
  const uint32_t slot = a.src_slot[src];
  const uint64_t bb = a.b.boffs[i];
  tally_item(a.b.members, a.b.coffs, a.b.committee[i], a.b.bits + bb, a.b.boffs[i + 1] - bb, a.b.balance, a.nval,
             a.bitmaps + (uint64_t)slot * a.words, a.totals + slot, a.err);
}

// ---- lookup: a read between calls ---------------------------------------------------------------
// A lane per query.  No launch writes the table, the keys or nslots while this one runs (the
// caller orders it after the cache's earlier calls), so none of the intern launch's atomics.
struct VcLookupArgs {
  const uint32_t* table;
  const uint8_t* keys;
  const uint32_t* nslots;
  const uint64_t* totals;
  uint32_t slot_cap, cells;
  const uint8_t* hashes;  // n x 32 B, 16-byte aligned
  uint64_t n;
  uint64_t* out_totals;
  uint32_t* out_slots;  // optional
};

extern "C" __global__ void __launch_bounds__(kThreads) pz_vc_lookup_kernel(VcLookupArgs a) {
  const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= a.n) return;
  const uint32_t ns = *a.nslots < a.slot_cap ? *a.nslots : a.slot_cap;
  const uint32_t slot = vc_probe(a.table, a.cells, a.keys, ns, vc_load_hash16(a.hashes + 32 * q));
  a.out_totals[q] = slot == kVcNone ? 0 : a.totals[slot];
  if (a.out_slots) a.out_slots[q] = slot;
}

// ---- host side ---------------------------------------------------------------------------------
// What can be told without reading a column; 1: nothing to do.
int check_args(const pz_vote_cache* h, const pz_vote_cols_batch* b) {
  if (!h) return fail(PZ_EINVAL, "vote cache is null");
  if (!b) return fail(PZ_EINVAL, "batch is null");
  if (b->natt == 0) return 1;
  if (!b->bits || !b->boffs || !b->status || !b->committee || !b->parents_start || !b->members || !b->coffs ||
      !b->balance)
    return fail(PZ_EINVAL, "vote columns: null bits / boffs / status / committee / parents_start / members / coffs / balance");
  if ((b->oblique_offs || b->oblique_first) && !b->oblique_parent_hashes)
    return fail(PZ_EINVAL, "oblique offsets without oblique_parent_hashes");
  if (b->n_oblique_total > 0 && (!b->oblique_parent_hashes || !b->oblique_offs || !b->oblique_first))
    return fail(PZ_EINVAL, "n_oblique_total %llu without the oblique columns", (unsigned long long)b->n_oblique_total);
  if (b->oblique_first && !b->oblique_offs) return fail(PZ_EINVAL, "oblique_first without oblique_offs");
  if (b->n_recent > 0 && !b->recent) return fail(PZ_EINVAL, "recent is null");
  if (b->n_recent >= (1ull << 31) || b->n_oblique_total >= (1ull << 31) || b->n_recent + b->n_oblique_total >= (1ull << 31))
    return fail(PZ_EINVAL, "%llu recent hashes + %llu oblique elements: 2^31 sources or more",
                (unsigned long long)b->n_recent, (unsigned long long)b->n_oblique_total);
  if (b->natt >= (1ull << 27)) return fail(PZ_EINVAL, "natt %llu: 2^27 attestations or more", (unsigned long long)b->natt);
  return PZ_OK;
}

uint64_t scratch_bytes(uint64_t natt, uint64_t nsrc) { return 16 + r16(nsrc) + 2 * r16(4 * nsrc) + r16(8 * natt); }

// The four launches (and the memset of the flags and used[]) on s.  ev (the A/B library's timed
// entry; null in the product): five events, one before the first launch and one after each.
int enqueue(pz_vote_cache* h, const pz_vote_cols_batch& b, void* d_scratch, hipStream_t s, Events* ev = nullptr) {
  VcArgs a;
  std::memset(&a, 0, sizeof a);
  a.b = b;
  a.bitmaps = static_cast<uint32_t*>(h->bitmaps.ptr);
  a.totals = static_cast<uint64_t*>(h->totals.ptr);
  a.keys = static_cast<uint8_t*>(h->keys.ptr);
  a.table = static_cast<uint32_t*>(h->table.ptr);
  a.nslots = static_cast<uint32_t*>(h->words2.ptr);
  a.err = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(h->words2.ptr) + 8);
  a.nval = h->nval, a.words = h->words, a.slot_cap = h->slot_cap, a.cells = h->cells;
  a.nsrc = b.n_recent + b.n_oblique_total;
  uint8_t* p = static_cast<uint8_t*>(d_scratch);
  a.flags = reinterpret_cast<uint32_t*>(p);
  a.used = p + 16;
  a.src_slot = reinterpret_cast<uint32_t*>(p + 16 + r16(a.nsrc));
  a.src_cell = reinterpret_cast<uint32_t*>(p + 16 + r16(a.nsrc) + r16(4 * a.nsrc));
  a.mask = reinterpret_cast<uint64_t*>(p + 16 + r16(a.nsrc) + 2 * r16(4 * a.nsrc));
  hipError_t e = hipMemsetAsync(p, 0, 16 + r16(a.nsrc), s);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
  h->last = s;
  const uint32_t wave_blocks = (uint32_t)((b.natt * 64 + kThreads - 1) / kThreads);
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_vc_mark_kernel, dim3(wave_blocks), dim3(kThreads), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_vc_mark_kernel");
  stamp(ev, 1, s);
  if (a.nsrc) {
    hipLaunchKernelGGL(pz_vc_intern_kernel, dim3((uint32_t)((a.nsrc + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_vc_intern_kernel");
  }
  stamp(ev, 2, s);
  hipLaunchKernelGGL(pz_vc_commit_kernel, dim3(1), dim3(kCommitThreads), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_vc_commit_kernel");
  stamp(ev, 3, s);
  hipLaunchKernelGGL(pz_vc_tally_kernel, dim3(64 * wave_blocks), dim3(kThreads), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_vc_tally_kernel");
  stamp(ev, 4, s);
  return PZ_OK;
}

// Waits for the last tally and reads nslots and the sticky error word; the code to report.
int settle(pz_vote_cache* h, uint32_t* nslots, int* sticky) {
  uint64_t w[2] = {0, 0};
  int rc = h->settle(w, h->words2, sizeof w, "vote cache read");
  if (rc) return rc;
  *nslots = (uint32_t)w[0];
  *sticky = (w[1] & kVcErrPanic)      ? PZ_EINDEX
            : (w[1] & kVcErrCapacity) ? PZ_ERANGE
                                      : PZ_OK;
  return PZ_OK;
}

int report(int sticky) {
  if (sticky == PZ_EINDEX)
    return fail(PZ_EINDEX, "calculateBlockVoteCache would panic (committee index, short bitfield or voter >= len(validators))");
  if (sticky == PZ_ERANGE) return fail(PZ_ERANGE, "a tally call needed more slots than the vote cache holds; it was dropped whole");
  return PZ_OK;
}

int check_lookup(const pz_vote_cache* h, const uint8_t* hashes, uint64_t n, const uint64_t* totals) {
  if (!h) return fail(PZ_EINVAL, "vote cache is null");
  if (n == 0) return 1;
  if (!hashes || !totals) return fail(PZ_EINVAL, "lookup: null hashes / totals");
  if (n >> 38) return fail(PZ_EINVAL, "more than 2^38 queries");
  return PZ_OK;
}

int enqueue_lookup(pz_vote_cache* h, const uint8_t* d_hashes, uint64_t n, uint64_t* d_totals, uint32_t* d_slots,
                   hipStream_t s) {
  if (!aligned16(d_hashes)) return fail(PZ_EINVAL, "lookup: hashes must be 16-B aligned");
  VcLookupArgs a;
  a.table = static_cast<const uint32_t*>(h->table.ptr);
  a.keys = static_cast<const uint8_t*>(h->keys.ptr);
  a.nslots = static_cast<const uint32_t*>(h->words2.ptr);
  a.totals = static_cast<const uint64_t*>(h->totals.ptr);
  a.slot_cap = h->slot_cap, a.cells = h->cells;
  a.hashes = d_hashes, a.n = n, a.out_totals = d_totals, a.out_slots = d_slots;
  h->last = s;
  hipLaunchKernelGGL(pz_vc_lookup_kernel, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_vc_lookup_kernel");
}

}  // namespace

int vote_cache_view(pz_vote_cache* h, VcView* v, hipStream_t s) {
  if (!h || !v) return fail(PZ_EINVAL, "vote cache is null");
  std::lock_guard<std::mutex> lk(h->mu);
  v->device = h->device;
  v->nval = h->nval;
  v->slot_cap = h->slot_cap, v->cells = h->cells;
  v->table = static_cast<const uint32_t*>(h->table.ptr);
  v->keys = static_cast<const uint8_t*>(h->keys.ptr);
  v->nslots = static_cast<const uint32_t*>(h->words2.ptr);
  v->totals = static_cast<const uint64_t*>(h->totals.ptr);
  h->last = s;
  return PZ_OK;
}

}  // namespace pz

using namespace pz;

extern "C" {

int pz_dev_vote_cache_lookup(pz_vote_cache* h, const uint8_t* d_hashes, uint64_t n, uint64_t* d_totals, uint32_t* d_slots,
                             void* stream) {
  int rc = check_lookup(h, d_hashes, n, d_totals);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  return enqueue_lookup(h, d_hashes, n, d_totals, d_slots, static_cast<hipStream_t>(stream));
}

int pz_vote_cache_lookup(pz_vote_cache* h, const uint8_t* hashes, uint64_t n, uint64_t* totals, uint32_t* slots) {
  int rc = check_lookup(h, hashes, n, totals);
  if (rc) return rc < 0 ? rc : PZ_OK;
  HostForm f(h, "vote cache lookup");  // (the staging stream is not the last tally's: it waits)
  if (f.rc) return f.rc;
  Stager& st = f.st;
  const uint8_t* d_hashes = st.up(hashes, n * 32);
  uint64_t* d_totals = st.up<uint64_t>(nullptr, n);
  uint32_t* d_slots = slots ? st.up<uint32_t>(nullptr, n) : nullptr;
  if (st.rc) return st.rc;
  if ((rc = enqueue_lookup(h, d_hashes, n, d_totals, d_slots, st.s))) return rc;
  st.down(totals, static_cast<const uint64_t*>(d_totals), n);
  if (slots) st.down(slots, static_cast<const uint32_t*>(d_slots), n);
  return st.sync();
}

int pz_vote_cache_new(uint64_t nval, uint32_t slot_cap, int device, pz_vote_cache** out) {
  if (!out) return fail(PZ_EINVAL, "out is null");
  *out = nullptr;
  if (nval > PZ_MAX_VALIDATORS) return fail(PZ_ETOOMANY, "validator count %llu above MaxValidators", (unsigned long long)nval);
  if (nval == 0 || slot_cap == 0 || slot_cap > kVcMaxSlotCap)
    return fail(PZ_EINVAL, "vote cache of %llu validators and %u slots", (unsigned long long)nval, slot_cap);
  int rc = Resident::open(device);
  if (rc) return rc;
  hipError_t e;
  auto* h = new pz_vote_cache();
  h->device = device;
  h->nval = nval;
  h->words = (nval + 31) / 32;
  h->slot_cap = slot_cap;
  h->cells = vc_cells(slot_cap);
  const size_t bm = (size_t)slot_cap * h->words * 4;
  const char* what = "vote cache init";
  if ((rc = h->bitmaps.fill(bm, 0, what)) || (rc = h->totals.fill((size_t)slot_cap * 8, 0, what)) ||
      (rc = h->keys.fill((size_t)slot_cap * 32, 0, what)) || (rc = h->table.fill((size_t)h->cells * 4, 0xFF, what)) ||
      (rc = h->words2.fill(16, 0, what)) || ((e = hipDeviceSynchronize()) != hipSuccess && (rc = hip_fail(e, what)))) {
    delete h;
    return rc;
  }
  *out = h;
  return PZ_OK;
}

void pz_vote_cache_free(pz_vote_cache* h) { delete h; }

uint64_t pz_vote_cache_scratch_bytes(uint64_t natt, uint64_t n_recent, uint64_t n_oblique_total) {
  return scratch_bytes(natt, n_recent + n_oblique_total);
}

int pz_dev_vote_cache_tally(pz_vote_cache* h, const pz_vote_cols_batch* b, void* d_scratch, void* stream) {
  int rc = check_args(h, b);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!d_scratch || !aligned16(d_scratch)) return fail(PZ_EINVAL, "d_scratch must be a 16-B aligned device pointer");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  return enqueue(h, *b, d_scratch, static_cast<hipStream_t>(stream));
}

#ifdef PZ_AB_BUILD
// (tools/votecache_probe.py) pz_dev_vote_cache_tally with one event pair per launch; synchronises
// and returns the four phases' milliseconds (mark, intern, commit, tally) in ms[0..4).
int pz_debug_vote_cache_tally_timed(pz_vote_cache* h, const pz_vote_cols_batch* b, void* d_scratch, void* stream,
                                    float ms[4]) {
  int rc = check_args(h, b);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!d_scratch || !ms) return fail(PZ_EINVAL, "null pointer");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  Events ev;
  if ((rc = ev.create(5))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return ev.elapsed(enqueue(h, *b, d_scratch, s, &ev), ms, nullptr, 4, s, "timed vote cache tally");
}
#endif

int pz_vote_cache_tally(pz_vote_cache* h, const pz_vote_cols_batch* hb) {
  int rc = check_args(h, hb);
  if (rc) return rc < 0 ? rc : PZ_OK;
  const uint64_t n = hb->natt, ne = hb->n_oblique_total;
  if ((rc = check_csr(hb->boffs, n, "bitfield")) || (rc = check_csr(hb->coffs, hb->ncomm, "committee"))) return rc;
  if (hb->oblique_first) {
    if ((rc = check_csr(hb->oblique_first, n, "oblique_first")) || (rc = check_csr(hb->oblique_offs, ne, "oblique"))) return rc;
    if (hb->oblique_first[n] > ne) return fail(PZ_EINVAL, "oblique_first reaches past n_oblique_total");
  }
  HostForm f(h, "vote cache tally");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_vote_cols_batch d = *hb;
  if (hb->n_oblique) d.n_oblique = st.up(hb->n_oblique, n);
  pz_attestation_cols hc{}, dc;  // the batch's attestation columns under their pz_attestation_cols names
  hc.oblique_parent_hashes = hb->oblique_parent_hashes, hc.oblique_offs = hb->oblique_offs, hc.oblique_first = hb->oblique_first;
  hc.attester_bitfield = hb->bits, hc.attester_bitfield_offs = hb->boffs;
  uint64_t staged[kAttTotals];
  stage_att_cols(st, hc, n, kAttObliqueCols | kAttBitsCols, &dc, staged);
  d.oblique_parent_hashes = dc.oblique_parent_hashes, d.oblique_offs = dc.oblique_offs, d.oblique_first = dc.oblique_first;
  d.n_oblique_total = staged[kTotElems];  // the sources are the elements the rows name
  d.bits = dc.attester_bitfield, d.boffs = dc.attester_bitfield_offs;
  d.status = st.up(hb->status, n);
  d.committee = st.up(hb->committee, n);
  d.parents_start = st.up(hb->parents_start, n);
  if (hb->take) d.take = st.up(hb->take, n);
  d.recent = st.up(hb->recent, hb->n_recent * 32);
  d.members = st.up(hb->members, hb->coffs[hb->ncomm]);
  d.coffs = st.up(hb->coffs, hb->ncomm + 1);
  d.balance = st.up(hb->balance, h->nval);
  uint8_t* scr = st.up<uint8_t>(nullptr, scratch_bytes(n, hb->n_recent + d.n_oblique_total));
  if (st.rc) return st.rc;
  if ((rc = enqueue(h, d, scr, st.s))) return rc;
  return st.sync();
}

int pz_vote_cache_read(pz_vote_cache* h, uint8_t* hashes, uint64_t* totals, uint64_t cap, uint64_t* count) {
  if (!h || !count) return fail(PZ_EINVAL, "vote cache / count is null");
  int rc = h->use();
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  uint32_t ns;
  int sticky;
  if ((rc = settle(h, &ns, &sticky))) return rc;
  *count = ns;
  if (ns && cap >= ns) {
    hipError_t e = hipSuccess;
    if (hashes) e = hipMemcpy(hashes, h->keys.ptr, (size_t)ns * 32, hipMemcpyDeviceToHost);
    if (e == hipSuccess && totals) e = hipMemcpy(totals, h->totals.ptr, (size_t)ns * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "vote cache read");
  }
  return report(sticky);
}

int pz_vote_cache_voters(pz_vote_cache* h, const uint8_t hash[32], uint32_t* words, int* present) {
  if (!h || !hash || !present) return fail(PZ_EINVAL, "vote cache / hash / present is null");
  int rc = h->use();
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  uint32_t ns;
  int sticky;
  if ((rc = settle(h, &ns, &sticky))) return rc;
  // (a read-side lookup: the keys come to the host; the tally never does this)
  std::vector<uint8_t> keys((size_t)ns * 32);
  hipError_t e = ns ? hipMemcpy(keys.data(), h->keys.ptr, keys.size(), hipMemcpyDeviceToHost) : hipSuccess;
  if (e != hipSuccess) return hip_fail(e, "vote cache voters");
  *present = 0;
  uint32_t slot = 0;
  for (; slot < ns; ++slot)
    if (!std::memcmp(keys.data() + 32ull * slot, hash, 32)) break;
  if (slot < ns) {
    *present = 1;
    if (words) e = hipMemcpy(words, static_cast<uint32_t*>(h->bitmaps.ptr) + (size_t)slot * h->words, h->words * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "vote cache voters");
  } else if (words) {
    std::memset(words, 0, h->words * 4);
  }
  return report(sticky);
}

}  // extern "C"
