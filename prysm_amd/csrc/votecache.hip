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
//
// The reference's map only grows (types/state.go:27-31).  pz_[dev_]vote_cache_reserve gives the
// cache more slots and pz_[dev_]vote_cache_retain keeps only the entries a caller names; both move
// the entries into the handle's second buffer set, allocated at the first such call, and swap the
// sets (keep, renumber, move, rehash below; the rules and the retirement argument are
// votecache_dev.h's).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "att_cols.h"
#include "resident.h"
#include "tile_scan.h"
#include "votecache_dev.h"
#include "votes_dev.h"

struct pz_vote_cache : pz::Resident {  // (last: read / voters / the host forms wait for it)
  uint64_t nval = 0, words = 0;
  uint32_t slot_cap = 0, cells = 0;
  // Two buffer sets: set `live` is the map; the other one, allocated at the first reserve or retain,
  // is where that call moves the entries to before the sets swap (the pool's prune, the block set's
  // reserve).  words2: nslots (u32) at 0, the error word (u64) at 8 -- one pair for both sets.
  pz::DevBuf bitmaps[2], totals[2], keys[2], table[2], words2;
  int live = 0;
  ~pz_vote_cache() {
    drain();
    for (int k = 0; k < 2; ++k)
      for (pz::DevBuf* b : {&bitmaps[k], &totals[k], &keys[k], &table[k]}) b->release();
    words2.release();
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

// ---- reserve and retain: the entries move to the other buffer set ------------------------------
// A reserve is a memset of the new table and two launches (move, rehash); a retain puts a memset of
// the flags and two launches in front (keep, renumber).  Every fact crosses a launch boundary: the
// flags keep -> renumber, new nslots and old_of renumber -> move, the moved keys move -> rehash.
struct VcSet {
  uint32_t* bitmaps;
  uint64_t* totals;
  uint8_t* keys;
  uint32_t* table;
  uint32_t slot_cap, cells;
};

struct VcMoveArgs {
  VcSet from, to;
  uint32_t* nslots;  // the cache's count: the old one up to renumber, the new one after it
  uint64_t* err;
  uint64_t words;
  uint64_t per_row;  // move: lanes a destination row
  // a retain's scratch and keep-hashes (a reserve: NULL, every slot keeps its id)
  uint32_t* flag;
  uint32_t* new_id;
  uint32_t* old_of;
  const uint8_t* hashes;  // n x 32 B, 16-byte aligned
  uint64_t n;
};

__device__ __forceinline__ uint32_t vc_count(const uint32_t* nslots, uint32_t slot_cap) {
  const uint32_t ns = *nslots;
  return ns < slot_cap ? ns : slot_cap;
}

// keep: a lane per keep-hash.  Lanes that find the same slot store the same word.
extern "C" __global__ void __launch_bounds__(kThreads) pz_vc_keep_kernel(VcMoveArgs a) {
  const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= a.n) return;
  const uint32_t ns = vc_count(a.nslots, a.from.slot_cap);
  const uint32_t slot = vc_keep_mark(a.from.table, a.from.cells, a.from.keys, ns, vc_load_hash16(a.hashes + 32 * q));
  if (slot != kVcNone) a.flag[slot] = 1;
}

// renumber: ONE workgroup scans the flags a tile (tile_scan.h) at a time: new_id[old], old_of[new]
// for the move, and the new count into the cache's word.
extern "C" __global__ void __launch_bounds__(kTile) pz_vc_renumber_kernel(VcMoveArgs a) {
  __shared__ uint64_t s_tile;
  const uint32_t ns = vc_count(a.nslots, a.from.slot_cap);
  __syncthreads();  // every lane has read the old count before lane 0 writes the new one
  uint64_t kept_before = 0;
  for (uint64_t s0 = 0; s0 < ns; s0 += kTile) {  // (block-uniform)
    const uint64_t s = s0 + threadIdx.x;
    const bool kept = vc_kept(a.flag, ns, s);
    const uint64_t v[1] = {kept ? 1ull : 0ull};
    uint64_t ex[1];
    tile_excl<1>(v, ex);
    if (threadIdx.x == kTile - 1) s_tile = ex[0] + v[0];
    const uint32_t id = vc_new_id(kept, kept_before + ex[0]);
    if (s < ns) a.new_id[s] = id;
    if (kept) a.old_of[id] = (uint32_t)s;
    __syncthreads();
    kept_before += s_tile;
    __syncthreads();  // (s_tile and tile_excl's sums are read: the next tile may write them)
  }
  if (threadIdx.x == 0) *a.nslots = (uint32_t)kept_before;
}

// move: per_row lanes a destination row d of the new set, every row of it: below the new count the
// row of slot old_of[d] (a reserve: d), at or past it zeros -- the other set may hold an earlier
// swap's rows, and the tally counts on fresh slots reading zero.  Lane i moves 16-byte piece i of
// the voters (aligned stores; the source row may start at another dword: unaligned loads, which
// gfx950 runs); lane 0 also moves the head and tail dwords, the key and the total.
extern "C" __global__ void __launch_bounds__(kThreads) pz_vc_move_kernel(VcMoveArgs a) {
  const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint64_t d = g / a.per_row, i = g - d * a.per_row;
  if (d >= a.to.slot_cap) return;
  const uint32_t ns = vc_count(a.nslots, a.to.slot_cap);
  uint64_t o = 0;
  bool live = d < ns;
  if (live) {
    o = a.old_of ? a.old_of[d] : d;
    live = o < a.from.slot_cap;  // (always: old_of holds old slot ids)
    if (!live) o = 0;
  }
  const uint64_t w = a.words;
  uint32_t* dst = a.to.bitmaps + d * w;
  const uint32_t* src = a.from.bitmaps + o * w;
  const uint32_t head = vc_row_head(d * w, w);
  const uint64_t pieces = (w - head) / 4;
  if (i < pieces) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (live) __builtin_memcpy(&v, src + head + 4 * i, 16);
    *reinterpret_cast<uint4*>(__builtin_assume_aligned(dst + head + 4 * i, 16)) = v;
  }
  if (i != 0) return;
  for (uint64_t k = 0; k < head; ++k) dst[k] = live ? src[k] : 0;
  for (uint64_t k = head + 4 * pieces; k < w; ++k) dst[k] = live ? src[k] : 0;
  a.to.totals[d] = live ? a.from.totals[o] : 0;
  uint4 k0 = make_uint4(0, 0, 0, 0), k1 = k0;
  if (live) {
    const uint4* fk = reinterpret_cast<const uint4*>(a.from.keys + 32 * o);
    k0 = fk[0], k1 = fk[1];
  }
  uint4* tk = reinterpret_cast<uint4*>(a.to.keys + 32 * d);
  tk[0] = k0, tk[1] = k1;
}

// rehash: a lane per slot of the new set claims the first empty cell of its key's probe in the new
// table (cleared by the memset before the move); only atomics touch a cell.
extern "C" __global__ void __launch_bounds__(kThreads) pz_vc_rehash_kernel(VcMoveArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= vc_count(a.nslots, a.to.slot_cap)) return;
  const Hash32 h = vc_load_hash16(a.to.keys + 32 * s);
  uint32_t* table = a.to.table;
  const uint32_t cell = vc_rehash_insert(a.to.cells, h, [table, s](uint32_t c) { return atomicCAS(&table[c], kVcEmpty, (uint32_t)s) == kVcEmpty; });
  if (cell == kVcNone) atomicOr((unsigned long long*)a.err, (unsigned long long)kVcErrCapacity);  // (cells >= 2 * slots: unreachable)
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
  a.bitmaps = static_cast<uint32_t*>(h->bitmaps[h->live].ptr);
  a.totals = static_cast<uint64_t*>(h->totals[h->live].ptr);
  a.keys = static_cast<uint8_t*>(h->keys[h->live].ptr);
  a.table = static_cast<uint32_t*>(h->table[h->live].ptr);
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
  a.table = static_cast<const uint32_t*>(h->table[h->live].ptr);
  a.keys = static_cast<const uint8_t*>(h->keys[h->live].ptr);
  a.nslots = static_cast<const uint32_t*>(h->words2.ptr);
  a.totals = static_cast<const uint64_t*>(h->totals[h->live].ptr);
  a.slot_cap = h->slot_cap, a.cells = h->cells;
  a.hashes = d_hashes, a.n = n, a.out_totals = d_totals, a.out_slots = d_slots;
  h->last = s;
  hipLaunchKernelGGL(pz_vc_lookup_kernel, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_vc_lookup_kernel");
}

// ---- reserve and retain, host side ---------------------------------------------------------------
VcSet set_of(pz_vote_cache* h, int which, uint32_t slot_cap, uint32_t cells) {
  return VcSet{static_cast<uint32_t*>(h->bitmaps[which].ptr), static_cast<uint64_t*>(h->totals[which].ptr),
               static_cast<uint8_t*>(h->keys[which].ptr), static_cast<uint32_t*>(h->table[which].ptr), slot_cap, cells};
}

uint64_t retain_scratch_bytes(uint32_t slot_cap) { return 3 * r16(4ull * slot_cap); }  // flag | new_id | old_of

int check_reserve(const pz_vote_cache* h, uint32_t min_slots) {
  if (!h) return fail(PZ_EINVAL, "vote cache is null");
  if (min_slots > kVcMaxSlotCap) return fail(PZ_EINVAL, "a vote cache of %u slots: above 2^30", min_slots);
  return PZ_OK;
}

int check_retain(const pz_vote_cache* h, const uint8_t* hashes, uint64_t n) {
  if (!h) return fail(PZ_EINVAL, "vote cache is null");
  if (n >= (1ull << 31)) return fail(PZ_EINVAL, "retain: n %llu: 2^31 hashes or more", (unsigned long long)n);
  if (n && !hashes) return fail(PZ_EINVAL, "retain: null hashes");
  return PZ_OK;
}

// The entries into the other buffer set, of new_cap slots, on s; then the sets swap.  retain: only
// the entries whose key is among the n hashes, renumbered (d_scratch: retain_scratch_bytes of the
// cache's slot_cap); else every entry where it was.  An allocation failure leaves the cache as it
// was.  ev (the A/B library's timed entry): seven events around the six steps, a reserve from 3 on.
int enqueue_move(pz_vote_cache* h, uint32_t new_cap, bool retain, const uint8_t* d_hashes, uint64_t n, void* d_scratch,
                 hipStream_t s, Events* ev = nullptr) {
  const uint32_t new_cells = vc_cells(new_cap);
  const int other = h->live ^ 1;
  VcMoveArgs a;
  std::memset(&a, 0, sizeof a);
  a.words = h->words;
  a.per_row = h->words / 4 + 1;
  const uint64_t move_blocks = ((uint64_t)new_cap * a.per_row + kThreads - 1) / kThreads;
  if (move_blocks >= (1ull << 31)) return fail(PZ_EINVAL, "a vote cache of %u slots of %llu words: too large to move", new_cap, (unsigned long long)h->words);
  int rc;
  if ((rc = h->bitmaps[other].reserve((size_t)new_cap * h->words * 4)) || (rc = h->totals[other].reserve((size_t)new_cap * 8)) ||
      (rc = h->keys[other].reserve((size_t)new_cap * 32)) || (rc = h->table[other].reserve((size_t)new_cells * 4)))
    return rc;
  a.from = set_of(h, h->live, h->slot_cap, h->cells);
  a.to = set_of(h, other, new_cap, new_cells);
  a.nslots = static_cast<uint32_t*>(h->words2.ptr);
  a.err = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(h->words2.ptr) + 8);
  hipError_t e;
  h->last = s;
  if (retain) {
    uint8_t* p = static_cast<uint8_t*>(d_scratch);
    const uint64_t part = r16(4ull * h->slot_cap);
    a.flag = reinterpret_cast<uint32_t*>(p);
    a.new_id = reinterpret_cast<uint32_t*>(p + part);
    a.old_of = reinterpret_cast<uint32_t*>(p + 2 * part);
    a.hashes = d_hashes, a.n = n;
    stamp(ev, 0, s);
    if ((e = hipMemsetAsync(a.flag, 0, part, s)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    stamp(ev, 1, s);
    if (n) {
      hipLaunchKernelGGL(pz_vc_keep_kernel, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
      if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_vc_keep_kernel");
    }
    stamp(ev, 2, s);
    hipLaunchKernelGGL(pz_vc_renumber_kernel, dim3(1), dim3(kTile), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_vc_renumber_kernel");
  }
  stamp(ev, 3, s);
  if ((e = hipMemsetAsync(a.to.table, 0xFF, (size_t)new_cells * 4, s)) != hipSuccess) return hip_fail(e, "hipMemsetAsync");
  stamp(ev, 4, s);
  hipLaunchKernelGGL(pz_vc_move_kernel, dim3((uint32_t)move_blocks), dim3(kThreads), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_vc_move_kernel");
  stamp(ev, 5, s);
  hipLaunchKernelGGL(pz_vc_rehash_kernel, dim3((new_cap + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_vc_rehash_kernel");
  stamp(ev, 6, s);
  h->live = other, h->slot_cap = new_cap, h->cells = new_cells;
  return PZ_OK;
}

}  // namespace

int vote_cache_view(pz_vote_cache* h, VcView* v, hipStream_t s) {
  if (!h || !v) return fail(PZ_EINVAL, "vote cache is null");
  std::lock_guard<std::mutex> lk(h->mu);
  v->device = h->device;
  v->nval = h->nval;
  v->slot_cap = h->slot_cap, v->cells = h->cells;
  v->table = static_cast<const uint32_t*>(h->table[h->live].ptr);
  v->keys = static_cast<const uint8_t*>(h->keys[h->live].ptr);
  v->nslots = static_cast<const uint32_t*>(h->words2.ptr);
  v->totals = static_cast<const uint64_t*>(h->totals[h->live].ptr);
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
  if ((rc = h->bitmaps[0].fill(bm, 0, what)) || (rc = h->totals[0].fill((size_t)slot_cap * 8, 0, what)) ||
      (rc = h->keys[0].fill((size_t)slot_cap * 32, 0, what)) || (rc = h->table[0].fill((size_t)h->cells * 4, 0xFF, what)) ||
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

int pz_vote_cache_capacity(pz_vote_cache* h, uint32_t* slot_cap) {
  if (!h || !slot_cap) return fail(PZ_EINVAL, "vote cache / slot_cap is null");
  std::lock_guard<std::mutex> lk(h->mu);
  *slot_cap = h->slot_cap;
  return PZ_OK;
}

int pz_dev_vote_cache_reserve(pz_vote_cache* h, uint32_t min_slots, void* stream) {
  int rc = check_reserve(h, min_slots);
  if (rc) return rc;
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (min_slots <= h->slot_cap) return PZ_OK;
  return enqueue_move(h, min_slots, false, nullptr, 0, nullptr, static_cast<hipStream_t>(stream));
}

int pz_vote_cache_reserve(pz_vote_cache* h, uint32_t min_slots) {
  int rc = check_reserve(h, min_slots);
  if (rc) return rc;
  HostForm f(h, "vote cache reserve");
  if (f.rc) return f.rc;
  if (min_slots <= h->slot_cap) return PZ_OK;
  if ((rc = enqueue_move(h, min_slots, false, nullptr, 0, nullptr, f.st.s))) return rc;
  return f.st.sync();
}

uint64_t pz_vote_cache_retain_scratch_bytes(uint32_t slot_cap, uint64_t n) {
  (void)n;  // (the keep-hashes are read where they lie)
  return retain_scratch_bytes(slot_cap);
}

int pz_dev_vote_cache_retain(pz_vote_cache* h, const uint8_t* d_hashes, uint64_t n, void* d_scratch, void* stream) {
  int rc = check_retain(h, d_hashes, n);
  if (rc) return rc;
  if (n && !aligned16(d_hashes)) return fail(PZ_EINVAL, "retain: hashes must be a 16-B aligned device pointer");
  if (!d_scratch || !aligned16(d_scratch)) return fail(PZ_EINVAL, "d_scratch must be a 16-B aligned device pointer");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  return enqueue_move(h, h->slot_cap, true, d_hashes, n, d_scratch, static_cast<hipStream_t>(stream));
}

int pz_vote_cache_retain(pz_vote_cache* h, const uint8_t* hashes, uint64_t n) {
  int rc = check_retain(h, hashes, n);
  if (rc) return rc;
  HostForm f(h, "vote cache retain");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  const uint8_t* d_hashes = n ? st.up(hashes, n * 32) : nullptr;
  uint8_t* scr = st.up<uint8_t>(nullptr, retain_scratch_bytes(h->slot_cap));
  if (st.rc) return st.rc;
  if ((rc = enqueue_move(h, h->slot_cap, true, d_hashes, n, scr, st.s))) return rc;
  return st.sync();
}

#ifdef PZ_AB_BUILD
// (tools/votecache_retain_probe.py) pz_dev_vote_cache_retain (retain != 0) or pz_dev_vote_cache_reserve
// with one event pair per step; synchronises and returns the steps' milliseconds in ms[0..6): the
// flags' memset, keep, renumber (a reserve: zeros), the table's memset, move, rehash.
int pz_debug_vote_cache_move_timed(pz_vote_cache* h, uint32_t min_slots, int retain, const uint8_t* d_hashes, uint64_t n,
                                   void* d_scratch, void* stream, float ms[6]) {
  int rc = retain ? check_retain(h, d_hashes, n) : check_reserve(h, min_slots);
  if (rc) return rc;
  if (!ms || (retain && !d_scratch) || (!retain && min_slots <= h->slot_cap)) return fail(PZ_EINVAL, "timed move: nothing to time");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  Events ev;
  if ((rc = ev.create(7))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int k = 0; k < 6; ++k) ms[k] = 0;
  rc = enqueue_move(h, retain ? h->slot_cap : min_slots, retain != 0, d_hashes, n, d_scratch, s, &ev);
  const int first = retain ? 0 : 3;
  static const int pairs[6] = {0, 1, 2, 3, 4, 5};
  return ev.elapsed(rc, ms + first, pairs + first, 6 - first, s, "timed vote cache move");
}
#endif

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
    if (hashes) e = hipMemcpy(hashes, h->keys[h->live].ptr, (size_t)ns * 32, hipMemcpyDeviceToHost);
    if (e == hipSuccess && totals) e = hipMemcpy(totals, h->totals[h->live].ptr, (size_t)ns * 8, hipMemcpyDeviceToHost);
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
  hipError_t e = ns ? hipMemcpy(keys.data(), h->keys[h->live].ptr, keys.size(), hipMemcpyDeviceToHost) : hipSuccess;
  if (e != hipSuccess) return hip_fail(e, "vote cache voters");
  *present = 0;
  uint32_t slot = 0;
  for (; slot < ns; ++slot)
    if (!std::memcmp(keys.data() + 32ull * slot, hash, 32)) break;
  if (slot < ns) {
    *present = 1;
    if (words) e = hipMemcpy(words, static_cast<uint32_t*>(h->bitmaps[h->live].ptr) + (size_t)slot * h->words, h->words * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "vote cache voters");
  } else if (words) {
    std::memset(words, 0, h->words * 4);
  }
  return report(sticky);
}

}  // extern "C"
