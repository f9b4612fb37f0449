// ActiveState.PendingAttestations resident on one device, for gfx950.
//
// The attestations a block contributes (processedAttestations, blockchain/service.go:280-301)
// become pending attestations (NewPendingAttestation, computeNewActiveState, core.go:223-237) and
// stay until stateRecalc drops those of slots up to lastStateRecalc (core.go:444-450).  The handle
// owns them as the full pz_attestation_cols column set plus `committee` (the checks' committee id)
// and `shard32` (shard_id saturated to u32): what the epoch kernels read as bits / boffs / att_comm
// / att_shard, what pz_dev_wire_attestations(field_num = 1) encodes into the stored ActiveState,
// and what a crosslink winner's ShardBlockHash is read from -- all in place.
//
// Append and prune are one operation: an order-preserving selection of rows of a column set into
// another column set at a base.  Each is four dependent launches on the caller's stream, in the
// decoder's reduce-then-scan shape (tile_scan.h); no workgroup waits for another, nothing spins,
// nothing looks back: every cross-workgroup fact travels through a launch boundary.
//   1 size    a lane per row, 256 rows per tile: the keep predicate and the row's seven sizes
//             (attpool_dev.h), the tile's seven sums.
//   2 scan    pz_unwire_scan_kernel with ncols = 7: the tiles' bases and the call's totals.
//   3 commit  one lane: snapshots the pool's seven counts as the call's base, decides
//             base + total <= cap for all seven, and either advances the counts or marks the call
//             void and sets the sticky capacity bit.  A call lands whole or not at all.
//   4 write   scans the tile's sizes again, adds the tile's base and the call's base: the five
//             offsets columns are written once; scalars, committee, shard32, the bytes ranges, the
//             element offsets (rebased) and the sig values are copied.  A range up to kApLongBytes
//             goes lane by lane (copy_span); a longer one is copied by its whole wave.  A void call
//             writes nothing.
// A prune selects from the live buffer set into the other one at base 0, then the sets swap.
//
// The capacities grow as the Go slice does under append (core.go:223-237; types/state.go:169):
// pz_[dev_]att_pool_reserve grows the other buffer set to max(cap, min_caps) and ONE launch,
// pz_att_pool_move_kernel, copies the live prefix of every column there -- the seven counts are read
// on the device, the host knows only the capacities -- then the sets swap.  The set left behind
// keeps its buffers, so a kernel queued over a view still reads valid memory; it grows when a prune
// or a reserve next writes into it (DevBuf::reserve, a no-op while it is large enough).
// pz_[dev_]att_pool_need is the size and scan launches of an append without its commit: the seven
// sums a landing would add, for up to two take columns.
//
// Reads: only the rows' ranges of the source columns.  Writes: only inside the ranges the scan
// assigns, which the commit has checked against the capacities.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "att_cols.h"
#include "attpool_dev.h"
#include "resident.h"
#include "tile_scan.h"

namespace pz {
namespace {

constexpr int kSetBufs = kApSetBufs;  // pz_attestation_cols' columns (att_cols.h's order), committee, shard32

}  // namespace
}  // namespace pz

struct pz_att_pool : pz::Resident {  // (last: counts / read wait for it)
  uint64_t cap[pz::kApCols] = {};
  uint64_t rows_ub = 0;        // an upper bound of the rows held (a prune's grid; exact after counts)
  int live = 0;                // which buffer set holds the rows
  pz::DevBuf set[2][pz::kSetBufs];
  pz::DevBuf words;    // counts[7], then the sticky error word
  pz::DevBuf scratch;  // a prune's scratch (sized for cap[0] rows)
  ~pz_att_pool() {
    drain();
    for (auto& s : set)
      for (pz::DevBuf& b : s) b.release();
    words.release();
    scratch.release();
  }
};

namespace pz {
namespace {

// What one call leaves for its write launch (commit writes it).
struct ApCall {
  uint64_t base[kApCols];
  uint64_t n;        // source rows
  uint64_t is_void;  // the call did not fit: nothing is written
};

struct ApDst {
  pz_attestation_cols_out c;  // (n_oblique, last_byte and status unused)
  uint32_t* committee;
  uint32_t* shard32;
};

struct ApArgs {
  pz_attestation_cols src;
  const uint32_t* src_committee;
  const uint32_t* src_shard32;  // prune; an append derives it from shard_id
  const int32_t* status;        // append's predicate
  const uint8_t* take;
  uint64_t last_state_recalc;  // prune's predicate
  uint32_t prune;
  uint64_t n;  // append: the batch's rows; prune: the host's upper bound (the count is on the device)
  uint64_t ntiles;
  ApDst dst;
  uint64_t cap[kApCols];
  uint64_t* counts;  // [7], the error word at [7]
  uint64_t* tiles;   // [7][ntiles]
  uint64_t* totals;  // [7]
  ApCall* call;
  uint64_t long_bytes;
};

uint64_t g_long_bytes = kApLongBytes;  // (the A/B library's probe varies it)

__device__ __forceinline__ bool ap_keep(const ApArgs& a, uint64_t i) {
  if (a.prune) return ap_keep_prune(a.src.slot[i], a.last_state_recalc);
  return ap_keep_append(a.status, a.take, i);
}

// ---- 1: size -----------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kTile) pz_att_pool_size_kernel(ApArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  const uint64_t n = a.prune ? a.counts[kApRows] : a.n;
  uint64_t sz[kApCols];
  if (ap_kept_sizes(i < n && ap_keep(a, i), a.src, i, sz))
    atomicOr((unsigned long long*)(a.counts + kApCols), (unsigned long long)kApErrInverted);
  tile_sums<kApCols>(sz, a.tiles, a.ntiles);
}

// ---- need: the size phase of an append for two take columns, no pool --------------------------
struct ApNeedArgs {
  pz_attestation_cols src;
  const int32_t* status;
  const uint8_t* take[2];
  uint64_t n, ntiles;
  uint64_t* tiles;  // [2][7][ntiles]: fourteen columns for the scan
};

extern "C" __global__ void __launch_bounds__(kTile) pz_att_pool_need_kernel(ApNeedArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  const uint32_t k = blockIdx.y;
  uint64_t sz[kApCols];
  (void)ap_kept_sizes(i < a.n && ap_keep_append(a.status, a.take[k], i), a.src, i, sz);
  tile_sums<kApCols>(sz, a.tiles + (uint64_t)k * kApCols * a.ntiles, a.ntiles);
}

// ---- move: every column's live prefix into the grown buffer set -----------------------------------
struct ApMoveArgs {
  const uint8_t* src[kSetBufs];
  uint8_t* dst[kSetBufs];
  ApColRule rule[kSetBufs];
  uint64_t cap[kApCols];   // the capacities the source set was filled under: a count never exceeds its own
  const uint64_t* counts;  // [7], on the device
};

// A row of workgroups per buffer (blockIdx.y), a grid-wide lane index along it: the sixteen columns'
// round trips overlap instead of queueing behind each other.  Plain loads and stores, no workgroup
// waits for another.  The governing count is clamped to the old capacity, so no access leaves
// either buffer set whatever the words hold.
extern "C" __global__ void __launch_bounds__(kTile) pz_att_pool_move_kernel(ApMoveArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * kTile + threadIdx.x, T = (uint64_t)gridDim.x * kTile;
  const uint32_t k = blockIdx.y;
  const ApColRule r = a.rule[k];
  const uint64_t n = a.counts[r.count], cap = a.cap[r.count];
  ap_move_lane(a.dst[k], a.src[k], ap_col_live_bytes(r, n < cap ? n : cap), t, T);
}

// ---- 3: commit (one lane) --------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64) pz_att_pool_commit_kernel(ApArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint64_t base[kApCols], total[kApCols];
  const uint64_t rows = a.counts[kApRows];
#pragma unroll
  for (int c = 0; c < kApCols; ++c) {
    base[c] = a.prune ? 0 : a.counts[c];
    total[c] = a.totals[c];
  }
  const bool fits = ap_fits(base, total, a.cap);
#pragma unroll
  for (int c = 0; c < kApCols; ++c) {
    a.call->base[c] = base[c];
    if (fits) a.counts[c] = base[c] + total[c];
  }
  a.call->n = a.prune ? rows : a.n;
  a.call->is_void = !fits;
  if (!fits) atomicOr((unsigned long long*)(a.counts + kApCols), (unsigned long long)kApErrCapacity);
}

// ---- 4: write --------------------------------------------------------------------------------
// The wave copies the long ranges of its lanes one after another: lane q's (dst, src, len) goes
// wave-wide, every lane moves 16 unaligned bytes a step, and the tail is the last 16 bytes again
// (len > long_bytes >= 16: every access lies inside the range).  Every lane of the wave calls.
__device__ __forceinline__ void wave_copy_long(bool mine, uint8_t* dst, const uint8_t* src, uint64_t len) {
  const uint32_t lane = threadIdx.x & 63;
  uint64_t m = __ballot(mine);
  while (m) {  // (wave-uniform)
    const int q = __builtin_ctzll(m);
    m &= m - 1;
    gbyte* o = reinterpret_cast<gbyte*>((uintptr_t)__shfl((uint64_t)(uintptr_t)dst, q, 64));
    const gbyte* s = reinterpret_cast<const gbyte*>((uintptr_t)__shfl((uint64_t)(uintptr_t)src, q, 64));
    const uint64_t len_q = __shfl(len, q, 64);
    constexpr uint64_t kStep = 64 * 16;  // the wave's bytes a step
    uint64_t k = (uint64_t)lane * 16;
    for (; k + 3 * kStep + 16 <= len_q; k += 4 * kStep) {  // four loads in flight before the stores
      uint4 v0, v1, v2, v3;  // (named: an array here is promoted to LDS)
      __builtin_memcpy(&v0, s + k, 16);
      __builtin_memcpy(&v1, s + k + kStep, 16);
      __builtin_memcpy(&v2, s + k + 2 * kStep, 16);
      __builtin_memcpy(&v3, s + k + 3 * kStep, 16);
      __builtin_memcpy(o + k, &v0, 16);
      __builtin_memcpy(o + k + kStep, &v1, 16);
      __builtin_memcpy(o + k + 2 * kStep, &v2, 16);
      __builtin_memcpy(o + k + 3 * kStep, &v3, 16);
    }
    for (; k + 16 <= len_q; k += kStep) copy16(o + k, s + k);
    if (lane == 0 && (len_q & 15)) copy16(o + len_q - 16, s + len_q - 16);
  }
}

extern "C" __global__ void __launch_bounds__(kTile) pz_att_pool_write_kernel(ApArgs a) {
  if (a.call->is_void) return;  // (grid-uniform)
  const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  const bool keep = i < a.call->n && ap_keep(a, i);
  ApRow r;
#pragma unroll
  for (int c = 0; c < kApCols; ++c) r.sz[c] = 0, r.lo[c] = 0;
  r.inverted = false;
  if (keep) r = ap_row(a.src, i);
  uint64_t at[kApCols];
  tile_excl<kApCols>(r.sz, at);
#pragma unroll
  for (int c = 0; c < kApCols; ++c) at[c] += a.tiles[c * a.ntiles + blockIdx.x] + a.call->base[c];

  const ApDst& d = a.dst;
  if (i == 0) {  // the ends of the offsets columns: the pool's new counts
    uint64_t end[kApCols];
#pragma unroll
    for (int c = 0; c < kApCols; ++c) end[c] = a.call->base[c] + a.totals[c];
    d.c.justified_block_hash_offs[end[kApRows]] = end[kApJbh];
    d.c.shard_block_hash_offs[end[kApRows]] = end[kApSbh];
    d.c.attester_bitfield_offs[end[kApRows]] = end[kApBits];
    d.c.oblique_first[end[kApRows]] = end[kApElems];
    d.c.oblique_offs[end[kApElems]] = end[kApElemBytes];
    d.c.aggregate_sig_first[end[kApRows]] = end[kApSigs];
  }

  // the row's five ranges as (dst, src, bytes)
  uint8_t* dp[5] = {d.c.justified_block_hash + at[kApJbh], d.c.shard_block_hash + at[kApSbh],
                    d.c.attester_bitfield + at[kApBits], d.c.oblique_parent_hashes + at[kApElemBytes],
                    reinterpret_cast<uint8_t*>(d.c.aggregate_sig + at[kApSigs])};
  const uint8_t* sp[5] = {a.src.justified_block_hash + r.lo[kApJbh], a.src.shard_block_hash + r.lo[kApSbh],
                          a.src.attester_bitfield + r.lo[kApBits], a.src.oblique_parent_hashes + r.lo[kApElemBytes],
                          reinterpret_cast<const uint8_t*>(a.src.aggregate_sig + r.lo[kApSigs])};
  const uint64_t len[5] = {r.sz[kApJbh], r.sz[kApSbh], r.sz[kApBits], r.sz[kApElemBytes], r.sz[kApSigs] * 8};

  if (keep) {
    const uint64_t row = at[kApRows];
    const bool z = r.inverted;
    const uint64_t shard = (!z && a.src.shard_id) ? a.src.shard_id[i] : 0;
    d.c.slot[row] = (!z && a.src.slot) ? a.src.slot[i] : 0;
    d.c.shard_id[row] = shard;
    d.c.justified_slot[row] = (!z && a.src.justified_slot) ? a.src.justified_slot[i] : 0;
    d.committee[row] = z ? 0xFFFFFFFFu : a.src_committee[i];
    d.shard32[row] = (a.src_shard32 && !z) ? a.src_shard32[i] : ap_shard32(shard);
    d.c.justified_block_hash_offs[row] = at[kApJbh];
    d.c.shard_block_hash_offs[row] = at[kApSbh];
    d.c.attester_bitfield_offs[row] = at[kApBits];
    d.c.oblique_first[row] = at[kApElems];
    d.c.aggregate_sig_first[row] = at[kApSigs];
    for (uint64_t k = 0; k < r.sz[kApElems]; ++k)  // the element CSR, rebased
      d.c.oblique_offs[at[kApElems] + k] = at[kApElemBytes] + (a.src.oblique_offs[r.lo[kApElems] + k] - r.lo[kApElemBytes]);
#pragma unroll
    for (int c = 0; c < 5; ++c)
      if (len[c] <= a.long_bytes) copy_span(dp[c], sp[c], len[c]);
  }
#pragma unroll
  for (int c = 0; c < 5; ++c) wave_copy_long(keep && len[c] > a.long_bytes, dp[c], sp[c], len[c]);
}

// ---- host side ---------------------------------------------------------------------------------
uint64_t scratch_bytes(uint64_t n) { return pad256((kApCols * tiles_of(n) + kApCols + sizeof(ApCall) / 8) * 8); }

// Bytes of buffer k of a set: a column at its capacity (cap[1..] are att_cols.h's totals), a bytes
// column with the digest kernels' 4 readable bytes and the 16-byte pieces' room, the sig values
// with one entry's; committee, shard32.
uint64_t buf_bytes(const uint64_t cap[kApCols], int k) {
  if (k >= kAttNCols) return cap[kApRows] * 4;
  const AttCol& c = kAttTable[k];
  const uint64_t room = c.total < 0 || c.plus ? 0 : c.width == 1 ? 16 : 1;
  return (att_col_len(c, cap[kApRows], cap + 1) + room) * c.width;
}

ApDst set_dst(pz_att_pool* h, int s) {
  ApDst d{};
  pz::DevBuf* b = h->set[s];
  for (int k = 0; k < kAttNCols; ++k) att_set_out(&d.c, k, b[k].ptr);
  d.committee = (uint32_t*)b[kAttNCols].ptr, d.shard32 = (uint32_t*)b[kAttNCols + 1].ptr;
  return d;
}

pz_attestation_cols as_cols(const ApDst& d) {
  pz_attestation_cols c{};
  for (int k = 0; k < kAttNCols; ++k) att_set_in(&c, k, att_out(d.c, k));
  return c;
}

// What can be told about an append without reading a column; 1: nothing to do.
int check_append(const pz_att_pool* h, const pz_attestation_cols* a, uint64_t n, const int32_t* status,
                 const uint32_t* committee) {
  if (!h) return fail(PZ_EINVAL, "attestation pool is null");
  if (n == 0) return 1;
  if (!a) return fail(PZ_EINVAL, "columns are null");
  if (!status || !committee) return fail(PZ_EINVAL, "append: null status / committee");
  if ((a->justified_block_hash_offs && !a->justified_block_hash) || (a->shard_block_hash_offs && !a->shard_block_hash) ||
      (a->attester_bitfield_offs && !a->attester_bitfield) ||
      (a->oblique_first && (!a->oblique_offs || !a->oblique_parent_hashes)) || (a->aggregate_sig_first && !a->aggregate_sig))
    return fail(PZ_EINVAL, "offsets without their data column");
  if (n >> 38) return fail(PZ_EINVAL, "more than 2^38 rows");  // (a tile per workgroup: the grid's limit)
  return PZ_OK;
}

// The four launches on s.  scratch: tiles, totals, the call record.  ev (the A/B library's timed
// entry; null in the product): five events, one before the first launch and one after each.
int enqueue(pz_att_pool* h, ApArgs a, void* d_scratch, hipStream_t s, Events* ev = nullptr) {
  a.ntiles = tiles_of(a.n);
  std::memcpy(a.cap, h->cap, sizeof a.cap);
  a.counts = static_cast<uint64_t*>(h->words.ptr);
  a.tiles = static_cast<uint64_t*>(d_scratch);
  a.totals = a.tiles + kApCols * a.ntiles;
  a.call = reinterpret_cast<ApCall*>(a.totals + kApCols);
  a.long_bytes = g_long_bytes;
  h->last = s;
  hipError_t e;
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_att_pool_size_kernel, dim3((uint32_t)a.ntiles), dim3(kTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_att_pool_size_kernel");
  stamp(ev, 1, s);
  if ((e = launch_tile_scan(a.tiles, a.ntiles, (uint32_t)kApCols, a.totals, s)) != hipSuccess)
    return hip_fail(e, "pz_unwire_scan_kernel");
  stamp(ev, 2, s);
  hipLaunchKernelGGL(pz_att_pool_commit_kernel, dim3(1), dim3(64), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_att_pool_commit_kernel");
  stamp(ev, 3, s);
  hipLaunchKernelGGL(pz_att_pool_write_kernel, dim3((uint32_t)a.ntiles), dim3(kTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_att_pool_write_kernel");
  stamp(ev, 4, s);
  return PZ_OK;
}

ApArgs append_args(pz_att_pool* h, const pz_attestation_cols& a, uint64_t n, const int32_t* status,
                   const uint32_t* committee, const uint8_t* take) {
  ApArgs g;
  std::memset(&g, 0, sizeof g);
  g.src = a;
  g.src_committee = committee;
  g.status = status;
  g.take = take;
  g.n = n;
  g.dst = set_dst(h, h->live);
  return g;
}

ApArgs prune_args(pz_att_pool* h, uint64_t last_state_recalc) {
  ApArgs g;
  std::memset(&g, 0, sizeof g);
  const ApDst from = set_dst(h, h->live);
  g.src = as_cols(from);
  g.src_committee = from.committee;
  g.src_shard32 = from.shard32;
  g.prune = 1;
  g.last_state_recalc = last_state_recalc;
  g.n = h->rows_ub;
  g.dst = set_dst(h, h->live ^ 1);
  return g;
}

// Waits for the last call and reads the counts and the sticky error word; the code to report.
int settle(pz_att_pool* h, uint64_t counts[kApCols], int* sticky) {
  uint64_t w[kApCols + 1] = {};
  int rc = h->settle(w, h->words, sizeof w, "attestation pool read");
  if (rc) return rc;
  std::memcpy(counts, w, kApCols * 8);
  h->rows_ub = w[kApRows];
  *sticky = (w[kApCols] & kApErrInverted) ? PZ_EINVAL : (w[kApCols] & kApErrCapacity) ? PZ_ERANGE : PZ_OK;
  return PZ_OK;
}

int report(int sticky) {
  if (sticky == PZ_EINVAL) return fail(PZ_EINVAL, "an appended row had an inverted range; it landed empty");
  if (sticky == PZ_ERANGE) return fail(PZ_ERANGE, "an append needed more than the pool holds; it was dropped whole");
  return PZ_OK;
}

// ---- reserve and need, host side ---------------------------------------------------------------
// Set s's buffers hold at least `cap` (grow-only, buffer by buffer: nothing happens where they do).
int grow_set(pz_att_pool* h, int s, const uint64_t cap[kApCols]) {
  int rc = PZ_OK;
  for (int k = 0; k < kSetBufs && !rc; ++k) rc = h->set[s][k].reserve((size_t)buf_bytes(cap, k));
  return rc;
}

int check_reserve(const pz_att_pool* h, const uint64_t* min_caps) {
  if (!h) return fail(PZ_EINVAL, "attestation pool is null");
  if (!min_caps) return fail(PZ_EINVAL, "min_caps is null");
  for (int c = 0; c < kApCols; ++c)
    if (min_caps[c] >> 40) return fail(PZ_EINVAL, "capacity %d is %llu: 2^40 or more", c, (unsigned long long)min_caps[c]);
  return PZ_OK;
}

// The live prefixes into the other set, grown to new_cap, on s; then the sets swap.  An allocation
// failure leaves the pool as it was (the other set holds no rows).  ev (the A/B library's timed
// entry): one event pair around the launch.
int enqueue_reserve(pz_att_pool* h, const uint64_t new_cap[kApCols], hipStream_t s, Events* ev = nullptr) {
  const int other = h->live ^ 1;
  int rc;
  if ((rc = grow_set(h, other, new_cap)) || (rc = h->scratch.reserve(scratch_bytes(new_cap[kApRows])))) return rc;
  ApMoveArgs a;
  std::memset(&a, 0, sizeof a);
  uint64_t most = 0;  // the largest column's bytes at the old capacities: the grid
  for (int k = 0; k < kSetBufs; ++k) {
    a.src[k] = static_cast<const uint8_t*>(h->set[h->live][k].ptr);
    a.dst[k] = static_cast<uint8_t*>(h->set[other][k].ptr);
    a.rule[k] = ap_col_rule(k);
    most = std::max(most, ap_col_live_bytes(a.rule[k], h->cap));
  }
  std::memcpy(a.cap, h->cap, sizeof a.cap);
  a.counts = static_cast<const uint64_t*>(h->words.ptr);
  const uint64_t blocks = std::min<uint64_t>(std::max<uint64_t>((most + kTile * 64 - 1) / (kTile * 64), 1), 1024);
  h->last = s;
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_att_pool_move_kernel, dim3((uint32_t)blocks, kSetBufs), dim3(kTile), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "pz_att_pool_move_kernel");
  stamp(ev, 1, s);
  h->live = other;
  std::memcpy(h->cap, new_cap, sizeof h->cap);
  return PZ_OK;
}

uint64_t need_scratch_bytes(uint64_t n) { return pad256(2 * kApCols * tiles_of(n) * 8 + 16); }

// What can be told about a need call without reading a column; 1: nothing to count.
int check_need(const pz_attestation_cols* a, uint64_t n, const int32_t* status) {
  if (n == 0) return 1;
  if (!a) return fail(PZ_EINVAL, "columns are null");
  if (!status) return fail(PZ_EINVAL, "need: null status");
  if ((a->justified_block_hash_offs && !a->justified_block_hash) || (a->shard_block_hash_offs && !a->shard_block_hash) ||
      (a->attester_bitfield_offs && !a->attester_bitfield) ||
      (a->oblique_first && (!a->oblique_offs || !a->oblique_parent_hashes)) || (a->aggregate_sig_first && !a->aggregate_sig))
    return fail(PZ_EINVAL, "offsets without their data column");
  if (n >> 38) return fail(PZ_EINVAL, "more than 2^38 rows");
  return PZ_OK;
}

// The two launches on s (n > 0); d_need: [2][7].  ev: three events, one before the first launch and
// one after each.
int enqueue_need(const pz_attestation_cols& cols, uint64_t n, const int32_t* status, const uint8_t* take0,
                 const uint8_t* take1, uint64_t* d_need, void* d_scratch, hipStream_t s, Events* ev = nullptr) {
  ApNeedArgs a;
  std::memset(&a, 0, sizeof a);
  a.src = cols;
  a.status = status;
  a.take[0] = take0, a.take[1] = take1;
  a.n = n, a.ntiles = tiles_of(n);
  a.tiles = static_cast<uint64_t*>(d_scratch);
  hipError_t e;
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_att_pool_need_kernel, dim3((uint32_t)a.ntiles, 2), dim3(kTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_att_pool_need_kernel");
  stamp(ev, 1, s);
  if ((e = launch_tile_scan(a.tiles, a.ntiles, 2u * kApCols, d_need, s)) != hipSuccess) return hip_fail(e, "pz_unwire_scan_kernel");
  stamp(ev, 2, s);
  return PZ_OK;
}

}  // namespace

int att_pool_peek(pz_att_pool* h, ApView* v, hipStream_t s) {
  if (!h || !v) return fail(PZ_EINVAL, "attestation pool is null");
  std::lock_guard<std::mutex> lk(h->mu);
  const ApDst d = set_dst(h, h->live);
  v->device = h->device;
  v->rows_cap = h->cap[kApRows];
  v->rows_ub = h->rows_ub;
  v->cols = as_cols(d);
  v->committee = d.committee;
  v->shard32 = d.shard32;
  v->counts = static_cast<const uint64_t*>(h->words.ptr);
  h->last = s;
  return PZ_OK;
}

Resident* resident_of(pz_att_pool* h) { return h; }

void att_pool_note_rows(pz_att_pool* h, uint64_t rows) {
  std::lock_guard<std::mutex> lk(h->mu);
  h->rows_ub = rows;
}

}  // namespace pz

using namespace pz;

extern "C" {

int pz_att_pool_new(const uint64_t caps[7], int device, pz_att_pool** out) {
  if (!out) return fail(PZ_EINVAL, "out is null");
  *out = nullptr;
  if (!caps) return fail(PZ_EINVAL, "caps is null");
  if (caps[kApRows] == 0) return fail(PZ_EINVAL, "an attestation pool of zero rows");
  for (int c = 0; c < kApCols; ++c)
    if (caps[c] >> 40) return fail(PZ_EINVAL, "capacity %d is %llu: 2^40 or more", c, (unsigned long long)caps[c]);
  int rc = Resident::open(device);
  if (rc) return rc;
  hipError_t e;
  auto* h = new pz_att_pool();
  h->device = device;
  std::memcpy(h->cap, caps, sizeof h->cap);
  const char* what = "attestation pool init";
  for (int k = 0; k < 2 * kSetBufs && !rc; ++k) rc = h->set[k / kSetBufs][k % kSetBufs].fill((size_t)buf_bytes(caps, k % kSetBufs), 0, what);
  if (!rc) rc = h->words.fill((kApCols + 1) * 8, 0, what);
  if (!rc) rc = h->scratch.reserve(scratch_bytes(caps[kApRows]));
  if (!rc && (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(e, what);
  if (rc) {
    delete h;
    return rc;
  }
  *out = h;
  return PZ_OK;
}

void pz_att_pool_free(pz_att_pool* h) { delete h; }

uint64_t pz_att_pool_scratch_bytes(uint64_t n) { return scratch_bytes(n); }

int pz_dev_att_pool_append(pz_att_pool* h, const pz_attestation_cols* a, uint64_t n, const int32_t* status,
                           const uint32_t* committee, const uint8_t* take, void* d_scratch, void* stream) {
  int rc = check_append(h, a, n, status, committee);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!d_scratch || !aligned16(d_scratch)) return fail(PZ_EINVAL, "d_scratch must be a 16-B aligned device pointer");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if ((rc = enqueue(h, append_args(h, *a, n, status, committee, take), d_scratch, static_cast<hipStream_t>(stream)))) return rc;
  h->rows_ub = std::min(h->cap[kApRows], h->rows_ub + n);
  return PZ_OK;
}

int pz_att_pool_append(pz_att_pool* h, const pz_attestation_cols* ha, uint64_t n, const int32_t* status,
                       const uint32_t* committee, const uint8_t* take) {
  int rc = check_append(h, ha, n, status, committee);
  if (rc) return rc < 0 ? rc : PZ_OK;
  HostForm f(h, "attestation pool append");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_attestation_cols d;
  stage_att_cols(st, *ha, n, kAttAllCols, &d);
  const int32_t* d_status = st.up(status, n);
  const uint32_t* d_comm = st.up(committee, n);
  const uint8_t* d_take = take ? st.up(take, n) : nullptr;
  uint8_t* scr = st.up<uint8_t>(nullptr, scratch_bytes(n));
  if (st.rc) return st.rc;
  if ((rc = enqueue(h, append_args(h, d, n, d_status, d_comm, d_take), scr, st.s))) return rc;
  h->rows_ub = std::min(h->cap[kApRows], h->rows_ub + n);
  return st.sync();
}

int pz_dev_att_pool_prune(pz_att_pool* h, uint64_t last_state_recalc, void* stream) {
  if (!h) return fail(PZ_EINVAL, "attestation pool is null");
  int rc = h->use();
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->rows_ub == 0) return PZ_OK;  // nothing was ever appended since the last exact count of 0
  if ((rc = grow_set(h, h->live ^ 1, h->cap))) return rc;  // (the set a reserve left behind: it grows here)
  if ((rc = enqueue(h, prune_args(h, last_state_recalc), h->scratch.ptr, static_cast<hipStream_t>(stream)))) return rc;
  h->live ^= 1;
  return PZ_OK;
}

int pz_att_pool_counts(pz_att_pool* h, uint64_t counts[7]) {
  if (!h || !counts) return fail(PZ_EINVAL, "attestation pool / counts is null");
  int rc = h->use();
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  int sticky;
  if ((rc = settle(h, counts, &sticky))) return rc;
  return report(sticky);
}

int pz_att_pool_view(pz_att_pool* h, pz_attestation_cols* cols, const uint32_t** committee, const uint32_t** shard32) {
  if (!h) return fail(PZ_EINVAL, "attestation pool is null");
  std::lock_guard<std::mutex> lk(h->mu);
  const ApDst d = set_dst(h, h->live);
  if (cols) *cols = as_cols(d);
  if (committee) *committee = d.committee;
  if (shard32) *shard32 = d.shard32;
  return PZ_OK;
}

int pz_att_pool_read(pz_att_pool* h, const pz_attestation_cols_out* out, uint32_t* committee, const uint64_t caps[6]) {
  if (!h || !out || !caps) return fail(PZ_EINVAL, "attestation pool / out / caps is null");
  int rc = h->use();
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  uint64_t n[kApCols];
  int sticky;
  if ((rc = settle(h, n, &sticky))) return rc;
  for (int c = 0; c < kAttTotals; ++c)
    if (n[c + 1] > caps[c])
      return fail(PZ_ERANGE, "%s holds %llu, capacity %llu", att_total_name(c), (unsigned long long)n[c + 1],
                  (unsigned long long)caps[c]);
  const ApDst d = set_dst(h, h->live);
  for (int k = 0; k < kAttNCols; ++k) {
    const uint64_t bytes = att_col_len(kAttTable[k], n[kApRows], n + 1) * kAttTable[k].width;
    if ((rc = down(static_cast<uint8_t*>(att_out(*out, k)), att_out(d.c, k), bytes, "attestation pool read"))) return rc;
  }
  if ((rc = down(committee, d.committee, n[kApRows], "attestation pool read"))) return rc;
  return report(sticky);
}

int pz_att_pool_shard_block_hashes(pz_att_pool* h, const uint32_t* rows, uint64_t nrows, uint8_t* out, uint64_t cap,
                                   uint64_t* offs) {
  if (!h || !offs || (nrows && !rows)) return fail(PZ_EINVAL, "attestation pool / rows / offs is null");
  int rc = h->use();
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  uint64_t n[kApCols];
  int sticky;
  if ((rc = settle(h, n, &sticky))) return rc;
  const ApDst d = set_dst(h, h->live);
  std::vector<uint64_t> so(n[kApRows] + 1);
  std::vector<uint8_t> sb(n[kApSbh]);
  if ((rc = down(so.data(), d.c.shard_block_hash_offs, so.size(), "attestation pool read")) ||
      (rc = down(sb.data(), d.c.shard_block_hash, sb.size(), "attestation pool read")))
    return rc;
  offs[0] = 0;
  for (uint64_t k = 0; k < nrows; ++k) {
    if (rows[k] >= n[kApRows])
      return fail(PZ_EINDEX, "row %u of a pool of %llu rows", rows[k], (unsigned long long)n[kApRows]);
    offs[k + 1] = offs[k] + (so[rows[k] + 1] - so[rows[k]]);
  }
  if (offs[nrows] > cap)
    return fail(PZ_ERANGE, "the hashes take %llu bytes, capacity %llu", (unsigned long long)offs[nrows], (unsigned long long)cap);
  for (uint64_t k = 0; k < nrows; ++k)
    if (offs[k + 1] > offs[k]) std::memcpy(out + offs[k], sb.data() + so[rows[k]], offs[k + 1] - offs[k]);
  return PZ_OK;
}

int pz_att_pool_capacity(pz_att_pool* h, uint64_t caps[7]) {
  if (!h || !caps) return fail(PZ_EINVAL, "attestation pool / caps is null");
  std::lock_guard<std::mutex> lk(h->mu);
  std::memcpy(caps, h->cap, sizeof h->cap);
  return PZ_OK;
}

int pz_dev_att_pool_reserve(pz_att_pool* h, const uint64_t min_caps[7], void* stream) {
  int rc = check_reserve(h, min_caps);
  if (rc) return rc;
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  uint64_t new_cap[kApCols];
  if (!ap_reserve_caps(h->cap, min_caps, new_cap)) return PZ_OK;
  return enqueue_reserve(h, new_cap, static_cast<hipStream_t>(stream));
}

int pz_att_pool_reserve(pz_att_pool* h, const uint64_t min_caps[7]) {
  int rc = check_reserve(h, min_caps);
  if (rc) return rc;
  HostForm f(h, "attestation pool reserve");
  if (f.rc) return f.rc;
  uint64_t new_cap[kApCols];
  if (!ap_reserve_caps(h->cap, min_caps, new_cap)) return PZ_OK;
  if ((rc = enqueue_reserve(h, new_cap, f.st.s))) return rc;
  return f.st.sync();
}

uint64_t pz_att_pool_need_scratch_bytes(uint64_t n) { return need_scratch_bytes(n); }

int pz_dev_att_pool_need(const pz_attestation_cols* a, uint64_t n, const int32_t* status, const uint8_t* take0,
                         const uint8_t* take1, uint64_t* d_need, void* d_scratch, void* stream) {
  int rc = check_need(a, n, status);
  if (rc < 0) return rc;
  if (!d_need || (reinterpret_cast<uintptr_t>(d_need) & 7)) return fail(PZ_EINVAL, "d_need must be an 8-B aligned device pointer");
  if (!d_scratch || !aligned16(d_scratch)) return fail(PZ_EINVAL, "d_scratch must be a 16-B aligned device pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rc == 1) {  // no row: zeros, in stream order
    hipError_t e = hipMemsetAsync(d_need, 0, 2 * kApCols * 8, s);
    return e == hipSuccess ? PZ_OK : hip_fail(e, "hipMemsetAsync");
  }
  return enqueue_need(*a, n, status, take0, take1, d_need, d_scratch, s);
}

int pz_att_pool_need(const pz_attestation_cols* ha, uint64_t n, const int32_t* status, const uint8_t* take0,
                     const uint8_t* take1, uint64_t need[2][7]) {
  int rc = check_need(ha, n, status);
  if (rc < 0) return rc;
  if (!need) return fail(PZ_EINVAL, "need is null");
  std::memset(need, 0, 2 * kApCols * 8);
  if (rc == 1) return PZ_OK;
  HostForm f(nullptr, "attestation pool need");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_attestation_cols d;
  stage_att_cols(st, *ha, n, kAttAllCols, &d);
  const int32_t* d_status = st.up(status, n);
  const uint8_t* d_take0 = take0 ? st.up(take0, n) : nullptr;
  const uint8_t* d_take1 = take1 ? st.up(take1, n) : nullptr;
  uint64_t* d_need = st.up<uint64_t>(nullptr, 2 * kApCols);
  uint8_t* scr = st.up<uint8_t>(nullptr, need_scratch_bytes(n));
  if (st.rc) return st.rc;
  if ((rc = enqueue_need(d, n, d_status, d_take0, d_take1, d_need, scr, st.s))) return rc;
  st.down(&need[0][0], d_need, 2 * kApCols);
  return st.sync();
}

#ifdef PZ_AB_BUILD
// (tools/attpool_reserve_probe.py) pz_dev_att_pool_reserve with one event pair on its launch;
// synchronises and returns the launch's milliseconds in ms[0].  PZ_EINVAL where nothing would grow.
int pz_debug_att_pool_reserve_timed(pz_att_pool* h, const uint64_t min_caps[7], void* stream, float ms[1]) {
  int rc = check_reserve(h, min_caps);
  if (rc) return rc;
  if (!ms) return fail(PZ_EINVAL, "null ms");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  uint64_t new_cap[kApCols];
  if (!ap_reserve_caps(h->cap, min_caps, new_cap)) return fail(PZ_EINVAL, "nothing to time");
  Events ev;
  if ((rc = ev.create(2))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = enqueue_reserve(h, new_cap, s, &ev);
  return ev.elapsed(rc, ms, nullptr, 1, s, "timed attestation pool reserve");
}

// (tools/attpool_reserve_probe.py) pz_dev_att_pool_need (n > 0) with one event pair per launch;
// synchronises and returns the two launches' milliseconds (need, scan) in ms[0..2).
int pz_debug_att_pool_need_timed(const pz_attestation_cols* a, uint64_t n, const int32_t* status, const uint8_t* take0,
                                 const uint8_t* take1, uint64_t* d_need, void* d_scratch, void* stream, float ms[2]) {
  int rc = check_need(a, n, status);
  if (rc) return rc < 0 ? rc : fail(PZ_EINVAL, "nothing to time");
  if (!ms || !d_need || !d_scratch) return fail(PZ_EINVAL, "null pointer");
  Events ev;
  if ((rc = ev.create(3))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = enqueue_need(*a, n, status, take0, take1, d_need, d_scratch, s, &ev);
  return ev.elapsed(rc, ms, nullptr, 2, s, "timed attestation pool need");
}

// (tools/attpool_probe.py) The long-range threshold of the write launch (0: the product's); returns
// the previous one.  At least 16: the wave copy's tail is the range's last 16 bytes.
uint64_t pz_debug_att_pool_long_bytes(uint64_t bytes) {
  const uint64_t old = g_long_bytes;
  g_long_bytes = bytes == 0 ? kApLongBytes : std::max<uint64_t>(bytes, 16);
  return old;
}

// (tools/attpool_probe.py) pz_dev_att_pool_append (a non-null a) or pz_dev_att_pool_prune (a null)
// with one event pair per launch; synchronises and returns the four launches' milliseconds (size,
// scan, commit, write) in ms[0..4).
int pz_debug_att_pool_timed(pz_att_pool* h, const pz_attestation_cols* a, uint64_t n, const int32_t* status,
                            const uint32_t* committee, const uint8_t* take, uint64_t last_state_recalc, void* d_scratch,
                            void* stream, float ms[4]) {
  if (!h || !ms) return fail(PZ_EINVAL, "null pointer");
  int rc = h->use();
  if (rc) return rc;
  if (a && ((rc = check_append(h, a, n, status, committee)) || !d_scratch)) return rc < 0 ? rc : fail(PZ_EINVAL, "nothing to time");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!a && h->rows_ub == 0) return fail(PZ_EINVAL, "nothing to time");
  Events ev;
  if ((rc = ev.create(5))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a) {
    rc = enqueue(h, append_args(h, *a, n, status, committee, take), d_scratch, s, &ev);
    if (!rc) h->rows_ub = std::min(h->cap[kApRows], h->rows_ub + n);
  } else {
    if ((rc = grow_set(h, h->live ^ 1, h->cap))) return rc;
    rc = enqueue(h, prune_args(h, last_state_recalc), h->scratch.ptr, s, &ev);
    if (!rc) h->live ^= 1;
  }
  return ev.elapsed(rc, ms, nullptr, 4, s, "timed attestation pool call");
}
#endif

}  // extern "C"
