// The two states' proto3 encodings from the device-resident objects, for gfx950: what
// PersistActiveState / PersistCrystallizedState store and ActiveState.Hash() / CrystallizedState.Hash()
// hash (blockchain/core.go:161-177, types/state.go:138-149, 237-248).
//
// No workgroup ever waits for another (no spin, no look-back, no polling) in the kernels of this
// file: every cross-launch fact travels through a launch boundary, and the sums that only the device
// knows are read on the device while the grids come from host bounds.
//
// ShardAndCommitteesForSlots (field 12), pz_dev_wire_committees, four launches:
//   1 plan   one workgroup: validates the table (the arrays' offsets, every committee id, the member
//            sum against members_cap) and turns the entries' committee sizes into a prefix of chunks,
//            a chunk being up to kWsChunk members of one entry.
//   2 size   a workgroup per chunk: finds its entry by a binary search of that prefix (one lane),
//            loads its members coalesced and sums their varint lengths.
//   3 scan   one workgroup forms the nested lengths bottom-up -- packed body, ShardAndCommittee,
//            framed entry, array body, framed array -- as three exclusive scans (chunks, entries,
//            arrays) and the total.
//   4 write  a workgroup per chunk scans its members' lengths again and writes the varints; behind
//            them in the same grid a lane per entry and a lane per array write the headers, so an
//            entry with an empty committee and an array without entries still get theirs.
// A table error leaves its code beside the length and every later launch returns at once.
//
// The CrystallizedState, pz_dev_crystallized_state_bytes: the head (fields 1-9 and the crosslink
// records, one workgroup, a lane per record) is written right-aligned so that it ends at the
// host-known bound H; pz_dev_wire_validators runs as it is at d_out + H; a tail launch reads the
// validators' length on the device and copies the caller's encoded field 12 behind them.
//
// The ActiveState, pz_dev_active_state_bytes: pz_dev_wire_attestations(field 1) over the pool's view,
// then one workgroup writes recent_block_hashes (field 2, a lane per hash) at the device-known end.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "attpool_dev.h"
#include "recalc_dev.h"
#include "resident.h"
#include "serial_hash.h"
#include "tile_scan.h"
#include "wire_state_dev.h"

namespace pz {
namespace {

constexpr int kWsThreads = 256;  // == kWsChunk: one member per lane
static_assert(kWsThreads == (int)kWsChunk, "a chunk is one member per lane");

struct WcArgs {
  pz_committee_table t;
  uint64_t nentries, members_cap, chunks_cap;
  uint32_t field;
  uint8_t* out;
  uint64_t* result;       // [2]: length, status
  uint64_t* status;       // scratch [2]: error bits, chunks
  uint64_t* chunk_first;  // scratch [nentries + 1]
  uint64_t* chunk_pre;    // scratch [chunks_cap + 1]: the chunks' byte sums, then their exclusive prefix
  uint64_t* entry_pre;    // scratch [nentries + 1]: exclusive prefix of the framed entries
  uint64_t* arr_adj;      // scratch [narr]: entry e of array a starts at entry_pre[e] + arr_adj[a]
};

// Exclusive prefix of v over the workgroup (any number of whole waves up to 1024 lanes; every lane
// calls); *total: the workgroup's sum.  lds: 16 words.
__device__ __forceinline__ uint64_t block_excl(uint64_t v, uint64_t* total, uint64_t* lds) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint64_t inc = wscan(v);
  __syncthreads();  // (lds may still be read from the call before)
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  uint64_t before = 0, t = 0;
  for (int k = 0; k < nw; ++k) {
    const uint64_t x = lds[k];
    before += k < w ? x : 0;
    t += x;
  }
  *total = t;
  return before + inc - v;
}

// The last index i in [0, n) with a[i] <= key (a non-decreasing, a[0] <= key).
__device__ __forceinline__ uint64_t last_at_most(const uint64_t* a, uint64_t n, uint64_t key) {
  uint64_t lo = 0, hi = n;  // a[lo] <= key; every index >= hi is > key
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a[mid] <= key) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t vlen32(uint32_t x) {
  return 1 + (x >= (1u << 7)) + (x >= (1u << 14)) + (x >= (1u << 21)) + (x >= (1u << 28));
}

// ---- 1: plan -------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kScanThreads) pz_wc_plan_kernel(WcArgs a) {
  __shared__ uint64_t lds[16];
  __shared__ uint32_t s_err;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_err = 0;
  __syncthreads();  // (with no entries the loop below has no barrier: the 0 must land before any lane's bit)
  uint32_t err = 0;
  if (tid == 0 && (a.t.arr_offs[0] != 0 || a.t.arr_offs[a.t.narr] != a.nentries)) err |= (uint32_t)kWsErrRange;
  for (uint64_t k = tid; k < a.t.narr; k += kScanThreads)
    if (a.t.arr_offs[k] > a.t.arr_offs[k + 1]) err |= (uint32_t)kWsErrRange;
  uint64_t chunks = 0, members = 0;
  for (uint64_t base = 0; base < a.nentries; base += kScanThreads) {
    const uint64_t e = base + tid;
    uint64_t size = 0;
    if (e < a.nentries) {
      const uint32_t c = a.t.arr_comm[e];
      if (c >= a.t.ncomm) {
        err |= (uint32_t)kWsErrIndex;
      } else {
        const uint64_t lo = a.t.coffs[c], hi = a.t.coffs[c + 1];
        if (hi < lo || hi - lo > a.members_cap) err |= (uint32_t)kWsErrRange;
        else size = hi - lo;
      }
    }
    uint64_t tc, tm;
    const uint64_t ex = block_excl(ws_chunks(size), &tc, lds);
    if (e < a.nentries) a.chunk_first[e] = chunks + ex;
    (void)block_excl(size, &tm, lds);
    chunks += tc;
    members += tm;
  }
  if (members > a.members_cap || chunks > a.chunks_cap) err |= (uint32_t)kWsErrRange;
  if (err) atomicOr(&s_err, err);
  __syncthreads();
  if (tid == 0) {
    a.chunk_first[a.nentries] = chunks;
    a.status[0] = s_err;
    a.status[1] = chunks;
  }
}

// The chunk's entry and its members' range.
struct WcChunk {
  uint64_t e, lo, hi;
};
__device__ __forceinline__ WcChunk chunk_of(const WcArgs& a, uint64_t k) {
  WcChunk c;
  c.e = last_at_most(a.chunk_first, a.nentries, k);
  const uint32_t id = a.t.arr_comm[c.e];
  c.lo = a.t.coffs[id] + (k - a.chunk_first[c.e]) * kWsChunk;
  c.hi = a.t.coffs[id + 1] < c.lo + kWsChunk ? a.t.coffs[id + 1] : c.lo + kWsChunk;
  return c;
}

// ---- 2: size -------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kWsThreads) pz_wc_size_kernel(WcArgs a) {
  __shared__ uint64_t lds[16];
  __shared__ WcChunk s_c;
  const uint64_t k = blockIdx.x;
  if (a.status[0] || k >= a.status[1]) return;  // (workgroup-uniform)
  if (threadIdx.x == 0) s_c = chunk_of(a, k);
  __syncthreads();
  const uint64_t i = s_c.lo + threadIdx.x;
  const uint64_t v = i < s_c.hi ? vlen32(a.t.members[i]) : 0;
  uint64_t total;
  (void)block_excl(v, &total, lds);
  if (threadIdx.x == 0) a.chunk_pre[k] = total;
}

// ---- 3: scan -------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kScanThreads) pz_wc_scan_kernel(WcArgs a) {
  __shared__ uint64_t lds[16];
  const uint32_t tid = threadIdx.x;
  const uint64_t st = a.status[0];
  if (st) {
    if (tid == 0) {
      a.result[0] = 0;
      a.result[1] = (uint64_t)(int64_t)((st & kWsErrIndex) ? PZ_EINDEX : PZ_ERANGE);
    }
    return;
  }
  const uint64_t nch = a.status[1];
  uint64_t carry = 0, total;
  for (uint64_t base = 0; base < nch; base += kScanThreads) {  // the chunks' bytes
    const uint64_t k = base + tid;
    const uint64_t v = k < nch ? a.chunk_pre[k] : 0;
    const uint64_t ex = block_excl(v, &total, lds);
    if (k < nch) a.chunk_pre[k] = carry + ex;
    carry += total;
  }
  if (tid == 0) a.chunk_pre[nch] = carry;
  __syncthreads();
  carry = 0;
  for (uint64_t base = 0; base < a.nentries; base += kScanThreads) {  // the framed entries
    const uint64_t e = base + tid;
    uint64_t v = 0;
    if (e < a.nentries)
      v = ws_entry_framed(a.t.arr_shard[e], a.chunk_pre[a.chunk_first[e + 1]] - a.chunk_pre[a.chunk_first[e]]);
    const uint64_t ex = block_excl(v, &total, lds);
    if (e < a.nentries) a.entry_pre[e] = carry + ex;
    carry += total;
  }
  if (tid == 0) a.entry_pre[a.nentries] = carry;
  __syncthreads();
  carry = 0;
  for (uint64_t base = 0; base < a.t.narr; base += kScanThreads) {  // the framed arrays
    const uint64_t k = base + tid;
    uint64_t v = 0, head = 0, first = 0;
    if (k < a.t.narr) {
      first = a.entry_pre[a.t.arr_offs[k]];
      const uint64_t body = a.entry_pre[a.t.arr_offs[k + 1]] - first;
      head = ws_array_head_len(a.field, body);
      v = head + body;
    }
    const uint64_t ex = block_excl(v, &total, lds);
    if (k < a.t.narr) a.arr_adj[k] = carry + ex + head - first;
    carry += total;
  }
  if (tid == 0) {
    a.result[0] = carry;
    a.result[1] = PZ_OK;
  }
}

// ---- 4: write ------------------------------------------------------------------------------------
struct WcPlace {
  uint64_t lo, hi, out;
};

extern "C" __global__ void __launch_bounds__(kWsThreads) pz_wc_write_kernel(WcArgs a) {
  __shared__ uint64_t lds[16];
  __shared__ WcPlace s_p;
  if (a.status[0]) return;
  const uint64_t nch = a.status[1];
  gbyte* out = reinterpret_cast<gbyte*>((uintptr_t)a.out);
  if (blockIdx.x < a.chunks_cap) {  // a chunk's members
    const uint64_t k = blockIdx.x;
    if (k >= nch) return;
    if (threadIdx.x == 0) {
      const WcChunk c = chunk_of(a, k);
      const uint64_t arr = last_at_most(a.t.arr_offs, a.t.narr, c.e);
      const uint64_t first = a.chunk_pre[a.chunk_first[c.e]];
      const uint64_t packed = a.chunk_pre[a.chunk_first[c.e + 1]] - first;
      s_p.lo = c.lo, s_p.hi = c.hi;
      s_p.out = a.entry_pre[c.e] + a.arr_adj[arr] + ws_entry_head_len(a.t.arr_shard[c.e], packed) + (a.chunk_pre[k] - first);
    }
    __syncthreads();
    const uint64_t i = s_p.lo + threadIdx.x;
    const bool live = i < s_p.hi;
    const uint32_t m = live ? a.t.members[i] : 0;
    uint64_t total;
    const uint64_t ex = block_excl(live ? vlen32(m) : 0, &total, lds);
    if (live) (void)ws_put(out + s_p.out + ex, m);
    return;
  }
  // the headers: a lane per entry, then a lane per array
  const uint64_t i = (uint64_t)(blockIdx.x - a.chunks_cap) * kWsThreads + threadIdx.x;
  if (i < a.nentries) {
    const uint64_t arr = last_at_most(a.t.arr_offs, a.t.narr, i);
    const uint64_t packed = a.chunk_pre[a.chunk_first[i + 1]] - a.chunk_pre[a.chunk_first[i]];
    (void)ws_put_entry_head(out + a.entry_pre[i] + a.arr_adj[arr], a.t.arr_shard[i], packed);
  } else if (i - a.nentries < a.t.narr) {
    const uint64_t k = i - a.nentries;
    const uint64_t first = a.entry_pre[a.t.arr_offs[k]];
    const uint64_t body = a.entry_pre[a.t.arr_offs[k + 1]] - first;
    const uint32_t head = ws_array_head_len(a.field, body);
    (void)ws_put_array_head(out + a.arr_adj[k] + first - head, a.field, body);
  }
}

uint64_t chunks_cap_of(uint64_t nentries, uint64_t members_cap) { return members_cap / kWsChunk + nentries; }

struct WcLayout {
  uint64_t status, chunk_first, chunk_pre, entry_pre, arr_adj, end;  // byte offsets
};
WcLayout wc_layout(uint64_t narr, uint64_t nentries, uint64_t members_cap) {
  WcLayout l;
  l.status = 0;
  l.chunk_first = 16;
  l.chunk_pre = l.chunk_first + r16(8 * (nentries + 1));
  l.entry_pre = l.chunk_pre + r16(8 * (chunks_cap_of(nentries, members_cap) + 1));
  l.arr_adj = l.entry_pre + r16(8 * (nentries + 1));
  l.end = l.arr_adj + r16(8 * std::max<uint64_t>(narr, 1));
  return l;
}

int wc_check(const pz_committee_table* t, uint64_t nentries, uint64_t members_cap, uint32_t field_num) {
  if (!t) return fail(PZ_EINVAL, "committee table is null");
  if (field_num >= (1u << 29)) return fail(PZ_EINVAL, "field number %u out of range", field_num);
  if (t->narr >= (1ull << 31) || nentries >= (1ull << 31) || members_cap >= (1ull << 40))
    return fail(PZ_EINVAL, "committee table: 2^31 arrays or entries, or 2^40 members, or more");
  const uint64_t heads = (nentries + t->narr + kWsThreads - 1) / kWsThreads;
  if (chunks_cap_of(nentries, members_cap) + heads >= (1ull << 31))
    return fail(PZ_EINVAL, "committee table: members_cap / %u + nentries + (nentries + narr) / %u must stay below 2^31 (the write grid)",
                kWsChunk, kWsThreads);
  if (t->narr && !t->arr_offs) return fail(PZ_EINVAL, "committee table: arr_offs is null");
  if (nentries && (!t->arr_shard || !t->arr_comm || !t->coffs)) return fail(PZ_EINVAL, "committee table: null entry columns or coffs");
  if (members_cap && !t->members) return fail(PZ_EINVAL, "committee table: members is null");
  return PZ_OK;
}

// The four launches on s; d_scratch holds wc_layout(...).end bytes.  narr > 0.
hipError_t wc_enqueue(const pz_committee_table& t, uint64_t nentries, uint64_t members_cap, uint32_t field_num, uint8_t* d_out,
                      uint64_t* d_result, void* d_scratch, hipStream_t s) {
  const WcLayout l = wc_layout(t.narr, nentries, members_cap);
  uint8_t* p = static_cast<uint8_t*>(d_scratch);
  WcArgs a;
  std::memset(&a, 0, sizeof a);
  a.t = t;
  a.nentries = nentries, a.members_cap = members_cap, a.chunks_cap = chunks_cap_of(nentries, members_cap);
  a.field = field_num;
  a.out = d_out, a.result = d_result;
  a.status = reinterpret_cast<uint64_t*>(p + l.status);
  a.chunk_first = reinterpret_cast<uint64_t*>(p + l.chunk_first);
  a.chunk_pre = reinterpret_cast<uint64_t*>(p + l.chunk_pre);
  a.entry_pre = reinterpret_cast<uint64_t*>(p + l.entry_pre);
  a.arr_adj = reinterpret_cast<uint64_t*>(p + l.arr_adj);
  hipLaunchKernelGGL(pz_wc_plan_kernel, dim3(1), dim3(kScanThreads), 0, s, a);
  if (a.chunks_cap) hipLaunchKernelGGL(pz_wc_size_kernel, dim3((uint32_t)a.chunks_cap), dim3(kWsThreads), 0, s, a);
  hipLaunchKernelGGL(pz_wc_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, a);
  const uint64_t heads = (nentries + t.narr + kWsThreads - 1) / kWsThreads;
  hipLaunchKernelGGL(pz_wc_write_kernel, dim3((uint32_t)(a.chunks_cap + heads)), dim3(kWsThreads), 0, s, a);
  return hipGetLastError();
}

// ---- the CrystallizedState's head and tail -----------------------------------------------------------
struct WhArgs {
  const uint64_t* scalars;
  const uint64_t* rec_dynasty;
  const uint64_t* rec_slot;
  const uint8_t* rec_hash;
  const uint32_t* rec_hash_len;
  uint32_t nrec, stride;
  uint64_t start_shard, seed_reset;
  uint64_t seed[kWsMaxSeed / 8];
  uint32_t seed_len;
  uint8_t* out;
  uint64_t H;
  uint64_t* span;      // [2]: begin, length
  uint64_t* head_len;  // scratch
};

struct WhRec {
  uint64_t dynasty, slot;
  uint32_t len;
};
__device__ __forceinline__ WhRec head_rec(const WhArgs& a, uint64_t r) {
  WhRec x;
  x.dynasty = a.rec_dynasty[r], x.slot = a.rec_slot[r];
  x.len = a.rec_hash_len[r] < a.stride ? a.rec_hash_len[r] : a.stride;
  return x;
}

extern "C" __global__ void __launch_bounds__(kScanThreads) pz_ws_head_kernel(WhArgs a) {
  __shared__ uint64_t lds[16];
  const uint32_t tid = threadIdx.x;
  WsHeadScalars s;
  s.f[0] = s.f[8] = 0;
  s.f[1] = a.scalars[PZ_RS_LAST_STATE_RECALC], s.f[2] = a.scalars[PZ_RS_JUSTIFIED_STREAK];
  s.f[3] = a.scalars[PZ_RS_LAST_JUSTIFIED_SLOT], s.f[4] = a.scalars[PZ_RS_LAST_FINALIZED_SLOT];
  s.f[5] = a.scalars[PZ_RS_CURRENT_DYNASTY], s.f[6] = a.start_shard, s.f[7] = a.scalars[PZ_RS_TOTAL_DEPOSITS];
  s.f[9] = a.seed_reset;
  s.seed_len = a.seed_len;
  const uint32_t sc_len = ws_head_scalars_size(s);
  uint64_t recs = 0, total;
  for (uint64_t base = 0; base < a.nrec; base += kScanThreads) {  // the records' bytes
    const uint64_t r = base + tid;
    uint64_t v = 0;
    if (r < a.nrec) {
      const WhRec x = head_rec(a, r);
      v = ws_record_framed(x.dynasty, x.len, x.slot);
    }
    (void)block_excl(v, &total, lds);
    recs += total;
  }
  const uint64_t head_len = sc_len + recs, begin = ws_span_begin(a.H, head_len);
  gbyte* out = reinterpret_cast<gbyte*>((uintptr_t)a.out);
  if (tid == 0) {
    a.span[0] = begin;
    *a.head_len = head_len;
    gbyte* p = out + begin;
    uint32_t n = 0;
#pragma unroll
    for (uint32_t k = 1; k <= 7; ++k) n += ws_put_scalar(p + n, k, s.f[k]);
    if (a.seed_len) {
      p[n++] = 0x42;
      n += ws_put(p + n, a.seed_len);
#pragma unroll
      for (uint32_t k = 0; k < kWsMaxSeed; ++k)  // (unrolled: the seed is indexed by constants only)
        if (k < a.seed_len) p[n + k] = (uint8_t)(a.seed[k >> 3] >> (8 * (k & 7)));
      n += a.seed_len;
    }
    (void)ws_put_scalar(p + n, 9, s.f[9]);
  }
  uint64_t carry = begin + sc_len;
  for (uint64_t base = 0; base < a.nrec; base += kScanThreads) {
    const uint64_t r = base + tid;
    uint64_t v = 0;
    WhRec x = {0, 0, 0};
    if (r < a.nrec) {
      x = head_rec(a, r);
      v = ws_record_framed(x.dynasty, x.len, x.slot);
    }
    const uint64_t ex = block_excl(v, &total, lds);
    if (r < a.nrec) (void)ws_put_record(out + carry + ex, x.dynasty, a.rec_hash + r * a.stride, x.len, x.slot);
    carry += total;
  }
}

// Copies src[0, len) behind the validators (16-byte pieces inside the span only, as copy_span) and
// completes the span.
extern "C" __global__ void __launch_bounds__(kWsThreads) pz_ws_tail_kernel(uint8_t* out, uint64_t H, const uint64_t* val_len,
                                                                          const uint64_t* head_len, const uint8_t* src,
                                                                          uint64_t len, uint64_t* span) {
  const uint64_t i = (uint64_t)blockIdx.x * kWsThreads + threadIdx.x;
  const uint64_t vl = *val_len;
  if (i == 0) span[1] = ws_span_len(*head_len, vl, len);
  gbyte* o = reinterpret_cast<gbyte*>((uintptr_t)out) + ws_tail_begin(H, vl);
  const gbyte* s = reinterpret_cast<const gbyte*>((uintptr_t)src);
  if (len < 16) {
    if (i == 0)
      for (uint64_t k = 0; k < len; ++k) o[k] = s[k];
    return;
  }
  const uint64_t k = 16 * i;
  if (k + 16 <= len) copy16(o + k, s + k);
  else if (k < len) copy16(o + len - 16, s + len - 16);
}

int cs_check(const pz_recalc_state* st, const pz_cstate_rest* rest, const pz_validator_cols* v, const uint8_t* d_field12,
             uint64_t field12_len) {
  if (!st || !rest || !v) return fail(PZ_EINVAL, "crystallized state: null state / rest / columns");
  if (rest->dynasty_seed_len > kWsMaxSeed) return fail(PZ_EINVAL, "dynasty_seed of %u bytes, at most %u", rest->dynasty_seed_len, kWsMaxSeed);
  if (field12_len && !d_field12) return fail(PZ_EINVAL, "crystallized state: d_field12 is null");
  return PZ_OK;
}

uint64_t cs_scratch(uint64_t nval) { return 16 + r16(pz_wire_scratch_bytes(nval)); }

// Head, validators, tail on s.  d_scratch: [0] the validators' length, [1] the head's, then the
// validators' own scratch.
int cs_enqueue(const RsView& rv, const pz_cstate_rest& rest, const pz_validator_cols* v, uint64_t nval, const uint8_t* d_field12,
               uint64_t field12_len, uint8_t* d_out, uint64_t* d_span, void* d_scratch, hipStream_t s) {
  uint64_t* w = static_cast<uint64_t*>(d_scratch);
  WhArgs a;
  std::memset(&a, 0, sizeof a);
  a.scalars = rv.words;
  a.rec_dynasty = rv.rec_dynasty, a.rec_slot = rv.rec_slot, a.rec_hash = rv.rec_hash, a.rec_hash_len = rv.rec_hash_len;
  a.nrec = rv.nrec, a.stride = rv.stride;
  a.start_shard = rest.crosslinking_start_shard, a.seed_reset = rest.dynasty_seed_last_reset;
  std::memcpy(a.seed, rest.dynasty_seed, rest.dynasty_seed_len);
  a.seed_len = rest.dynasty_seed_len;
  a.out = d_out;
  a.H = ws_head_bound(rv.nrec, rv.stride);
  a.span = d_span;
  a.head_len = w + 1;
  hipLaunchKernelGGL(pz_ws_head_kernel, dim3(1), dim3(kScanThreads), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "pz_ws_head_kernel");
  int rc = pz_dev_wire_validators(v, nval, 11, d_out + a.H, nullptr, w + 2, w, s);
  if (rc) return rc;
  const uint64_t pieces = (field12_len + 15) / 16;
  hipLaunchKernelGGL(pz_ws_tail_kernel, dim3((uint32_t)std::max<uint64_t>((pieces + kWsThreads - 1) / kWsThreads, 1)),
                     dim3(kWsThreads), 0, s, d_out, a.H, w, w + 1, d_field12, field12_len, d_span);
  return (e = hipGetLastError()) == hipSuccess ? PZ_OK : hip_fail(e, "pz_ws_tail_kernel");
}

// ---- the ActiveState's recent_block_hashes ------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kScanThreads) pz_ws_recent_kernel(const uint8_t* recent, const uint8_t* recent_len,
                                                                              uint64_t n, uint8_t* out, const uint64_t* field1_len,
                                                                              uint64_t* total_out) {
  __shared__ uint64_t lds[16];
  const uint32_t tid = threadIdx.x;
  gbyte* o = reinterpret_cast<gbyte*>((uintptr_t)out);
  const gbyte* src = reinterpret_cast<const gbyte*>((uintptr_t)recent);
  uint64_t carry = field1_len ? *field1_len : 0, total;
  for (uint64_t base = 0; base < n; base += kScanThreads) {
    const uint64_t i = base + tid;
    uint32_t len = 0;
    if (i < n) len = recent_len ? (recent_len[i] < 32 ? recent_len[i] : 32) : 32;
    const uint64_t ex = block_excl(i < n ? ws_recent_size(len) : 0, &total, lds);
    if (i < n) (void)ws_put_recent(o + carry + ex, src + 32 * i, len);
    carry += total;
  }
  if (tid == 0) *total_out = carry;
}

int sticky_of(uint64_t word) { return (word & kApErrInverted) ? PZ_EINVAL : (word & kApErrCapacity) ? PZ_ERANGE : PZ_OK; }

int report_pool(int sticky) {
  if (sticky == PZ_EINVAL) return fail(PZ_EINVAL, "an appended row had an inverted range; it landed empty");
  if (sticky == PZ_ERANGE) return fail(PZ_ERANGE, "an append needed more than the pool holds; it was dropped whole");
  return PZ_OK;
}

// The whole ActiveState on s, with its one wait; the pool's sticky code comes back in *sticky and
// the exact row count in *rows_out.  Takes no lock.
int as_enqueue(const ApView& pv, const uint8_t* d_recent, const uint8_t* d_recent_len, uint64_t n_recent,
               uint8_t* d_out, uint64_t cap, uint64_t* d_total, hipStream_t s, int* sticky, uint64_t* rows_out) {
  uint64_t w[kApCols + 1];
  hipError_t e;
  if ((e = hipMemcpyAsync(w, pv.counts, sizeof w, hipMemcpyDeviceToHost, s)) != hipSuccess ||
      (e = hipStreamSynchronize(s)) != hipSuccess)
    return hip_fail(e, "active state: the pool's counts");
  const uint64_t rows = w[kApRows];
  if (rows > pv.rows_cap) return fail(PZ_EINVAL, "the pool reports %llu rows", (unsigned long long)rows);
  *rows_out = rows;  // (the caller notes them: this may run under a device context's lock, where no handle is locked)
  *sticky = sticky_of(w[kApCols]);
  const uint64_t need = pz_active_state_bound(w, n_recent);
  if (cap < need)
    return fail(PZ_ERANGE, "active state: a capacity of %llu bytes, bound %llu; nothing written", (unsigned long long)cap,
                (unsigned long long)need);
  if (need && !d_out) return fail(PZ_EINVAL, "active state: d_out is null");
  uint64_t* d_offs = nullptr;
  if (rows) {
    const uint64_t offs_bytes = r16(8 * (rows + 1));
    void* tmp = nullptr;
    if ((e = hipMallocAsync(&tmp, offs_bytes + pz_wire_attestations_scratch_bytes(rows), s)) != hipSuccess)
      return hip_fail(e, "hipMallocAsync");
    d_offs = static_cast<uint64_t*>(tmp);
    int rc = pz_dev_wire_attestations(&pv.cols, rows, 1, d_out, d_offs, static_cast<uint8_t*>(tmp) + offs_bytes, s);
    if (rc) {
      (void)hipFreeAsync(tmp, s);
      return rc;
    }
  }
  hipLaunchKernelGGL(pz_ws_recent_kernel, dim3(1), dim3(kScanThreads), 0, s, d_recent, d_recent_len, n_recent, d_out,
                     d_offs ? d_offs + rows : nullptr, d_total);
  e = hipGetLastError();
  if (d_offs) {
    const hipError_t e2 = hipFreeAsync(d_offs, s);
    if (e == hipSuccess) e = e2;
  }
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_ws_recent_kernel");
}

void root_of(const uint8_t* msg, uint64_t len, uint8_t root[32]) {
  uint8_t d[64];
  host_blake2b512(msg, (size_t)len, d);
  std::memcpy(root, d, 32);
}

}  // namespace
}  // namespace pz

using namespace pz;

extern "C" {

// ---- ShardAndCommitteesForSlots ------------------------------------------------------------------------
uint64_t pz_wire_committees_bound(uint64_t narr, uint64_t nentries, uint64_t members_cap) {
  return narr * 15 + nentries * 33 + members_cap * 5;
}

uint64_t pz_wire_committees_scratch_bytes(uint64_t narr, uint64_t nentries, uint64_t members_cap) {
  return wc_layout(narr, nentries, members_cap).end;
}

int pz_dev_wire_committees(const pz_committee_table* t, uint64_t nentries, uint64_t members_cap, uint32_t field_num,
                           uint8_t* d_out, uint64_t* d_result, void* d_scratch, void* stream) {
  int rc = wc_check(t, nentries, members_cap, field_num);
  if (rc) return rc;
  if (!d_result) return fail(PZ_EINVAL, "d_result is null");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (t->narr == 0) {
    hipError_t e = hipMemsetAsync(d_result, 0, 16, s);
    return e == hipSuccess ? PZ_OK : hip_fail(e, "hipMemsetAsync");
  }
  if (!d_out) return fail(PZ_EINVAL, "d_out is null");
  if (!d_scratch || !aligned16(d_scratch)) return fail(PZ_EINVAL, "d_scratch must be a 16-B aligned device pointer");
  hipError_t e = wc_enqueue(*t, nentries, members_cap, field_num, d_out, d_result, d_scratch, s);
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_wc_write_kernel");
}

int pz_wire_committees(const pz_committee_table* t, uint64_t nentries, uint32_t field_num, uint8_t* out, uint64_t cap,
                       uint64_t* len) {
  if (!len) return fail(PZ_EINVAL, "len is null");
  *len = 0;
  if (!t) return fail(PZ_EINVAL, "committee table is null");
  if (nentries && (!t->arr_comm || !t->coffs)) return fail(PZ_EINVAL, "committee table: null entry columns or coffs");
  int rc;
  if (t->ncomm && t->coffs && (rc = check_csr(t->coffs, t->ncomm, "committee"))) return rc;  // (sizes the members' upload)
  uint64_t members_cap = 0;  // the sum the table names; the device judges the rest of the table
  for (uint64_t e = 0; e < nentries; ++e) {
    const uint32_t c = t->arr_comm[e];
    if (c < t->ncomm && t->coffs[c + 1] >= t->coffs[c]) members_cap += t->coffs[c + 1] - t->coffs[c];
    if (members_cap >= (1ull << 40)) return fail(PZ_EINVAL, "committee table: 2^40 members or more");
  }
  if ((rc = wc_check(t, nentries, members_cap, field_num))) return rc;
  if (t->narr == 0) return PZ_OK;
  HostForm f(nullptr, "wire committees");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_committee_table d = *t;
  d.arr_offs = st.up(t->arr_offs, t->narr + 1);
  d.arr_shard = st.up(t->arr_shard, nentries);
  d.arr_comm = st.up(t->arr_comm, nentries);
  d.coffs = st.up(t->coffs, t->ncomm + 1);
  d.members = st.up(t->members, t->ncomm && t->coffs ? t->coffs[t->ncomm] : 0);
  void* scratch = st.put(nullptr, pz_wire_committees_scratch_bytes(t->narr, nentries, members_cap));
  uint64_t* d_result = st.zeros<uint64_t>(2);
  uint8_t* d_out = st.up<uint8_t>(nullptr, pz_wire_committees_bound(t->narr, nentries, members_cap));
  if (st.rc) return st.rc;
  st.check(wc_enqueue(d, nentries, members_cap, field_num, d_out, d_result, scratch, st.s), "pz_wc_write_kernel");
  uint64_t res[2] = {0, 0};
  st.down(res, d_result, 2);
  if (st.sync()) return st.rc;
  if ((int64_t)res[1] == PZ_EINDEX) return fail(PZ_EINDEX, "committee table: an entry names a committee the table does not hold");
  if (res[1]) return fail(PZ_ERANGE, "committee table: the arrays' offsets or the committees' ranges do not fit the table");
  *len = res[0];
  if (res[0] > cap)
    return fail(PZ_ERANGE, "output needs %llu bytes, capacity %llu", (unsigned long long)res[0], (unsigned long long)cap);
  if (res[0] && !out) return fail(PZ_EINVAL, "out is null");
  st.down(out, d_out, res[0]);
  return st.sync();
}

// ---- the CrystallizedState ---------------------------------------------------------------------------
uint64_t pz_crystallized_state_bound(uint32_t nrec, uint32_t hash_stride, uint64_t nval, uint64_t val_bytes_total,
                                     uint64_t field12_len) {
  return ws_head_bound(nrec, hash_stride) + pz_wire_validators_bound(nval, val_bytes_total) + field12_len;
}

uint64_t pz_crystallized_state_scratch_bytes(uint64_t nval) { return cs_scratch(nval); }

int pz_dev_crystallized_state_bytes(pz_recalc_state* st, const pz_cstate_rest* rest, const pz_validator_cols* v, uint64_t nval,
                                    const uint8_t* d_field12, uint64_t field12_len, uint8_t* d_out, uint64_t* d_span,
                                    void* d_scratch, void* stream) {
  int rc = cs_check(st, rest, v, d_field12, field12_len);
  if (rc) return rc;
  if (!d_out || !d_span) return fail(PZ_EINVAL, "crystallized state: null d_out / d_span");
  if (!d_scratch || !aligned16(d_scratch)) return fail(PZ_EINVAL, "d_scratch must be a 16-B aligned device pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  RsView rv;
  if ((rc = recalc_state_view(st, &rv, s, true))) return rc;
  hipError_t e = hipSetDevice(rv.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  return cs_enqueue(rv, *rest, v, nval, d_field12, field12_len, d_out, d_span, d_scratch, s);
}

int pz_crystallized_state_read(pz_recalc_state* st, const pz_cstate_rest* rest, const pz_validator_cols* v, uint64_t nval,
                               const uint8_t* d_field12, uint64_t field12_len, uint8_t* out, uint64_t cap, uint64_t* len,
                               uint8_t root[32]) {
  if (!len) return fail(PZ_EINVAL, "len is null");
  *len = 0;
  int rc = cs_check(st, rest, v, d_field12, field12_len);
  if (rc) return rc;
  RsView rv;
  if ((rc = recalc_state_view(st, &rv, nullptr, false))) return rc;
  hipError_t e = hipSetDevice(rv.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  // (the bytes columns' total is not known here: the bound takes every byte the columns could hold
  // from the caller through the offsets' last entries)
  uint64_t val_bytes = 0;
  for (const uint64_t* o : {v->withdrawal_address_offs, v->randao_commitment_offs})
    if (o && nval) {
      uint64_t ends[1];
      if ((e = hipMemcpy(ends, o + nval, 8, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e, "crystallized state read");
      val_bytes += ends[0];
    }
  // The host layer's order (resident.h): the handle, the wait for its last call, then the device
  // context.  No call below takes a handle's lock.
  Resident* r = resident_of(st);
  HostForm f(r, "crystallized state read");
  if (f.rc) return f.rc;
  r->last = f.st.s;  // (what is enqueued below is what the handle's next read waits for, also after an error)
  Stager& sg = f.st;
  const uint64_t bound = pz_crystallized_state_bound(rv.nrec, rv.stride, nval, val_bytes, field12_len);
  uint8_t* d_out = sg.up<uint8_t>(nullptr, bound);
  uint64_t* d_span = sg.zeros<uint64_t>(2);
  void* scratch = sg.put(nullptr, cs_scratch(nval));
  if (sg.rc) return sg.rc;
  if ((rc = cs_enqueue(rv, *rest, v, nval, d_field12, field12_len, d_out, d_span, scratch, sg.s))) return rc;
  uint64_t span[2] = {0, 0}, words[PZ_RS_COUNT + 1] = {};
  sg.down(span, d_span, 2);
  sg.down(words, rv.words, PZ_RS_COUNT + 1);
  if (sg.sync()) return sg.rc;
  *len = span[1];
  if (span[1] > cap)
    return fail(PZ_ERANGE, "output needs %llu bytes, capacity %llu", (unsigned long long)span[1], (unsigned long long)cap);
  if (span[1] && !out) return fail(PZ_EINVAL, "out is null");
  sg.down(out, d_out + span[0], span[1]);
  if (sg.sync()) return sg.rc;
  if (root) root_of(out, span[1], root);
  if (words[PZ_RS_COUNT] & kRsErrPanic)
    return fail(PZ_EINDEX, "stateRecalc would panic (processCrosslinks' indices or CalculateRewards' CheckBit); the state is as before it");
  return PZ_OK;
}

// ---- the ActiveState -----------------------------------------------------------------------------------
uint64_t pz_active_state_bound(const uint64_t counts[7], uint64_t n_recent) {
  if (!counts) return 0;
  return pz_wire_attestations_bound(counts[kApRows], counts[kApJbh] + counts[kApSbh] + counts[kApBits] + counts[kApElemBytes],
                                    counts[kApElems], counts[kApSigs]) +
         34 * n_recent;
}

int pz_dev_active_state_bytes(pz_att_pool* pool, const uint8_t* d_recent, const uint8_t* d_recent_len, uint64_t n_recent,
                              uint8_t* d_out, uint64_t cap, uint64_t* d_total, void* stream) {
  if (!pool || !d_total) return fail(PZ_EINVAL, "active state: null pool / d_total");
  if (n_recent && !d_recent) return fail(PZ_EINVAL, "active state: d_recent is null");
  hipStream_t s = static_cast<hipStream_t>(stream);
  ApView pv;
  int rc = att_pool_peek(pool, &pv, s);
  if (rc) return rc;
  hipError_t e = hipSetDevice(pv.device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  int sticky = PZ_OK;
  uint64_t rows = 0;
  if ((rc = as_enqueue(pv, d_recent, d_recent_len, n_recent, d_out, cap, d_total, s, &sticky, &rows))) return rc;
  att_pool_note_rows(pool, rows);  // (the exact count the wait brought: the next prune's grid)
  return report_pool(sticky);
}

int pz_active_state_read(pz_att_pool* pool, const uint8_t* recent, const uint8_t* recent_len, uint64_t n_recent, uint8_t* out,
                         uint64_t cap, uint64_t* len, uint8_t root[32]) {
  if (!len) return fail(PZ_EINVAL, "len is null");
  *len = 0;
  if (!pool) return fail(PZ_EINVAL, "active state: pool is null");
  if (n_recent && !recent) return fail(PZ_EINVAL, "active state: recent is null");
  uint64_t counts[kApCols];
  int rc = pz_att_pool_counts(pool, counts);  // (waits for the pool's earlier calls; the sticky code is taken below)
  if (rc != PZ_OK && rc != PZ_EINVAL && rc != PZ_ERANGE) return rc;
  ApView pv;
  if ((rc = att_pool_peek(pool, &pv, nullptr))) return rc;  // (nothing of the pool is pending: counts has waited)
  // The host layer's order (resident.h): the handle, the wait for its last call, then the device
  // context.  No call below takes a handle's lock.
  Resident* r = resident_of(pool);
  HostForm f(r, "active state read");
  if (f.rc) return f.rc;
  r->last = f.st.s;  // (what is enqueued below is what the pool's next read waits for, also after an error)
  Stager& sg = f.st;
  const uint64_t bound = pz_active_state_bound(counts, n_recent);
  const uint8_t* d_recent = sg.up(recent, 32 * n_recent);
  const uint8_t* d_len = recent_len ? sg.up(recent_len, n_recent) : nullptr;
  uint8_t* d_out = sg.up<uint8_t>(nullptr, bound);
  uint64_t* d_total = sg.zeros<uint64_t>(1);
  if (sg.rc) return sg.rc;
  int sticky = PZ_OK;
  uint64_t rows = 0;  // (counts has noted them already)
  if ((rc = as_enqueue(pv, d_recent, d_len, n_recent, d_out, bound, d_total, sg.s, &sticky, &rows))) return rc;
  uint64_t total = 0;
  sg.down(&total, d_total, 1);
  if (sg.sync()) return sg.rc;
  *len = total;
  if (total > cap)
    return fail(PZ_ERANGE, "output needs %llu bytes, capacity %llu", (unsigned long long)total, (unsigned long long)cap);
  if (total && !out) return fail(PZ_EINVAL, "out is null");
  sg.down(out, d_out, total);
  if (sg.sync()) return sg.rc;
  if (root) root_of(out, total, root);
  return report_pool(sticky);
}

}  // extern "C"
