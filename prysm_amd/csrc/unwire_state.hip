// The stored CrystallizedState read back into the resident objects' columns, for gfx950: what
// NewBeaconChain's proto.Unmarshal does on the host (blockchain/core.go:86-95; messages.pb.go's
// CrystallizedState) for the resident path.  The rules are unwire_state_dev.h's; exactly the canonical
// encoding is accepted (chain.hip's lenient `reload` stays the reader of anything else).
//
// Field 11 is ONE run of up to millions of length-prefixed records: where record i begins depends on
// every record before it.  No lane, wave or workgroup walks that run, and no workgroup waits for
// another: the order between the stages is the order between the launches.
//   a tile    a workgroup per T = 4,096 positions puts every position's frame_step into LDS; lane e
//             of E = 512 then follows the chain that enters the tile at offset e to where it leaves
//             the tile (or stops) and counts the records it passes: a walk in LDS, T / record-size
//             hops.  A chain can only enter at an offset below the length of the record that crosses
//             the edge, so E bounds a record's length (kRecordLimit) -- the table is E words a tile.
//   b group   a workgroup per G = 64 tiles: lane e composes the G tables for entry e.
//   c chain   one lane chains the groups' tables for the one true entry (offset 0 of tile 0): each
//             group's entry and record base, the number of records, where the run ends.  The run must
//             end at the message's end or at a field-12 header.
//   d tiles   a lane per group follows the true chain through its G tiles: each tile's entry and base.
//   e size    a workgroup per tile rebuilds its steps, one lane lists the records on the true chain
//             (T / record-size hops in LDS) and a lane per record walks it canonically and sizes its
//             two bytes fields: tile_scan.h's reduce-then-scan.
// The serial part is ntiles / G + G dependent steps where the plain walk makes nval.
// Field 12's top-level arrays (64 in practice) are framed by one lane, 1,024 headers a round, and a
// lane per array walks its entries; the members are counted without a walk: every header byte run
// ends in exactly two bytes with a clear top bit per key/length pair, so the members are the span's
// clear-top-bit bytes minus the headers' -- exact once every header has been judged canonical.
//
// Decode: the validators' write launch (a lane per record, all seven columns), then the committee
// table: the arrays' lanes leave every entry's packed span, a workgroup per entry counts its members,
// one workgroup scans the counts, and a workgroup per entry decodes them in parallel -- an element
// ends at each byte with a clear top bit, ranks come from a ballot/popcount scan, each element is
// read back from its last byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "resident.h"
#include "tile_scan.h"
#include "unwire_state_dev.h"

namespace pz {
namespace {

using namespace ustate;

constexpr uint32_t kT = kTileBytes, kE = kEntries, kG = kGroupTiles;
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint16_t kStepLong = 0xffff;
constexpr uint32_t kTermBit = 1u << 13;  // a tile table word: bits 0-12 position or offset, 13 stopped, 16-28 records
constexpr int kArrRound = 1024;          // array headers one lane frames between two barriers
static_assert(kRecordLimit == PZ_CSTATE_RECORD_LIMIT && kT == PZ_CSTATE_TILE_BYTES && kG == PZ_CSTATE_GROUP_TILES, "the header states the framing's units");

// The scratch's words: the result record first, then what the launches hand each other.
enum { W_BODY = 12, W_HTERM, W_TERMS, W_ERR, W_DERR, W_COUNT = 24 };

struct GEntry {
  uint64_t at;    // stopped: the position; else the offset into the next group's first tile
  uint64_t cnt;   // records passed; bit 63: stopped
};

struct UsArgs {
  const uint8_t* d;
  uint64_t len;
  uint64_t body;      // frame: the first byte behind field 10 (decode reads w[W_BODY])
  uint64_t* w;        // [W_COUNT]
  uint32_t* ttable;   // [ntiles * E]
  GEntry* gtable;     // [ngroups * E]
  uint32_t* gentry;   // [ngroups]
  uint64_t* gbase;    // [ngroups]
  uint32_t* tentry;   // [ntiles]
  uint64_t* tbase;    // [ntiles]
  uint64_t* tiles;    // [2 * ntiles]
  uint64_t* result;   // frame: [PZ_CSF_COUNT]; decode: [2]
  pz_validator_cols_out v;
  pz_committee_table_out t;
};

__host__ __device__ inline uint64_t us_tiles(uint64_t len, uint64_t body_beg) { return (len - body_beg) / kT + 1; }
__host__ __device__ inline uint64_t us_groups(uint64_t ntiles) { return (ntiles + kG - 1) / kG; }

__device__ __forceinline__ void err_at(uint64_t* word, uint64_t off) {
  atomicMin(reinterpret_cast<unsigned long long*>(word), (unsigned long long)off);
}

// As wire_state.hip's: the exclusive prefix of v over the workgroup and its sum.  lds: 16 words.
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

// Every position's frame_step of the tile at tile_beg (every lane of the workgroup calls).
__device__ __forceinline__ void build_steps(const uint8_t* d, uint64_t len, uint64_t tile_beg, uint16_t* step) {
  for (uint32_t p = threadIdx.x; p < kT; p += blockDim.x) {
    const uint64_t s = frame_step(d, tile_beg + p, len, kTagValidator);
    step[p] = s == 0 ? 0 : frame_long(s) ? kStepLong : (uint16_t)s;
  }
  __syncthreads();
}

// ---- a: a tile's table -----------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kE) pz_cs_tile_kernel(UsArgs a) {
  __shared__ uint16_t step[kT];
  if (blockIdx.x == 0 && threadIdx.x == 0) a.w[W_BODY] = a.body;  // (for the launches behind this one)
  build_steps(a.d, a.len, a.body + (uint64_t)blockIdx.x * kT, step);
  uint32_t pos = threadIdx.x, cnt = 0, stopped = 0;
  while (pos < kT) {
    const uint16_t s = step[pos];
    if (s == 0 || s == kStepLong) {
      stopped = kTermBit;
      break;
    }
    pos += s;
    ++cnt;
  }
  a.ttable[(uint64_t)blockIdx.x * kE + threadIdx.x] = (stopped ? pos : pos - kT) | stopped | (cnt << 16);
}

// ---- b: a group's table ----------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kE) pz_cs_group_kernel(UsArgs a) {
  const uint64_t body = a.w[W_BODY], ntiles = us_tiles(a.len, body);
  const uint64_t t0 = (uint64_t)blockIdx.x * kG, t1 = t0 + kG < ntiles ? t0 + kG : ntiles;
  uint32_t cur = threadIdx.x;
  GEntry g = {0, 0};
  for (uint64_t t = t0; t < t1; ++t) {
    const uint32_t s = a.ttable[t * kE + cur];
    g.cnt += s >> 16;
    cur = s & (kTermBit - 1);
    if (s & kTermBit) {
      g.at = body + t * kT + cur;
      g.cnt |= 1ull << 63;
      break;
    }
  }
  if (!(g.cnt >> 63)) g.at = cur;
  a.gtable[(uint64_t)blockIdx.x * kE + threadIdx.x] = g;
}

// ---- c: the true chain through the groups ------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64) pz_cs_chain_kernel(UsArgs a) {
  if (threadIdx.x) return;
  const uint64_t body = a.w[W_BODY], ngroups = us_groups(us_tiles(a.len, body));
  uint32_t cur = 0;
  uint64_t total = 0, end = a.len;
  for (uint64_t g = 0; g < ngroups; ++g) {
    a.gentry[g] = cur;
    a.gbase[g] = total;
    if (cur == kNone) continue;
    const GEntry e = a.gtable[g * kE + cur];
    total += e.cnt & ~(1ull << 63);
    if (e.cnt >> 63) {
      end = e.at;
      cur = kNone;
    } else {
      cur = (uint32_t)e.at;
    }
  }
  for (int k = 0; k < W_BODY; ++k) a.w[k] = 0;
  a.w[W_HTERM] = a.w[W_TERMS] = 0;
  a.w[W_ERR] = kNoOffset;
  if (frame_step(a.d, end, a.len, kTagValidator)) {  // (a header the chain stopped at: one over the limit)
    a.w[PZ_CSF_STATUS] = (uint64_t)(int64_t)PZ_ERANGE;
    a.w[PZ_CSF_OFFSET] = end;
  } else if (end != a.len && (end > a.len || a.d[end] != kTagCommittees)) {
    a.w[PZ_CSF_STATUS] = (uint64_t)(int64_t)PZ_EINVAL;
    a.w[PZ_CSF_OFFSET] = end;
  } else {
    a.w[PZ_CSF_NVAL] = total;
    a.w[PZ_CSF_VAL_END] = end;
  }
}

// ---- d: the true chain through each group's tiles -----------------------------------------------------
extern "C" __global__ void __launch_bounds__(kTile) pz_cs_entries_kernel(UsArgs a) {
  const uint64_t ntiles = us_tiles(a.len, a.w[W_BODY]);
  const uint64_t g = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  if (g >= us_groups(ntiles)) return;
  uint32_t cur = a.w[PZ_CSF_STATUS] ? kNone : a.gentry[g];
  uint64_t base = a.gbase[g];
  const uint64_t t1 = (g + 1) * kG < ntiles ? (g + 1) * kG : ntiles;
  for (uint64_t t = g * kG; t < t1; ++t) {
    a.tentry[t] = cur;
    a.tbase[t] = base;
    if (cur == kNone) continue;
    const uint32_t s = a.ttable[t * kE + cur];
    base += s >> 16;
    cur = (s & kTermBit) ? kNone : (s & (kTermBit - 1));
  }
}

// The records of the true chain in this tile, as positions in list; returns their number (every
// lane of the workgroup calls; step is built here).
__device__ __forceinline__ uint32_t list_records(const UsArgs& a, uint64_t tile_beg, uint32_t entry, uint16_t* step,
                                                 uint16_t* list, uint32_t* s_n) {
  build_steps(a.d, a.len, tile_beg, step);
  if (threadIdx.x == 0) {
    uint32_t pos = entry, n = 0;
    while (pos < kT) {
      const uint16_t s = step[pos];
      if (s == 0 || s == kStepLong) break;
      list[n++] = (uint16_t)pos;
      pos += s;
    }
    *s_n = n;
  }
  __syncthreads();
  return *s_n;
}

// ---- e: the validators' sizes -----------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kTile) pz_cs_val_size_kernel(UsArgs a) {
  __shared__ uint16_t step[kT];
  __shared__ uint16_t list[kT / 2];
  __shared__ uint32_t s_n;
  const uint64_t body = a.w[W_BODY], ntiles = us_tiles(a.len, body);
  const uint32_t entry = a.w[PZ_CSF_STATUS] ? kNone : a.tentry[blockIdx.x];
  uint64_t v[2] = {0, 0};
  if (entry != kNone) {  // (workgroup-uniform)
    const uint64_t tile_beg = body + (uint64_t)blockIdx.x * kT;
    const uint32_t n = list_records(a, tile_beg, entry, step, list, &s_n);
    for (uint32_t j = threadIdx.x; j < n; j += kTile) {
      uint64_t beg, blen, err;
      ValRec r;
      frame_body(a.d, tile_beg + list[j], a.len, &beg, &blen);
      if (!walk_validator(a.d, beg, blen, &r, &err)) err_at(a.w + W_ERR, err);
      else v[0] += r.blen[0], v[1] += r.blen[1];
    }
  }
  tile_sums<2>(v, a.tiles, ntiles);
}

// ---- field 12: the bytes with a clear top bit ---------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kTile) pz_cs_terms_kernel(UsArgs a) {
  if (a.w[PZ_CSF_STATUS]) return;
  const uint64_t lo = a.w[PZ_CSF_VAL_END];
  const uint64_t beg = a.w[W_BODY] + (uint64_t)blockIdx.x * kT;
  uint64_t n = 0;
  for (uint32_t p = threadIdx.x; p < kT; p += kTile) {
    const uint64_t at = beg + p;
    n += at >= lo && at < a.len && !(a.d[at] & 0x80);
  }
  n = wsum(n);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(reinterpret_cast<unsigned long long*>(a.w + W_TERMS), (unsigned long long)n);
}

// ---- field 12: the arrays and their entries -------------------------------------------------------------
// One workgroup.  W: also the table's arr_offs, arr_shard, and in coffs[e] entry e's packed span as
// (position << 32 | length) for the members' launches.
template <bool W>
__device__ __forceinline__ void arrays_pass(const UsArgs& a) {
  __shared__ uint64_t s_beg[kArrRound], s_len[kArrRound];
  __shared__ uint64_t lds[16];
  __shared__ uint64_t s_p;
  __shared__ uint32_t s_n;
  if (a.w[PZ_CSF_STATUS]) return;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) s_p = a.w[PZ_CSF_VAL_END];
  uint64_t narr = 0, nent = 0, hterm = 0;
  for (;;) {
    __syncthreads();
    if (tid == 0) {
      uint64_t p = s_p;
      uint32_t n = 0;
      for (uint64_t s; n < kArrRound && (s = frame_step(a.d, p, a.len, kTagCommittees)) != 0; p += s, ++n)
        frame_body(a.d, p, a.len, &s_beg[n], &s_len[n]);
      s_n = n, s_p = p;
    }
    __syncthreads();
    const uint32_t n = s_n;
    uint64_t mine = 0, heads = 0, err = 0;
    if (tid < n) {
      heads = 2;
      const bool ok = walk_committee_array(a.d, s_beg[tid], s_len[tid], [&](uint64_t, uint64_t shard, uint64_t, uint64_t plen) {
        ++mine;
        heads += 2 + (shard ? 2 : 0) + (plen ? 2 : 0);
        return true;
      }, &err);
      if (!ok) err_at(a.w + W_ERR, err);
    }
    uint64_t total, htotal;
    const uint64_t ex = block_excl(mine, &total, lds);
    (void)block_excl(heads, &htotal, lds);
    if (W && tid < n && narr + tid < a.t.narr) {
      a.t.arr_offs[narr + tid] = nent + ex;
      uint64_t e = nent + ex;
      (void)walk_committee_array(a.d, s_beg[tid], s_len[tid], [&](uint64_t, uint64_t shard, uint64_t ppos, uint64_t plen) {
        if (e < a.t.ncomm) {
          a.t.arr_shard[e] = shard;
          a.t.coffs[e] = ppos << 32 | plen;
        }
        ++e;
        return true;
      }, &err);
    }
    narr += n, nent += total, hterm += htotal;
    if (n < kArrRound) break;  // (workgroup-uniform)
  }
  if (tid == 0) {
    if (!W) {
      if (s_p != a.len) err_at(a.w + W_ERR, s_p);
      a.w[PZ_CSF_NARR] = narr, a.w[PZ_CSF_NENTRIES] = nent, a.w[W_HTERM] = hterm;
      a.w[PZ_CSF_F12_END] = s_p;
    } else if (narr == a.t.narr) {
      a.t.arr_offs[narr] = nent;
    }
  }
}
extern "C" __global__ void __launch_bounds__(kArrRound) pz_cs_arrays_kernel(UsArgs a) { arrays_pass<false>(a); }

// ---- the frame's result ---------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(64) pz_cs_result_kernel(UsArgs a) {
  if (threadIdx.x) return;
  uint64_t* w = a.w;
  if (!w[PZ_CSF_STATUS]) {
    if (w[W_ERR] != kNoOffset) {
      for (int k = 0; k < W_BODY; ++k) w[k] = 0;
      w[PZ_CSF_STATUS] = (uint64_t)(int64_t)PZ_EINVAL;
      w[PZ_CSF_OFFSET] = w[W_ERR];
    } else {
      w[PZ_CSF_NMEMBERS] = w[W_TERMS] - w[W_HTERM];
    }
  }
  for (int k = 0; k < PZ_CSF_COUNT; ++k) a.result[k] = w[k];
}

// A refusal or an empty body before any other launch: the record alone.
extern "C" __global__ void __launch_bounds__(64) pz_cs_record_kernel(uint64_t* w, uint64_t* result, int64_t status, uint64_t off,
                                                                    uint64_t body, uint64_t len) {
  if (threadIdx.x) return;
  for (int k = 0; k < W_COUNT; ++k) w[k] = 0;
  w[PZ_CSF_STATUS] = (uint64_t)status, w[PZ_CSF_OFFSET] = off;
  w[PZ_CSF_VAL_END] = w[PZ_CSF_F12_END] = status ? 0 : len;
  w[W_BODY] = body;
  for (int k = 0; k < PZ_CSF_COUNT; ++k) result[k] = w[k];
}

// ---- decode ----------------------------------------------------------------------------------------------
// The caller's sizes against the frame's; a frame that refused stays refused.
extern "C" __global__ void __launch_bounds__(64) pz_cs_begin_kernel(UsArgs a) {
  if (threadIdx.x) return;
  a.w[W_DERR] = kNoOffset;
  if (!a.w[PZ_CSF_STATUS] && (a.t.narr != a.w[PZ_CSF_NARR] || a.t.ncomm != a.w[PZ_CSF_NENTRIES])) a.w[W_DERR] = 0;
}
__device__ __forceinline__ bool decode_off(const UsArgs& a) { return a.w[PZ_CSF_STATUS] || a.w[W_DERR] == 0; }

extern "C" __global__ void __launch_bounds__(kTile) pz_cs_val_write_kernel(UsArgs a) {
  __shared__ uint16_t step[kT];
  __shared__ uint16_t list[kT / 2];
  __shared__ uint64_t lds[16];
  __shared__ uint32_t s_n;
  if (decode_off(a)) return;
  const uint64_t body = a.w[W_BODY], ntiles = us_tiles(a.len, body), nval = a.w[PZ_CSF_NVAL];
  const uint64_t total[2] = {a.w[PZ_CSF_ADDRESS_BYTES], a.w[PZ_CSF_COMMITMENT_BYTES]};
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.v.withdrawal_address_offs[nval] = total[0];
    a.v.randao_commitment_offs[nval] = total[1];
  }
  if (nval == 0 || blockIdx.x >= ntiles) return;
  const uint32_t entry = a.tentry[blockIdx.x];
  if (entry == kNone) return;  // (workgroup-uniform)
  const uint64_t tile_beg = body + (uint64_t)blockIdx.x * kT;
  const uint32_t n = list_records(a, tile_beg, entry, step, list, &s_n);
  uint64_t carry[2] = {a.tiles[blockIdx.x], a.tiles[ntiles + blockIdx.x]};
  uint8_t* const cols[2] = {a.v.withdrawal_address, a.v.randao_commitment};
  uint64_t* const offs[2] = {a.v.withdrawal_address_offs, a.v.randao_commitment_offs};
  for (uint32_t j0 = 0; j0 < n; j0 += kTile) {
    const uint32_t j = j0 + threadIdx.x;
    ValRec r;
    bool live = false;
    if (j < n) {
      uint64_t beg, blen, err;
      frame_body(a.d, tile_beg + list[j], a.len, &beg, &blen);
      live = walk_validator(a.d, beg, blen, &r, &err);
    }
    const uint64_t rank = a.tbase[blockIdx.x] + j;
    live = live && rank < nval;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      uint64_t sum;
      const uint64_t at = carry[c] + block_excl(live ? r.blen[c] : 0, &sum, lds);
      carry[c] += sum;
      if (!live) continue;
      offs[c][rank] = at;
      if (at + r.blen[c] <= total[c]) copy_span(cols[c] + at, a.d + r.bpos[c], r.blen[c]);
    }
    if (live) {
      a.v.public_key[rank] = r.s[1];
      a.v.withdrawal_shard[rank] = r.s[2];
      a.v.balance[rank] = r.s[5];
      a.v.start_dynasty[rank] = r.s[6];
      a.v.end_dynasty[rank] = r.s[7];
    }
  }
}

extern "C" __global__ void __launch_bounds__(kArrRound) pz_cs_arrays_write_kernel(UsArgs a) {
  if (decode_off(a)) return;
  arrays_pass<true>(a);
}

// Entry e's packed span, from coffs[e] as the arrays' launch left it.
__device__ __forceinline__ void packed_of(const UsArgs& a, uint64_t e, uint64_t* pos, uint64_t* len) {
  const uint64_t x = a.t.coffs[e];
  *pos = x >> 32, *len = x & 0xffffffffull;
}

// A workgroup per entry: its members' number, into arr_comm[e] until the scan.
extern "C" __global__ void __launch_bounds__(kTile) pz_cs_member_count_kernel(UsArgs a) {
  if (decode_off(a)) return;
  __shared__ uint64_t lds[16];
  uint64_t pos, len, n = 0, total;
  packed_of(a, blockIdx.x, &pos, &len);
  for (uint64_t i = threadIdx.x; i < len; i += kTile) n += !(a.d[pos + i] & 0x80);
  (void)block_excl(n, &total, lds);
  if (threadIdx.x == 0) a.t.arr_comm[blockIdx.x] = (uint32_t)total;
}

// One workgroup: the counts in arr_comm become the entries' first members (below 2^32: the message is).
extern "C" __global__ void __launch_bounds__(kScanThreads) pz_cs_member_scan_kernel(UsArgs a) {
  if (decode_off(a)) return;
  __shared__ uint64_t lds[16];
  uint64_t carry = 0, total;
  for (uint64_t base = 0; base < a.t.ncomm; base += kScanThreads) {
    const uint64_t e = base + threadIdx.x;
    const uint64_t ex = block_excl(e < a.t.ncomm ? a.t.arr_comm[e] : 0, &total, lds);
    if (e < a.t.ncomm) a.t.arr_comm[e] = (uint32_t)(carry + ex);
    carry += total;
  }
  if (threadIdx.x == 0) {
    a.t.coffs[a.t.ncomm] = carry;
    if (carry != a.w[PZ_CSF_NMEMBERS]) err_at(a.w + W_DERR, a.w[PZ_CSF_VAL_END]);
  }
}

// A workgroup per entry: an element ends at each byte with a clear top bit; its rank is the entry's
// first member plus the ballot/popcount scan of those bytes; it is read back from its last byte.
extern "C" __global__ void __launch_bounds__(kTile) pz_cs_member_write_kernel(UsArgs a) {
  if (decode_off(a)) return;
  __shared__ uint32_t s_wave[kTileWaves];
  __shared__ uint64_t s_pos, s_len, s_base;
  const uint64_t e = blockIdx.x;
  if (threadIdx.x == 0) {
    packed_of(a, e, &s_pos, &s_len);
    s_base = a.t.arr_comm[e];
  }
  __syncthreads();
  const uint64_t pos = s_pos, len = s_len, nmem = a.w[PZ_CSF_NMEMBERS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t carry = s_base;
  for (uint64_t i0 = 0; i0 < len; i0 += kTile) {
    const uint64_t i = i0 + threadIdx.x;
    const bool ends = i < len && !(a.d[pos + i] & 0x80);
    const uint64_t ballot = __ballot(ends);
    if (lane == 0) s_wave[w] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (int k = 0; k < kTileWaves; ++k) {
      before += k < w ? s_wave[k] : 0;
      all += s_wave[k];
    }
    __syncthreads();  // (s_wave is rewritten by the next round)
    if (ends) {
      const uint64_t rank = carry + before + __popcll(ballot & ((1ull << lane) - 1));
      uint32_t x;
      uint64_t first;
      if (!member_at(a.d, pos, pos + i, &x, &first)) err_at(a.w + W_DERR, first);
      else if (rank < nmem) a.t.members[rank] = x;
    }
    carry += all;
  }
  if (threadIdx.x == 0) {  // (every lane has read s_base and the packed span: the barriers above, or none was needed)
    a.t.coffs[e] = s_base;
    a.t.arr_comm[e] = (uint32_t)e;
  }
}

extern "C" __global__ void __launch_bounds__(64) pz_cs_end_kernel(UsArgs a) {
  if (threadIdx.x) return;
  if (a.w[PZ_CSF_STATUS]) {
    a.result[0] = a.w[PZ_CSF_STATUS], a.result[1] = a.w[PZ_CSF_OFFSET];
  } else {
    a.result[0] = a.w[W_DERR] == kNoOffset ? 0 : (uint64_t)(int64_t)PZ_EINVAL;
    a.result[1] = a.w[W_DERR] == kNoOffset ? 0 : a.w[W_DERR];
  }
}

// ---- the host side ---------------------------------------------------------------------------------------
struct UsLayout {
  uint64_t w, ttable, gtable, gentry, gbase, tentry, tbase, tiles, end;  // byte offsets
};
UsLayout us_layout(uint64_t len) {
  const uint64_t nt = us_tiles(len, 0), ng = us_groups(nt);
  UsLayout l;
  l.w = 0;
  l.ttable = r16(8 * W_COUNT);
  l.gtable = l.ttable + r16(4 * nt * kE);
  l.gentry = l.gtable + r16(sizeof(GEntry) * ng * kE);
  l.gbase = l.gentry + r16(4 * ng);
  l.tentry = l.gbase + r16(8 * ng);
  l.tbase = l.tentry + r16(4 * nt);
  l.tiles = l.tbase + r16(8 * nt);
  l.end = l.tiles + r16(16 * nt);
  return l;
}

UsArgs us_args(const uint8_t* d, uint64_t len, void* scratch, uint64_t* result) {
  const UsLayout l = us_layout(len);
  uint8_t* p = static_cast<uint8_t*>(scratch);
  UsArgs a;
  std::memset(&a, 0, sizeof a);
  a.d = d, a.len = len, a.result = result;
  a.w = reinterpret_cast<uint64_t*>(p + l.w);
  a.ttable = reinterpret_cast<uint32_t*>(p + l.ttable);
  a.gtable = reinterpret_cast<GEntry*>(p + l.gtable);
  a.gentry = reinterpret_cast<uint32_t*>(p + l.gentry);
  a.gbase = reinterpret_cast<uint64_t*>(p + l.gbase);
  a.tentry = reinterpret_cast<uint32_t*>(p + l.tentry);
  a.tbase = reinterpret_cast<uint64_t*>(p + l.tbase);
  a.tiles = reinterpret_cast<uint64_t*>(p + l.tiles);
  return a;
}

int check_bytes(const uint8_t* d_bytes, uint64_t len, const void* d_scratch, const char* what) {
  if (len && !d_bytes) return fail(PZ_EINVAL, "%s: d_bytes is null", what);
  if (!d_scratch || !aligned16(d_scratch)) return fail(PZ_EINVAL, "%s: d_scratch must be a 16-B aligned device pointer", what);
  return PZ_OK;
}

}  // namespace
}  // namespace pz

using namespace pz;

extern "C" {

int pz_cstate_head(const uint8_t* cstate, uint64_t len, uint64_t scalars[PZ_RS_COUNT], pz_cstate_rest* rest, uint64_t* rec_dynasty,
                   uint64_t* rec_slot, uint8_t* rec_hash, uint64_t* rec_hash_offs, uint64_t rec_cap, uint64_t* nrec,
                   uint64_t* body_beg) {
  if (!scalars || !rest || !nrec || !body_beg) return fail(PZ_EINVAL, "cstate head: null scalars / rest / nrec / body_beg");
  *nrec = 0, *body_beg = 0;
  if (len && !cstate) return fail(PZ_EINVAL, "cstate head: cstate is null");
  if (rec_cap && (!rec_dynasty || !rec_slot || !rec_hash || !rec_hash_offs))
    return fail(PZ_EINVAL, "cstate head: null record columns with rec_cap > 0");
  Head h;
  uint64_t err = 0, hash_end = 0;
  if (rec_hash_offs) rec_hash_offs[0] = 0;
  const bool ok = walk_head(cstate, len, &h, [&](uint64_t i, uint64_t dynasty, uint64_t hpos, uint64_t hlen, uint64_t slot) {
    if (i < rec_cap) {
      rec_dynasty[i] = dynasty, rec_slot[i] = slot;
      std::memcpy(rec_hash + hash_end, cstate + hpos, hlen);
      rec_hash_offs[i + 1] = hash_end += hlen;
    }
    return true;
  }, &err);
  if (!ok) {
    *body_beg = err;
    return fail(PZ_EINVAL, "stored CrystallizedState: the field at offset %llu is not canonical", (unsigned long long)err);
  }
  *nrec = h.nrec;
  if (h.nrec > rec_cap)
    return fail(PZ_ERANGE, "stored CrystallizedState holds %llu crosslink records, room for %llu", (unsigned long long)h.nrec,
                (unsigned long long)rec_cap);
  for (int k = 0; k < PZ_RS_COUNT; ++k) scalars[k] = 0;
  scalars[PZ_RS_LAST_STATE_RECALC] = h.f[1], scalars[PZ_RS_JUSTIFIED_STREAK] = h.f[2];
  scalars[PZ_RS_LAST_JUSTIFIED_SLOT] = h.f[3], scalars[PZ_RS_LAST_FINALIZED_SLOT] = h.f[4];
  scalars[PZ_RS_CURRENT_DYNASTY] = h.f[5], scalars[PZ_RS_TOTAL_DEPOSITS] = h.f[7];
  std::memset(rest, 0, sizeof *rest);
  rest->crosslinking_start_shard = h.f[6];
  rest->dynasty_seed_len = (uint32_t)h.seed_len;
  if (h.seed_len) std::memcpy(rest->dynasty_seed, cstate + h.seed_pos, h.seed_len);
  rest->dynasty_seed_last_reset = h.f[9];
  *body_beg = h.body_beg;
  return PZ_OK;
}

uint64_t pz_cstate_scratch_bytes(uint64_t len) { return us_layout(len).end; }

// The frame behind the ABI; ev: the A/B library's event pairs (runtime.h), NULL in the product.
static int frame_impl(const uint8_t* d_bytes, uint64_t len, uint64_t body_beg, void* d_scratch, uint64_t* d_result, void* stream,
                      Events* ev) {
  int rc = check_bytes(d_bytes, len, d_scratch, "cstate frame");
  if (rc) return rc;
  if (!d_result) return fail(PZ_EINVAL, "cstate frame: d_result is null");
  if (body_beg > len) return fail(PZ_EINVAL, "cstate frame: body_beg %llu behind the message's %llu bytes", (unsigned long long)body_beg,
                                  (unsigned long long)len);
  hipStream_t s = static_cast<hipStream_t>(stream);
  UsArgs a = us_args(d_bytes, len, d_scratch, d_result);
  if (len == 0) {  // zeros, nothing launched
    hipError_t e = hipMemsetAsync(d_result, 0, 8 * PZ_CSF_COUNT, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.w, 0, 8 * W_COUNT, s);
    return e == hipSuccess ? PZ_OK : hip_fail(e, "hipMemsetAsync");
  }
  if (body_beg == len || len >= (1ull << 32)) {  // nothing behind the head; or 4 GiB and more: refused
    const bool big = len >= (1ull << 32);
    hipLaunchKernelGGL(pz_cs_record_kernel, dim3(1), dim3(64), 0, s, a.w, d_result, (int64_t)(big ? PZ_ERANGE : PZ_OK),
                       (uint64_t)0, body_beg, len);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_cs_record_kernel");
  }
  a.body = body_beg;
  hipError_t e;
  const uint64_t nt = us_tiles(len, body_beg), ng = us_groups(nt);
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_cs_tile_kernel, dim3((uint32_t)nt), dim3(kE), 0, s, a);
  stamp(ev, 1, s);
  hipLaunchKernelGGL(pz_cs_group_kernel, dim3((uint32_t)ng), dim3(kE), 0, s, a);
  stamp(ev, 2, s);
  hipLaunchKernelGGL(pz_cs_chain_kernel, dim3(1), dim3(64), 0, s, a);
  hipLaunchKernelGGL(pz_cs_entries_kernel, dim3((uint32_t)((ng + kTile - 1) / kTile)), dim3(kTile), 0, s, a);
  stamp(ev, 3, s);
  hipLaunchKernelGGL(pz_cs_val_size_kernel, dim3((uint32_t)nt), dim3(kTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_cs_val_size_kernel");
  stamp(ev, 4, s);
  if ((e = launch_tile_scan(a.tiles, nt, 2, a.w + PZ_CSF_ADDRESS_BYTES, s)) != hipSuccess) return hip_fail(e, "pz_unwire_scan_kernel");
  stamp(ev, 5, s);
  hipLaunchKernelGGL(pz_cs_terms_kernel, dim3((uint32_t)nt), dim3(kTile), 0, s, a);
  hipLaunchKernelGGL(pz_cs_arrays_kernel, dim3(1), dim3(kArrRound), 0, s, a);
  stamp(ev, 6, s);
  hipLaunchKernelGGL(pz_cs_result_kernel, dim3(1), dim3(64), 0, s, a);
  stamp(ev, 7, s);
  return (e = hipGetLastError()) == hipSuccess ? PZ_OK : hip_fail(e, "pz_cs_result_kernel");
}

int pz_dev_cstate_frame(const uint8_t* d_bytes, uint64_t len, uint64_t body_beg, void* d_scratch, uint64_t* d_result, void* stream) {
  return frame_impl(d_bytes, len, body_beg, d_scratch, d_result, stream, nullptr);
}

static int decode_impl(const uint8_t* d_bytes, uint64_t len, void* d_scratch, const pz_validator_cols_out* v,
                       const pz_committee_table_out* t, uint64_t* d_status, void* stream, Events* ev) {
  int rc = check_bytes(d_bytes, len, d_scratch, "cstate decode");
  if (rc) return rc;
  if (!v || !t || !d_status) return fail(PZ_EINVAL, "cstate decode: null columns / table / d_status");
  if (!v->public_key || !v->withdrawal_shard || !v->balance || !v->start_dynasty || !v->end_dynasty || !v->withdrawal_address ||
      !v->randao_commitment || !v->withdrawal_address_offs || !v->randao_commitment_offs)
    return fail(PZ_EINVAL, "cstate decode: a null validator column (an empty one still needs an address)");
  if (!t->arr_offs || !t->coffs || !t->arr_shard || !t->arr_comm || !t->members)
    return fail(PZ_EINVAL, "cstate decode: a null table column (an empty one still needs an address)");
  if (t->narr >= (1ull << 31) || t->ncomm >= (1ull << 31)) return fail(PZ_EINVAL, "cstate decode: 2^31 arrays or entries, or more");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e;
  if (len == 0) {
    e = hipMemsetAsync(d_status, 0, 16, s);
    return e == hipSuccess ? PZ_OK : hip_fail(e, "hipMemsetAsync");
  }
  UsArgs a = us_args(d_bytes, len, d_scratch, d_status);
  a.v = *v, a.t = *t;
  const uint64_t nt = us_tiles(len, 0);  // (the host's bound: the launches read the frame's own numbers)
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_cs_begin_kernel, dim3(1), dim3(64), 0, s, a);
  hipLaunchKernelGGL(pz_cs_val_write_kernel, dim3((uint32_t)nt), dim3(kTile), 0, s, a);
  stamp(ev, 1, s);
  hipLaunchKernelGGL(pz_cs_arrays_write_kernel, dim3(1), dim3(kArrRound), 0, s, a);
  stamp(ev, 2, s);
  if (t->ncomm) hipLaunchKernelGGL(pz_cs_member_count_kernel, dim3((uint32_t)t->ncomm), dim3(kTile), 0, s, a);
  stamp(ev, 3, s);
  if (t->ncomm) hipLaunchKernelGGL(pz_cs_member_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, a);
  stamp(ev, 4, s);
  if (t->ncomm) hipLaunchKernelGGL(pz_cs_member_write_kernel, dim3((uint32_t)t->ncomm), dim3(kTile), 0, s, a);
  stamp(ev, 5, s);
  hipLaunchKernelGGL(pz_cs_end_kernel, dim3(1), dim3(64), 0, s, a);
  stamp(ev, 6, s);
  return (e = hipGetLastError()) == hipSuccess ? PZ_OK : hip_fail(e, "pz_cs_end_kernel");
}

int pz_dev_cstate_decode(const uint8_t* d_bytes, uint64_t len, void* d_scratch, const pz_validator_cols_out* v,
                         const pz_committee_table_out* t, uint64_t* d_status, void* stream) {
  return decode_impl(d_bytes, len, d_scratch, v, t, d_status, stream, nullptr);
}

#ifdef PZ_AB_BUILD
// (tests, tools/unwire_state_probe.py) unwire_state_dev.h's sequential verdict of a stored state, host
// only: out = {status, offset, nval, narr, nentries, nmembers}.
int pz_debug_cstate_check(const uint8_t* cstate, uint64_t len, uint64_t out[6]) {
  if (!out || (len && !cstate)) return fail(PZ_EINVAL, "cstate check: null cstate / out");
  const Verdict v = check_host(cstate, len);
  out[0] = (uint64_t)(int64_t)v.status, out[1] = v.off, out[2] = v.nval, out[3] = v.narr, out[4] = v.nentries, out[5] = v.nmembers;
  return PZ_OK;
}
// frame_host alone, timed on the calling thread: out = {status, offset, nval, val_end, narr, f12_end}.
int pz_debug_cstate_frame_host(const uint8_t* cstate, uint64_t len, uint64_t body_beg, uint64_t out[6]) {
  if (!out || (len && !cstate) || body_beg > len) return fail(PZ_EINVAL, "cstate frame_host: bad arguments");
  const Framed f = frame_host(cstate, len, body_beg);
  out[0] = (uint64_t)(int64_t)f.status, out[1] = f.off, out[2] = f.nval, out[3] = f.val_end, out[4] = f.narr, out[5] = f.f12_end;
  return PZ_OK;
}
// (tools/unwire_state_probe.py) The two calls with event pairs between their launches; synchronise and
// return the milliseconds.  Frame, ms[7]: tile, group, chain + entries, size, scan, terms + arrays,
// result.  Decode, ms[6]: begin + validators, arrays, member count, member scan, member write, end.
// Only for a message with a body (0 < body_beg < len < 4 GiB).
int pz_debug_cstate_frame_timed(const uint8_t* d_bytes, uint64_t len, uint64_t body_beg, void* d_scratch, uint64_t* d_result,
                                void* stream, float ms[7]) {
  if (!ms || len == 0 || body_beg >= len || len >= (1ull << 32)) return fail(PZ_EINVAL, "cstate frame timed: no body to frame");
  Events ev;
  int rc = ev.create(8);
  if (rc) return rc;
  rc = frame_impl(d_bytes, len, body_beg, d_scratch, d_result, stream, &ev);
  return ev.elapsed(rc, ms, nullptr, 7, static_cast<hipStream_t>(stream), "cstate frame timed");
}
int pz_debug_cstate_decode_timed(const uint8_t* d_bytes, uint64_t len, void* d_scratch, const pz_validator_cols_out* v,
                                 const pz_committee_table_out* t, uint64_t* d_status, void* stream, float ms[6]) {
  if (!ms || len == 0) return fail(PZ_EINVAL, "cstate decode timed: no body to decode");
  Events ev;
  int rc = ev.create(7);
  if (rc) return rc;
  rc = decode_impl(d_bytes, len, d_scratch, v, t, d_status, stream, &ev);
  return ev.elapsed(rc, ms, nullptr, 6, static_cast<hipStream_t>(stream), "cstate decode timed");
}
#endif

}  // extern "C"
