// The wave part of a block scan's tile, for gfx950: what pz_block_walk_scan_kernel (blockwalk.hip)
// and pz_block_cycle_scan_kernel (blockcycle.hip) do alike around blockwalk_dev.h's tile rules.  ONE
// workgroup of kBwTile lanes, a lane per block.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "blockwalk_dev.h"

namespace pz {

__device__ __forceinline__ void copy32(uint8_t* dst, const uint8_t* src) {  // both 16-byte aligned
  const uint4 a = reinterpret_cast<const uint4*>(src)[0], b = reinterpret_cast<const uint4*>(src)[1];
  reinterpret_cast<uint4*>(dst)[0] = a;
  reinterpret_cast<uint4*>(dst)[1] = b;
}

// Inclusive max-scan over the wave.
__device__ __forceinline__ uint64_t wmaxscan(uint64_t x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t y = __shfl_up(x, d, 64);
    if (lane >= d && y > x) x = y;
  }
  return x;
}

// The ring (129 x 32 bytes, in 16-byte pieces) into the head of the log.
__device__ __forceinline__ void scan_ring_head(uint8_t* log, const uint8_t* ring) {
  if (threadIdx.x < 2 * (uint32_t)kBwRing) reinterpret_cast<uint4*>(log)[threadIdx.x] = reinterpret_cast<const uint4*>(ring)[threadIdx.x];
}

// Round 1's words, a set a wave (bw_round1).
struct ScanWords {
  uint64_t max[kBwWaves], fslot[kBwWaves];
  uint32_t fgo[kBwWaves];
};

// Round 1 of the tile at t0 for block j = t0 + threadIdx.x: a wave max-scan by __shfl_up, a __ballot
// for the wave's first block that goes on, the waves' words through LDS and one barrier.  The
// caller's second barrier (behind its own ballot words) is what lets the next tile write s again.
__device__ __forceinline__ BwRound1 scan_round1(ScanWords& s, const BwCarry& c, uint64_t t0, uint64_t j, bool go, uint64_t slot) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t inc = wmaxscan(bw_scan_value(go, true, slot));
  uint64_t before = __shfl_up(inc, 1, 64);
  if (lane == 0) before = 0;
  const uint64_t gob = __ballot(go);
  const uint32_t fl = gob ? (uint32_t)__builtin_ctzll(gob) : 64;
  const uint64_t fs = __shfl(slot, (int)(fl & 63), 64);
  if (lane == 63) s.max[w] = inc;
  if (lane == 0) s.fgo[w] = fl, s.fslot[w] = fs;
  __syncthreads();
  return bw_round1(c, s.max, s.fgo, s.fslot, before, t0, w, j, go, slot);
}

// Candidate j's hash behind the ring, at its rank (two 16-byte loads and stores).
__device__ __forceinline__ void scan_put_hash(uint8_t* log, uint64_t rank, const uint8_t* block_hash, uint64_t j) {
  copy32(log + 32 * (kBwRing + rank), block_hash + 32 * j);
}

// The log's unused tail: entries 129 + ncand up to 129 + n, zeroed.
__device__ __forceinline__ void scan_zero_tail(uint8_t* log, uint64_t ncand, uint64_t n) {
  uint4* log16 = reinterpret_cast<uint4*>(log);
  for (uint64_t p = 2 * (kBwRing + ncand) + threadIdx.x; p < 2 * (kBwRing + n); p += kBwTile) log16[p] = make_uint4(0, 0, 0, 0);
}

}  // namespace pz
