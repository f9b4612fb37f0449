// The reduce-then-scan pieces the column decoder (unwire.hip) and the pending-attestation pool
// (attpool.hip) share: a tile is 256 rows of one workgroup; a size launch leaves every tile's sums,
// one single-workgroup launch (pz_unwire_scan_kernel, defined once in unwire.hip and reached through
// launch_tile_scan) turns them into the tiles' bases and the totals, and a write launch scans its
// tile's sizes again and adds the tile's base.  No workgroup waits for another inside a launch.
// Device inlines: each translation unit that includes this compiles its own copies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pz {

// Launch 2 of a reduce-then-scan: column c's tile sums tiles[c * ntiles ..] become the tiles'
// exclusive bases, totals[c] the column's sum (pz_unwire_scan_kernel; ntiles > 0).
hipError_t launch_tile_scan(uint64_t* tiles, uint64_t ntiles, uint32_t ncols, uint64_t* totals, hipStream_t s);

namespace {

constexpr int kTile = 256, kTileWaves = kTile / 64;
constexpr int kScanThreads = 1024;

inline uint64_t tiles_of(uint64_t n) { return (n + kTile - 1) / kTile; }
inline uint64_t pad256(uint64_t x) { return (x + 255) & ~uint64_t(255); }  // a scratch size

typedef __attribute__((address_space(1))) uint8_t gbyte;

// 16-byte unaligned pieces, the last one overlapping the one before it with the same bytes:
// every load and store lies inside [0, len) (gfx950 runs unaligned global accesses); a span under
// 16 bytes goes byte by byte.
__device__ __forceinline__ void copy16(gbyte* dst, const gbyte* src) {
  uint4 v;
  __builtin_memcpy(&v, src, 16);
  __builtin_memcpy(dst, &v, 16);
}

__device__ __forceinline__ void copy_span(uint8_t* dst, const uint8_t* src, uint64_t len) {
  gbyte* o = reinterpret_cast<gbyte*>((uintptr_t)dst);
  const gbyte* s = reinterpret_cast<const gbyte*>((uintptr_t)src);
  if (len >= 16) {
    uint64_t k = 0;
    for (; k + 16 <= len; k += 16) copy16(o + k, s + k);
    if (k < len) copy16(o + len - 16, s + len - 16);
  } else {
    for (uint64_t k = 0; k < len; ++k) o[k] = s[k];
  }
}

__device__ __forceinline__ uint64_t wsum(uint64_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

// Inclusive scan over the wave.
__device__ __forceinline__ uint64_t wscan(uint64_t x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// The tile's sums of N values per lane, to tiles[c * ntiles + blockIdx.x].
template <int N>
__device__ __forceinline__ void tile_sums(const uint64_t (&v)[N], uint64_t* tiles, uint64_t ntiles) {
  __shared__ uint64_t s_sum[N][kTileWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    const uint64_t t = wsum(v[c]);
    if (lane == 0) s_sum[c][w] = t;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    uint64_t t = 0;
    for (int k = 0; k < kTileWaves; ++k) t += s_sum[threadIdx.x][k];
    tiles[threadIdx.x * ntiles + blockIdx.x] = t;
  }
}

// Each lane's exclusive prefix of N values within the tile (every lane of the workgroup calls).
template <int N>
__device__ __forceinline__ void tile_excl(const uint64_t (&v)[N], uint64_t (&ex)[N]) {
  __shared__ uint64_t s_inc[N][kTileWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t inc[N];
#pragma unroll
  for (int c = 0; c < N; ++c) {
    inc[c] = wscan(v[c]);
    if (lane == 63) s_inc[c][w] = inc[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < N; ++c) {
    uint64_t before = 0;
    for (int k = 0; k < kTileWaves; ++k) before += k < w ? s_inc[c][k] : 0;
    ex[c] = before + inc[c] - v[c];
  }
}

}  // namespace
}  // namespace pz
