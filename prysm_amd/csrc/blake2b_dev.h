// BLAKE2b-512 device core (RFC 7693), shared by the kernels of blake2b.hip and attdigest.hip:
// one lane per message, the 16-word state v[] and the chaining value h[] in VGPR pairs,
// 64-bit adds as v_lshl_add_u64, rotr 32 a register-pair swap, rotr 24/16/63 two
// v_alignbit_b32 each, 12 rounds fully unrolled so sigma[] indexes registers statically.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pz {

#define IV0 0x6a09e667f3bcc908ULL
#define IV1 0xbb67ae8584caa73bULL
#define IV2 0x3c6ef372fe94f82bULL
#define IV3 0xa54ff53a5f1d36f1ULL
#define IV4 0x510e527fade682d1ULL
#define IV5 0x9b05688c2b3e6c1fULL
#define IV6 0x1f83d9abfb41bd6bULL
#define IV7 0x5be0cd19137e2179ULL

__device__ __forceinline__ uint64_t pack(uint32_t lo, uint32_t hi) {
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t rotr32(uint64_t x) { return (x >> 32) | (x << 32); }
__device__ __forceinline__ uint64_t rotr24(uint64_t x) {
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  return pack(__builtin_amdgcn_alignbit(hi, lo, 24), __builtin_amdgcn_alignbit(lo, hi, 24));
}
__device__ __forceinline__ uint64_t rotr16(uint64_t x) {
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  return pack(__builtin_amdgcn_alignbit(hi, lo, 16), __builtin_amdgcn_alignbit(lo, hi, 16));
}
__device__ __forceinline__ uint64_t rotr63(uint64_t x) {  // == rotl 1
  uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  return pack(__builtin_amdgcn_alignbit(lo, hi, 31), __builtin_amdgcn_alignbit(hi, lo, 31));
}

#define G(a, b, c, d, x, y)        \
  do {                             \
    a = a + b + (x);               \
    d = rotr32(d ^ a);             \
    c = c + d;                     \
    b = rotr24(b ^ c);             \
    a = a + b + (y);               \
    d = rotr16(d ^ a);             \
    c = c + d;                     \
    b = rotr63(b ^ c);             \
  } while (0)

// One round with the message permutation sigma[r] spelled out as literals (RFC 7693 §2.7).
#define ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
  do {                                                                             \
    G(v0, v4, v8, v12, m[s0], m[s1]);                                              \
    G(v1, v5, v9, v13, m[s2], m[s3]);                                              \
    G(v2, v6, v10, v14, m[s4], m[s5]);                                             \
    G(v3, v7, v11, v15, m[s6], m[s7]);                                             \
    G(v0, v5, v10, v15, m[s8], m[s9]);                                             \
    G(v1, v6, v11, v12, m[s10], m[s11]);                                           \
    G(v2, v7, v8, v13, m[s12], m[s13]);                                            \
    G(v3, v4, v9, v14, m[s14], m[s15]);                                            \
  } while (0)

// RFC 7693 compression function F(h, m, t, f); t < 2^64 here (messages < 16 EiB).
__device__ __forceinline__ void compress(uint64_t h[8], const uint64_t m[16], uint64_t t,
                                         bool last) {
  uint64_t v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3];
  uint64_t v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
  uint64_t v8 = IV0, v9 = IV1, v10 = IV2, v11 = IV3;
  uint64_t v12 = IV4 ^ t, v13 = IV5, v14 = last ? ~IV6 : IV6, v15 = IV7;
  ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
  ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
  ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4);
  ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8);
  ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13);
  ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9);
  ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11);
  ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10);
  ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5);
  ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0);
  ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
  ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3);
  h[0] ^= v0 ^ v8;
  h[1] ^= v1 ^ v9;
  h[2] ^= v2 ^ v10;
  h[3] ^= v3 ^ v11;
  h[4] ^= v4 ^ v12;
  h[5] ^= v5 ^ v13;
  h[6] ^= v6 ^ v14;
  h[7] ^= v7 ^ v15;
}

__device__ __forceinline__ void init_h(uint64_t h[8]) {
  // parameter block: digest length 64, key length 0, fanout 1, depth 1
  h[0] = IV0 ^ 0x01010040ULL;
  h[1] = IV1; h[2] = IV2; h[3] = IV3; h[4] = IV4; h[5] = IV5; h[6] = IV6; h[7] = IV7;
}

__device__ __forceinline__ void store_digest(uint8_t* out, const uint64_t h[8], uint32_t out_bytes) {
  // out is 32- or 64-byte aligned per message (out + i*out_bytes with a 16-B aligned base)
  uint4* o = reinterpret_cast<uint4*>(out);
  o[0] = make_uint4((uint32_t)h[0], (uint32_t)(h[0] >> 32), (uint32_t)h[1], (uint32_t)(h[1] >> 32));
  o[1] = make_uint4((uint32_t)h[2], (uint32_t)(h[2] >> 32), (uint32_t)h[3], (uint32_t)(h[3] >> 32));
  if (out_bytes == 64) {
    o[2] = make_uint4((uint32_t)h[4], (uint32_t)(h[4] >> 32), (uint32_t)h[5], (uint32_t)(h[5] >> 32));
    o[3] = make_uint4((uint32_t)h[6], (uint32_t)(h[6] >> 32), (uint32_t)h[7], (uint32_t)(h[7] >> 32));
  }
}

}  // namespace pz
