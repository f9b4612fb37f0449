// The pure rules of the two states' proto3 encodings (wire_state.hip): the varint length and put,
// the nested lengths of a ShardAndCommittee entry and of an array of them (messages.proto:72,75-77,
// 87-90), the sizes of the CrystallizedState's scalars and crosslink records (messages.proto:59-72,
// 122-126), the ActiveState's recent-hash entries (messages.proto:94-97) and the arithmetic that
// places the pieces of a message round a fixed point.  __host__ __device__ inlines: the kernels
// compile them, and prysm_amd/csrc/tests/wire_state_san.cpp runs them on the CPU under ASan+UBSan.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define WS_HD __host__ __device__ __forceinline__
#else
#define WS_HD inline
#endif

namespace pz {

constexpr uint32_t kWsChunk = 256;        // members of one entry a workgroup sizes and writes
constexpr uint32_t kWsMaxSeed = 64;       // pz_cstate_rest.dynasty_seed
constexpr uint64_t kWsErrRange = 1, kWsErrIndex = 2;  // the committee encoder's status bits

// ---- varints -------------------------------------------------------------------------------------
WS_HD uint32_t ws_vlen(uint64_t x) {
  uint32_t n = 1;
  while (x >= 0x80) {
    x >>= 7;
    ++n;
  }
  return n;
}

// The minimal varint of x at p; returns its length.
template <typename P>
WS_HD uint32_t ws_put(P p, uint64_t x) {
  uint32_t n = 0;
  while (x >= 0x80) {
    p[n++] = (uint8_t)(x | 0x80);
    x >>= 7;
  }
  p[n++] = (uint8_t)x;
  return n;
}

// The key of a length-delimited field (wire type 2); field_num < 2^29.
WS_HD uint64_t ws_key(uint32_t field_num) { return ((uint64_t)field_num << 3) | 2; }

// ---- ShardAndCommitteesForSlots -----------------------------------------------------------------
// Chunks (kWsChunk members each, the last one shorter) of a committee of `size` members.
WS_HD uint64_t ws_chunks(uint64_t size) { return (size + kWsChunk - 1) / kWsChunk; }

// ShardAndCommittee's body: shard_id (field 1, absent when 0), committee (packed field 2 of
// `packed` bytes, absent when empty).
WS_HD uint64_t ws_sc_body(uint64_t shard, uint64_t packed) {
  return (shard ? 1 + ws_vlen(shard) : 0) + (packed ? 1 + ws_vlen(packed) + packed : 0);
}
// The entry as element of ShardAndCommitteeArray.array_shard_and_committee (field 1): 0a, length, body.
WS_HD uint64_t ws_entry_framed(uint64_t shard, uint64_t packed) {
  const uint64_t b = ws_sc_body(shard, packed);
  return 1 + ws_vlen(b) + b;
}
// The bytes of an entry before its first member: 0a, length, [08 shard], [12 packed length].
WS_HD uint32_t ws_entry_head_len(uint64_t shard, uint64_t packed) {
  return 1 + ws_vlen(ws_sc_body(shard, packed)) + (shard ? 1 + ws_vlen(shard) : 0) + (packed ? 1 + ws_vlen(packed) : 0);
}
template <typename P>
WS_HD uint32_t ws_put_entry_head(P p, uint64_t shard, uint64_t packed) {
  uint32_t n = 0;
  p[n++] = 0x0a;
  n += ws_put(p + n, ws_sc_body(shard, packed));
  if (shard) {
    p[n++] = 0x08;
    n += ws_put(p + n, shard);
  }
  if (packed) {
    p[n++] = 0x12;
    n += ws_put(p + n, packed);
  }
  return n;
}
// An array of `body` bytes of framed entries as repeated field field_num: key, length (none of
// either with field_num 0: bare bodies).
WS_HD uint32_t ws_array_head_len(uint32_t field_num, uint64_t body) {
  return field_num ? ws_vlen(ws_key(field_num)) + ws_vlen(body) : 0;
}
template <typename P>
WS_HD uint32_t ws_put_array_head(P p, uint32_t field_num, uint64_t body) {
  if (!field_num) return 0;
  uint32_t n = ws_put(p, ws_key(field_num));
  return n + ws_put(p + n, body);
}

// ---- the CrystallizedState's head: fields 1-9 and the crosslink records --------------------------
// A varint field with a one-byte key (fields 1-15): absent when 0.
WS_HD uint32_t ws_scalar_size(uint64_t v) { return v ? 1 + ws_vlen(v) : 0; }
template <typename P>
WS_HD uint32_t ws_put_scalar(P p, uint32_t field_num, uint64_t v) {
  if (!v) return 0;
  p[0] = (uint8_t)(field_num << 3);
  return 1 + ws_put(p + 1, v);
}
// A bytes field with a one-byte key: absent when empty (the length only; the caller copies the bytes).
WS_HD uint32_t ws_bytes_size(uint32_t len) { return len ? 1 + ws_vlen(len) + len : 0; }
// CrosslinkRecord: dynasty 1, blockhash 2, slot 3.
WS_HD uint32_t ws_record_body(uint64_t dynasty, uint32_t hash_len, uint64_t slot) {
  return ws_scalar_size(dynasty) + ws_bytes_size(hash_len) + ws_scalar_size(slot);
}
// As element of crosslink_records (field 10): 52, length, body.
WS_HD uint32_t ws_record_framed(uint64_t dynasty, uint32_t hash_len, uint64_t slot) {
  const uint32_t b = ws_record_body(dynasty, hash_len, slot);
  return 1 + ws_vlen(b) + b;
}
// The record at p, its hash read from h; returns ws_record_framed.
template <typename P, typename Q>
WS_HD uint32_t ws_put_record(P p, uint64_t dynasty, Q h, uint32_t hash_len, uint64_t slot) {
  uint32_t n = 0;
  p[n++] = 0x52;
  n += ws_put(p + n, ws_record_body(dynasty, hash_len, slot));
  n += ws_put_scalar(p + n, 1, dynasty);
  if (hash_len) {
    p[n++] = 0x12;
    n += ws_put(p + n, hash_len);
    for (uint32_t k = 0; k < hash_len; ++k) p[n++] = h[k];
  }
  n += ws_put_scalar(p + n, 3, slot);
  return n;
}
// Fields 1-9: seven varints (s[0..5] fields 1-5 and 7 from the handle; field 6), the seed, field 9.
struct WsHeadScalars {
  uint64_t f[10];  // f[k]: field k's value, k = 1-7 and 9 (f[0], f[8] unused)
  uint32_t seed_len;
};
WS_HD uint32_t ws_head_scalars_size(const WsHeadScalars& s) {
  uint32_t n = ws_bytes_size(s.seed_len) + ws_scalar_size(s.f[9]);
  for (int k = 1; k <= 7; ++k) n += ws_scalar_size(s.f[k]);
  return n;
}
template <typename P, typename Q>
WS_HD uint32_t ws_put_head_scalars(P p, const WsHeadScalars& s, Q seed) {
  uint32_t n = 0;
  for (uint32_t k = 1; k <= 7; ++k) n += ws_put_scalar(p + n, k, s.f[k]);
  if (s.seed_len) {
    p[n++] = 0x42;
    n += ws_put(p + n, s.seed_len);
    for (uint32_t k = 0; k < s.seed_len; ++k) p[n++] = seed[k];
  }
  n += ws_put_scalar(p + n, 9, s.f[9]);
  return n;
}
// The host-known bound of the head: where the validators start in the output.  A multiple of 16.
WS_HD uint64_t ws_head_bound(uint32_t nrec, uint32_t hash_stride) {
  const uint64_t scalars = 8 * 11 + 2 + kWsMaxSeed;
  const uint64_t body = 11 + (1 + ws_vlen(hash_stride) + hash_stride) + 11;
  const uint64_t h = scalars + (uint64_t)nrec * (1 + ws_vlen(body) + body);
  return (h + 15) & ~15ull;
}

// ---- placement round the fixed point H -----------------------------------------------------------
// The head is written right-aligned, ending at H; the validators start at H; the tail follows them.
WS_HD uint64_t ws_span_begin(uint64_t H, uint64_t head_len) { return H - head_len; }
WS_HD uint64_t ws_tail_begin(uint64_t H, uint64_t validators_len) { return H + validators_len; }
WS_HD uint64_t ws_span_len(uint64_t head_len, uint64_t validators_len, uint64_t tail_len) {
  return head_len + validators_len + tail_len;
}

// ---- the ActiveState's recent_block_hashes (field 2) ----------------------------------------------
// Entry i: 12, length, the last `len` bytes of its 32-byte row (common.BytesToHash right-aligns).
WS_HD uint32_t ws_recent_size(uint32_t len) { return 2 + len; }
template <typename P, typename Q>
WS_HD uint32_t ws_put_recent(P p, Q row, uint32_t len) {
  p[0] = 0x12;
  p[1] = (uint8_t)len;
  for (uint32_t k = 0; k < len; ++k) p[2 + k] = row[32 - len + k];
  return 2 + len;
}

}  // namespace pz
