// The pure rules of the device-resident pending-attestation pool (attpool.hip), as host/device
// inlines: which rows an append keeps (processedAttestations = append(...), blockchain/service.go:
// 280-301) and which a prune keeps (stateRecalc's Slot > lastStateRecalc filter, core.go:444-450),
// a row's seven sizes with the inverted-range rule, shard32's saturation and the capacity decision
// of a call; and the rules of the pool's growth (pz_[dev_]att_pool_reserve, append's own growth of
// the Go slice, core.go:223-237): which count governs a column's live length, a reserve's
// capacities, a lane's share of a column's move, and what an append would add to the seven counts
// (pz_[dev_]att_pool_need).  The kernels and the stand-alone CPU checks (tests/attpool_san.cpp,
// tests/attpool_reserve_san.cpp, plain g++ under ASan+UBSan) compile the same text.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/prysm_hip.h"
#include "att_cols.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PZ_HD __host__ __device__ __forceinline__
#else
#define PZ_HD inline
#endif

namespace pz {

// The seven sizes of a row, a tile, a call and the pool, in the capacities' order.
constexpr int kApCols = 7;
enum { kApRows = 0, kApJbh = 1, kApSbh = 2, kApBits = 3, kApElems = 4, kApElemBytes = 5, kApSigs = 6 };

// The sticky error word's bits.
constexpr uint64_t kApErrCapacity = 1;  // a call needed more than a capacity holds: it was dropped whole
constexpr uint64_t kApErrInverted = 2;  // a kept row had an inverted range: the row landed empty

// A range above this many bytes is copied by its whole wave, 16 bytes a lane a step; up to it the
// row's own lane copies it (copy_span).
constexpr uint64_t kApLongBytes = 512;

// An append keeps the rows processAttestation passed (and the caller takes).
PZ_HD bool ap_keep_append(const int32_t* status, const uint8_t* take, uint64_t i) {
  return status[i] == PZ_ATT_PROCESSED && (!take || take[i] != 0);
}

// A prune keeps the rows stateRecalc keeps (core.go:446).
PZ_HD bool ap_keep_prune(uint64_t slot, uint64_t last_state_recalc) { return slot > last_state_recalc; }

// AttestationRecord.ShardId as the epoch kernels' u32 column: 2^32 and above still name no
// crosslink record (PZ_XLERR_SHARD), so they saturate.
PZ_HD uint32_t ap_shard32(uint64_t shard_id) { return shard_id > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)shard_id; }

// Where a kept row's ranges start in the source columns, and its sizes.
struct ApRow {
  uint64_t sz[kApCols];  // 1, then the six range lengths
  uint64_t lo[kApCols];  // [kApJbh..kApBits]: byte starts; [kApElems]: first element; [kApElemBytes]: its
                         // first byte; [kApSigs]: first value.  lo[kApRows] unused.
  bool inverted;
};

PZ_HD bool ap_range(const uint64_t* offs, uint64_t i, uint64_t* lo, uint64_t* len) {
  *lo = 0, *len = 0;
  if (!offs) return true;  // (pz_attestation_cols: NULL offsets are empty ranges)
  const uint64_t a = offs[i], b = offs[i + 1];
  if (b < a) return false;
  *lo = a, *len = b - a;
  return true;
}

// Row i of `a` as a kept row.  An inverted range anywhere (offs[i+1] < offs[i], or the element
// bytes' ends the wrong way round) empties the row: it keeps its place with zero scalars and six
// empty ranges, and the caller raises kApErrInverted.
PZ_HD ApRow ap_row(const pz_attestation_cols& a, uint64_t i) {
  ApRow r;
  for (int c = 0; c < kApCols; ++c) r.sz[c] = 0, r.lo[c] = 0;
  r.sz[kApRows] = 1;
  bool ok = ap_range(a.justified_block_hash_offs, i, &r.lo[kApJbh], &r.sz[kApJbh]);
  ok = ap_range(a.shard_block_hash_offs, i, &r.lo[kApSbh], &r.sz[kApSbh]) && ok;
  ok = ap_range(a.attester_bitfield_offs, i, &r.lo[kApBits], &r.sz[kApBits]) && ok;
  ok = ap_range(a.oblique_first, i, &r.lo[kApElems], &r.sz[kApElems]) && ok;
  ok = ap_range(a.aggregate_sig_first, i, &r.lo[kApSigs], &r.sz[kApSigs]) && ok;
  if (ok && r.sz[kApElems]) {
    const uint64_t b0 = a.oblique_offs[r.lo[kApElems]], b1 = a.oblique_offs[r.lo[kApElems] + r.sz[kApElems]];
    r.lo[kApElemBytes] = b0;
    if (b1 < b0) ok = false;
    else r.sz[kApElemBytes] = b1 - b0;
  }
  r.inverted = !ok;
  if (!ok)
    for (int c = 1; c < kApCols; ++c) r.sz[c] = 0;
  return r;
}

// The sizes row i adds to a call: ap_row's when the call keeps it (an inverted row counts as the
// empty row it lands as: 1, then zeros), else zeros.  Returns whether a kept row was inverted.  The
// size phase of append and prune and pz_att_pool_need_kernel are this function under a tile sum.
PZ_HD bool ap_kept_sizes(bool keep, const pz_attestation_cols& a, uint64_t i, uint64_t sz[kApCols]) {
  for (int c = 0; c < kApCols; ++c) sz[c] = 0;
  if (!keep) return false;
  const ApRow r = ap_row(a, i);
  for (int c = 0; c < kApCols; ++c) sz[c] = r.sz[c];
  return r.inverted;
}

// What an append of row i would add (service.go:299-300): the append's size phase without a commit.
PZ_HD bool ap_append_sizes(const pz_attestation_cols& a, const int32_t* status, const uint8_t* take, uint64_t i,
                           uint64_t sz[kApCols]) {
  return ap_kept_sizes(ap_keep_append(status, take, i), a, i, sz);
}

// The commit's decision: the call lands iff base + total fits every capacity (sums that wrap do
// not fit).
PZ_HD bool ap_fits(const uint64_t base[kApCols], const uint64_t total[kApCols], const uint64_t cap[kApCols]) {
  bool fits = true;
  for (int c = 0; c < kApCols; ++c) fits = fits && base[c] <= cap[c] && total[c] <= cap[c] - base[c];
  return fits;
}

// ---- growth ------------------------------------------------------------------------------------
// The pool's buffers: pz_attestation_cols' columns in att_cols.h's order, then committee, shard32.
constexpr int kApSetBufs = kAttNCols + 2;

// Which of the seven counts governs how many elements of a buffer are live, what is added to it (an
// offsets column holds its count + 1 entries; oblique_offs goes by the element count + 1), and the
// element's bytes.
struct ApColRule {
  uint8_t count, plus, width;
};

// Buffer k's rule, read off att_cols.h's table (total < 0: the rows; else totals[total], which is
// count total + 1); committee and shard32 are a u32 a row.  Host: the kernel takes the rules as
// arguments.
inline ApColRule ap_col_rule(int k) {
  if (k >= kAttNCols) return ApColRule{(uint8_t)kApRows, 0, 4};
  const AttCol& c = kAttTable[k];
  return ApColRule{(uint8_t)(c.total < 0 ? kApRows : c.total + 1), c.plus, c.width};
}

// The live bytes of a buffer whose rule is r: under its governing count, and under the seven counts.
PZ_HD uint64_t ap_col_live_bytes(const ApColRule& r, uint64_t governing) { return (governing + r.plus) * r.width; }
PZ_HD uint64_t ap_col_live_bytes(const ApColRule& r, const uint64_t counts[kApCols]) {
  return ap_col_live_bytes(r, counts[r.count]);
}

// A reserve's capacities: max(cap, min_caps) column by column.  Returns whether any capacity rises;
// false is "nothing to do": every min_caps[c] <= cap[c].
PZ_HD bool ap_reserve_caps(const uint64_t cap[kApCols], const uint64_t min_caps[kApCols], uint64_t new_cap[kApCols]) {
  bool grows = false;
  for (int c = 0; c < kApCols; ++c) {
    new_cap[c] = cap[c] > min_caps[c] ? cap[c] : min_caps[c];
    grows = grows || new_cap[c] != cap[c];
  }
  return grows;
}

// Lane t of T's share of moving a column's `live` bytes (T >= 6): the 16-byte pieces t, t + T, ...;
// then of the tail behind the last whole piece, the 4-byte pieces by lanes 0.., the last live & 3
// bytes by the lanes after them.  Every access lies inside [0, live).  dst and src are 16-byte
// aligned (a buffer's start), so every piece is aligned to its size.
PZ_HD void ap_move_lane(uint8_t* dst, const uint8_t* src, uint64_t live, uint64_t t, uint64_t T) {
  const uint64_t n16 = live >> 4;
  for (uint64_t j = t; j < n16; j += T) {
#if defined(__HIP_DEVICE_COMPILE__)
    reinterpret_cast<uint4*>(dst)[j] = reinterpret_cast<const uint4*>(src)[j];
#else
    memcpy(dst + 16 * j, src + 16 * j, 16);
#endif
  }
  const uint64_t base = n16 << 4, n4 = (live & 15) >> 2, n1 = live & 3;
  if (t < n4) {
#if defined(__HIP_DEVICE_COMPILE__)
    reinterpret_cast<uint32_t*>(dst + base)[t] = reinterpret_cast<const uint32_t*>(src + base)[t];
#else
    memcpy(dst + base + 4 * t, src + base + 4 * t, 4);
#endif
  } else if (t < n4 + n1) {
    const uint64_t at = base + 4 * n4 + (t - n4);
    dst[at] = src[at];
  }
}

}  // namespace pz
