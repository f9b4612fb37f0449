// The pure rules of the device-resident pending-attestation pool (attpool.hip), as host/device
// inlines: which rows an append keeps (processedAttestations = append(...), blockchain/service.go:
// 280-301) and which a prune keeps (stateRecalc's Slot > lastStateRecalc filter, core.go:444-450),
// a row's seven sizes with the inverted-range rule, shard32's saturation and the capacity decision
// of a call.  The kernels and the stand-alone CPU check (tests/attpool_san.cpp, plain g++ under
// ASan+UBSan) compile the same text.
#pragma once
#include <stdint.h>

#include "../../include/prysm_hip.h"

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

// The commit's decision: the call lands iff base + total fits every capacity (sums that wrap do
// not fit).
PZ_HD bool ap_fits(const uint64_t base[kApCols], const uint64_t total[kApCols], const uint64_t cap[kApCols]) {
  bool fits = true;
  for (int c = 0; c < kApCols; ++c) fits = fits && base[c] <= cap[c] && total[c] <= cap[c] - base[c];
  return fits;
}

}  // namespace pz
