// The attestation columns, described once, and the one rule for staging them.  Host-only and free
// of HIP: the C-ABI translation units walk the table instead of spelling the fourteen members out,
// and tests/att_cols_san.cpp drives the same code with a memcpy uploader.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/prysm_hip.h"

namespace pz {

// The six totals, in the order pz_unwire_attestations' totals / caps and pz_att_pool_counts[1..] use.
enum { kTotJbh = 0, kTotSbh, kTotBits, kTotElems, kTotElemBytes, kTotSigs, kAttTotals };

struct AttCol {
  const char* name;        // for messages (the column that answers for a total carries the total's name)
  size_t in_off, out_off;  // the member in pz_attestation_cols / pz_attestation_cols_out
  uint8_t width;           // bytes an element
  int8_t total;            // the length that governs it: totals[total], or (-1) the rows,
  uint8_t plus;            // plus this (1: an offsets column)
};

#define PZ_ATT_COL(member, name, width, total, plus) \
  {name, offsetof(pz_attestation_cols, member), offsetof(pz_attestation_cols_out, member), width, total, plus}
constexpr AttCol kAttTable[] = {
    PZ_ATT_COL(slot, "slot", 8, -1, 0),
    PZ_ATT_COL(shard_id, "shard_id", 8, -1, 0),
    PZ_ATT_COL(justified_slot, "justified_slot", 8, -1, 0),
    PZ_ATT_COL(justified_block_hash, "justified_block_hash", 1, kTotJbh, 0),
    PZ_ATT_COL(justified_block_hash_offs, "justified_block_hash_offs", 8, -1, 1),
    PZ_ATT_COL(shard_block_hash, "shard_block_hash", 1, kTotSbh, 0),
    PZ_ATT_COL(shard_block_hash_offs, "shard_block_hash_offs", 8, -1, 1),
    PZ_ATT_COL(attester_bitfield, "attester_bitfield", 1, kTotBits, 0),
    PZ_ATT_COL(attester_bitfield_offs, "attester_bitfield_offs", 8, -1, 1),
    PZ_ATT_COL(oblique_parent_hashes, "oblique bytes", 1, kTotElemBytes, 0),
    PZ_ATT_COL(oblique_offs, "oblique elements", 8, kTotElems, 1),
    PZ_ATT_COL(oblique_first, "oblique_first", 8, -1, 1),
    PZ_ATT_COL(aggregate_sig, "aggregate_sig", 8, kTotSigs, 0),
    PZ_ATT_COL(aggregate_sig_first, "aggregate_sig_first", 8, -1, 1),
};
#undef PZ_ATT_COL
constexpr int kAttNCols = sizeof kAttTable / sizeof kAttTable[0];

// A member's place in the table (both structs are pointers only, in the table's order).
#define PZ_COL(member) int(offsetof(pz_attestation_cols, member) / sizeof(void*))
enum { kColObl = PZ_COL(oblique_parent_hashes), kColOblOffs = PZ_COL(oblique_offs), kColOblFirst = PZ_COL(oblique_first) };
// The one-level ranges columns as (data, per-row offsets) pairs; the oblique column has two levels.
constexpr int kAttRanges[4][2] = {{PZ_COL(justified_block_hash), PZ_COL(justified_block_hash_offs)},
                                  {PZ_COL(shard_block_hash), PZ_COL(shard_block_hash_offs)},
                                  {PZ_COL(attester_bitfield), PZ_COL(attester_bitfield_offs)},
                                  {PZ_COL(aggregate_sig), PZ_COL(aggregate_sig_first)}};
// `which` of stage_att_cols: a bit per column; a ranges column goes by the bit of its per-row offsets.
constexpr uint32_t kAttAllCols = (1u << kAttNCols) - 1;
constexpr uint32_t kAttBitsCols = 1u << PZ_COL(attester_bitfield_offs), kAttObliqueCols = 1u << kColOblFirst;
constexpr uint32_t kAttKeyCols =  // what Key() and the signed message read
    1u << PZ_COL(slot) | 1u << PZ_COL(shard_id) | 1u << PZ_COL(shard_block_hash_offs) | kAttObliqueCols;
#undef PZ_COL

inline uint64_t att_col_len(const AttCol& c, uint64_t rows, const uint64_t totals[kAttTotals]) {
  return (c.total < 0 ? rows : totals[c.total]) + c.plus;
}
inline const char* att_total_name(int total) {
  for (const AttCol& c : kAttTable)
    if (c.total == total) return c.name;
  return "";
}

// Member k of either struct (memcpy: the members' pointer types differ).
inline void* ptr_at(const void* s, size_t off) {
  void* p;
  std::memcpy(&p, static_cast<const char*>(s) + off, sizeof p);
  return p;
}
inline void set_ptr_at(void* s, size_t off, const void* p) { std::memcpy(static_cast<char*>(s) + off, &p, sizeof p); }
inline const void* att_in(const pz_attestation_cols& c, int k) { return ptr_at(&c, kAttTable[k].in_off); }
inline void att_set_in(pz_attestation_cols* c, int k, const void* p) { set_ptr_at(c, kAttTable[k].in_off, p); }
inline void* att_out(const pz_attestation_cols_out& c, int k) { return ptr_at(&c, kAttTable[k].out_off); }
inline void att_set_out(pz_attestation_cols_out* c, int k, void* p) { set_ptr_at(c, kAttTable[k].out_off, p); }

// The staging rule for a ranges column over the entries a call reads: lo = min(offs),
// hi = max(offs); the device gets data[lo, hi) and offs - lo.  For monotone offsets that is the
// rebase to 0; an inverted range still lies inside the span, so a kernel that reports it can.
struct Span { uint64_t lo = 0, hi = 0; };
inline Span plan_span(const uint64_t* offs, uint64_t entries, std::vector<uint64_t>* rebased) {
  Span s;
  if (entries) s.lo = *std::min_element(offs, offs + entries), s.hi = *std::max_element(offs, offs + entries);
  rebased->resize(entries);
  for (uint64_t i = 0; i < entries; ++i) (*rebased)[i] = offs[i] - s.lo;
  return s;
}

// Applies the rule to the columns of `host` named by `which` (n rows): *dev gets their staged
// copies and NULL everywhere else; a NULL scalar or a NULL offsets column stays NULL with its data.
// staged[kAttTotals] (optional): what was uploaded of each total.  Up is the Stager (runtime.h), or anything
// with its put(host, bytes) -> the device copy, keep() -> a vector that lives until the call's last
// sync, and rc.  Validation is the caller's: nothing here asks for monotone offsets.
template <class Up>
int stage_att_cols(Up& st, const pz_attestation_cols& host, uint64_t n, uint32_t which, pz_attestation_cols* dev,
                   uint64_t* staged = nullptr) {
  uint64_t unused[kAttTotals];
  if (!staged) staged = unused;
  *dev = pz_attestation_cols{};
  std::fill(staged, staged + kAttTotals, 0);
  auto ranges = [&](int kd, int ko, const uint64_t* offs, uint64_t entries) {
    std::vector<uint64_t>& r = st.keep();
    const Span s = plan_span(offs, entries, &r);
    const uint64_t w = kAttTable[kd].width;
    const uint8_t* data = static_cast<const uint8_t*>(att_in(host, kd));
    att_set_in(dev, kd, st.put(data ? data + s.lo * w : nullptr, (s.hi - s.lo) * w));
    att_set_in(dev, ko, st.put(r.data(), entries * 8));
    return s.hi - s.lo;
  };
  for (int k = 0; k < kAttNCols; ++k)  // the scalars
    if (kAttTable[k].total < 0 && !kAttTable[k].plus && (which >> k & 1) && att_in(host, k))
      att_set_in(dev, k, st.put(att_in(host, k), n * kAttTable[k].width));
  for (const auto& r : kAttRanges)
    if ((which >> r[1] & 1) && att_in(host, r[1]))
      staged[kAttTable[r[0]].total] = ranges(r[0], r[1], static_cast<const uint64_t*>(att_in(host, r[1])), n + 1);
  if ((which & kAttObliqueCols) && host.oblique_first) {  // the same rule at both levels
    std::vector<uint64_t>& fr = st.keep();
    const Span f = plan_span(host.oblique_first, n + 1, &fr);
    staged[kTotElems] = f.hi - f.lo;
    staged[kTotElemBytes] = ranges(kColObl, kColOblOffs, host.oblique_offs + f.lo, staged[kTotElems] + 1);
    dev->oblique_first = static_cast<const uint64_t*>(st.put(fr.data(), (n + 1) * 8));
  }
  return st.rc;
}

}  // namespace pz
