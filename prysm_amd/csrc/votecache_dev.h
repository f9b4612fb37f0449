// The pure rules of the device-resident block vote cache (votecache.hip), as host/device inlines:
// the hash-to-slot table's cell encodings, home cell and probe step, common.BytesToHash from a
// byte range, the oblique skip rule of calculateBlockVoteCache (blockchain/core.go:300-345) and
// the place of a signed parent hash (getSignedParentHashes, core.go:348-360) among a call's
// sources, and the rules of its growth and retirement (the keep decision, the renumbering, the
// rehash insert, with the argument for which entries may be retired).  The kernels and the
// stand-alone CPU checks (tests/votecache_san.cpp, tests/votecache_retain_san.cpp, plain g++
// under ASan+UBSan) compile the same text.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PZ_HD __host__ __device__ __forceinline__
#else
#define PZ_HD inline
#endif

namespace pz {

// ---- the table ---------------------------------------------------------------------------
// Open addressing over u32 cells.  cells = the smallest power of two >= 2 * slot_cap, at least 2;
// the home cell of a hash is le32(hash[0..4]) & (cells - 1); linear probing, wrapping around.
// A cell holds kVcEmpty, a committed slot id (bit 31 clear), or a tentative claim
// kVcTentative | source index (bit 31 set; a call's source count is below 2^31, so the largest
// claim is 0xFFFFFFFE and never reads as kVcEmpty).
constexpr uint32_t kVcEmpty = 0xFFFFFFFFu;
constexpr uint32_t kVcTentative = 0x80000000u;
constexpr uint32_t kVcNone = 0xFFFFFFFFu;  // src_slot / src_cell: none
constexpr uint32_t kVcMaxSlotCap = 1u << 30;

PZ_HD uint32_t vc_cells(uint32_t slot_cap) {
  uint32_t c = 2;
  while (c < 2ull * slot_cap) c <<= 1;
  return c;
}
PZ_HD bool vc_is_empty(uint32_t cell) { return cell == kVcEmpty; }
PZ_HD bool vc_is_slot(uint32_t cell) { return (cell & kVcTentative) == 0; }
PZ_HD bool vc_is_claim(uint32_t cell) { return cell != kVcEmpty && (cell & kVcTentative) != 0; }
PZ_HD uint32_t vc_claim(uint32_t source) { return kVcTentative | source; }
PZ_HD uint32_t vc_claim_source(uint32_t cell) { return cell & ~kVcTentative; }

struct Hash32 {
  uint32_t w[8];  // little-endian words of the 32 bytes
};

PZ_HD uint32_t vc_home(const Hash32& h, uint32_t cells) { return h.w[0] & (cells - 1); }
PZ_HD uint32_t vc_next(uint32_t cell, uint32_t cells) { return (cell + 1) & (cells - 1); }

PZ_HD bool vc_hash_eq(const Hash32& a, const Hash32& b) {
  uint32_t d = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) d |= a.w[k] ^ b.w[k];
  return d == 0;
}

// The 32 bytes at p, at any alignment (byte loads: nothing outside [p, p + 32) is read).
PZ_HD Hash32 vc_load_hash(const uint8_t* p) {
  Hash32 h;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    h.w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) |
             ((uint32_t)p[4 * k + 3] << 24);
  return h;
}

// The 32 bytes at a 16-byte aligned p as two 16-byte loads (a query row, keys[slot]).
PZ_HD Hash32 vc_load_hash16(const uint8_t* p) {
  const uint8_t* q = static_cast<const uint8_t*>(__builtin_assume_aligned(p, 16));
  Hash32 h;
  __builtin_memcpy(&h.w[0], q, 16);
  __builtin_memcpy(&h.w[4], q + 16, 16);
  return h;
}

// A read of the table between calls (no launch writes it meanwhile: plain loads): the slot of h,
// or kVcNone.  `if _, ok := blockVoteCache[blockHash]` (core.go:414).  Probes from the home cell
// for at most `cells` steps; an empty cell ends the probe; a cell holding a slot id below nslots
// is compared with keys[slot] (32-byte aligned); any other value -- a claim, which cannot exist
// between calls, or an id the cache never gave out -- is skipped and never used as an index.
PZ_HD uint32_t vc_probe(const uint32_t* table, uint32_t cells, const uint8_t* keys, uint32_t nslots, const Hash32& h) {
  uint32_t c = vc_home(h, cells);
  for (uint32_t step = 0; step < cells; ++step, c = vc_next(c, cells)) {
    const uint32_t v = table[c];
    if (vc_is_empty(v)) return kVcNone;
    if (v < nslots && vc_hash_eq(h, vc_load_hash16(keys + 32ull * v))) return v;
  }
  return kVcNone;
}

// common.BytesToHash of data[lo .. hi): the last 32 bytes of a longer range, a shorter one
// right-aligned behind zeros.  Reads only bytes of the range.  (hi < lo counts as empty.)
PZ_HD Hash32 vc_bytes_to_hash(const uint8_t* data, uint64_t lo, uint64_t hi) {
  const uint64_t len = hi > lo ? hi - lo : 0;
  if (len >= 32) return vc_load_hash(data + (hi - 32));
  const uint32_t pad = 32u - (uint32_t)len;
  Hash32 h;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t at = 4u * k + j;
      if (at >= pad) w |= (uint32_t)data[lo + (at - pad)] << (8 * j);
    }
    h.w[k] = w;
  }
  return h;
}

// ---- calculateBlockVoteCache's rules --------------------------------------------------------
constexpr uint32_t kVcParents = 64;  // params.CycleLength signed parent hashes per attestation

// core.go:318-320 for one (parent, oblique element) pair: the parent is skipped when the RAW
// element (elem_len bytes; elem = its bytes when elem_len == 32) equals it.  Go compares a
// [32]byte converted to a slice with the element's slice, so only a 32-byte element can match.
PZ_HD bool vc_skipped_by(const Hash32& parent, const Hash32& elem, uint64_t elem_len) {
  return elem_len == 32 && vc_hash_eq(parent, elem);
}

// A row's parents stay inside recent[]: m <= 64 obliques and recent[ps .. ps + 64 - m) exists
// (core.go:353's slice bounds, which the checks report as PZ_ERANGE).
PZ_HD bool vc_parents_in_range(uint64_t m, uint64_t ps, uint64_t n_recent) {
  return m <= kVcParents && ps <= n_recent && kVcParents - m <= n_recent - ps;
}

// The source index of parent r of a row (m obliques starting at element f0, parents_start ps):
// source s < n_recent is recent[s], source n_recent + e is oblique element e, normalised.
PZ_HD uint64_t vc_parent_source(uint32_t r, uint64_t m, uint64_t ps, uint64_t f0, uint64_t n_recent) {
  const uint64_t nrec = kVcParents - m;
  return r < nrec ? ps + r : n_recent + f0 + (r - nrec);
}

// ---- growth and retirement (pz_[dev_]vote_cache_reserve, pz_[dev_]vote_cache_retain) ---------
// The reference's map only grows (types/state.go:27-31): every candidate block's hash and every
// oblique parent hash becomes an entry (core.go:300-345) and none is ever deleted.  A reserve
// keeps that meaning exactly: more slots, every entry where it was.  A retain keeps the entries
// whose key is among the caller's hashes and drops the rest.
//
// Which entries a later stateRecalc can still read.  The justification loop (core.go:411-431)
// reads blockVoteCache only at RecentBlockHashes()[0..63] of the ActiveState being promoted; the
// map is part of neither state's encoding nor root and is not persisted.  RecentBlockHashes is a
// window of 128 candidate hashes that moves on by one whenever a block replaces the candidate, and
// a candidate is only ever replaced by a block of a strictly higher slot (service.go:320-333): a
// block hash that has left the ring never enters it again.  So an entry whose key is neither in
// the ring (its 128 entries and the one hash of history beside them) nor among the candidates of
// the run in hand -- the run's hash log, every window any block of the run or any later block can
// name -- is read by no later justification loop: a later tally may create it anew (an oblique
// parent of that hash), but no loop asks for it.
// What the argument does NOT cover: a hash that is voted for as an OBLIQUE parent before the block
// it names becomes a candidate.  The reference keeps those votes until the hash enters the ring; a
// retain between the vote and the block's arrival drops them.  Retirement is therefore a caller's
// choice (prysm_amd.blockchain.ResidentChain cache_policy="retire"), never the default; growth
// alone ("grow") is exact.
//
// The rules, shared by the kernels of votecache.hip and tests/votecache_retain_san.cpp:
//   keep      a keep-hash marks the slot its probe finds (vc_keep_mark: vc_probe's answer; an
//             absent hash marks nothing, a hash given twice marks the same slot twice);
//   renumber  a kept slot's new id is its rank among the kept slots in ascending old id
//             (vc_new_id over the exclusive count of kept flags before it), a dropped slot's is
//             kVcDropped: slot ids stay deterministic;
//   rehash    the kept keys are distinct, so the first empty cell of a key's probe is claimed
//             without comparing keys (vc_rehash_insert; the claim is an atomicCAS on the device).
constexpr uint32_t kVcDropped = 0xFFFFFFFFu;  // new_id of a slot the retain drops

PZ_HD uint32_t vc_keep_mark(const uint32_t* table, uint32_t cells, const uint8_t* keys, uint32_t nslots, const Hash32& h) {
  return vc_probe(table, cells, keys, nslots, h);
}
PZ_HD bool vc_kept(const uint32_t* flag, uint32_t nslots, uint64_t slot) { return slot < nslots && flag[slot] != 0; }
PZ_HD uint32_t vc_new_id(bool kept, uint64_t kept_before) { return kept ? (uint32_t)kept_before : kVcDropped; }

// claim(cell): true iff the cell was empty and now holds the key's slot.  Linear probing with
// wraparound from the home cell, at most `cells` steps; the cell taken, or kVcNone when every
// cell is full (cells >= 2 * slots: unreachable).
template <class Claim>
PZ_HD uint32_t vc_rehash_insert(uint32_t cells, const Hash32& h, Claim claim) {
  uint32_t c = vc_home(h, cells);
  for (uint32_t step = 0; step < cells; ++step, c = vc_next(c, cells))
    if (claim(c)) return c;
  return kVcNone;
}

// The move of one voter row (`words` u32) between buffer sets whose rows start at any dword: the
// destination is written in 16-byte pieces where it is 16-byte aligned, so a row splits into a head
// of vc_row_head dwords, (words - head) / 4 pieces and a tail of (words - head) % 4 dwords.
PZ_HD uint32_t vc_row_head(uint64_t first_dword, uint64_t words) {
  const uint64_t h = (4 - (first_dword & 3)) & 3;
  return (uint32_t)(h < words ? h : words);
}

// The sticky error word's bits.
constexpr uint64_t kVcErrPanic = 1;     // where Go panics (votes_dev.h tally_item raises bit 0)
constexpr uint64_t kVcErrCapacity = 2;  // a call needed more slots (or probes) than the cache has

}  // namespace pz
