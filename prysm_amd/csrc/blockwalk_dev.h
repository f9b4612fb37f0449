// The block walk's rules (blockwalk.hip), stated once as host/device inlines: the sequential
// decisions blockProcessing takes over a run of received blocks that go on (the candidate rule and
// updateHead, blockchain/service.go:320-333; IsCycleTransition, core.go:181-183) and the window of
// ActiveState.RecentBlockHashes each block of the run reads (getSignedParentHashes, core.go:348-360,
// after computeNewActiveState, core.go:223-237, has appended the earlier candidates' hashes in
// place on the chain's own ActiveState, service.go:346, :356) -- block by block first, then a tile
// of the scan at a time (the carry, the two rounds, the stop), which blockcycle_dev.h's scan takes
// too.  The kernels and the stand-alone CPU checks (tests/blockwalk_san.cpp and
// tests/blockcycle_san.cpp, plain g++ under ASan+UBSan) compile the same text.  No HIP types.
//
// Which blocks go on is the block gate's report (blockgate_dev.h): go_j = report[j] != 0.  The gate
// knows nothing of the parent check (service.go:261-269) or of CanProcessBlock (:272, :308): the
// caller applies both by handing the gate a block_status other than PZ_OK for an ineligible block,
// which closes it.
//
// In block order, with "pending" = a candidate was carried in or an earlier block of the run went on
// (the first block that goes on with nothing pending always becomes the candidate, :331-361):
//   cand_j  = go_j and (not pending, or slot_j > 1 and slot_j > max_j)                    (:320-333)
//   max_j   = the largest of the carried candidate's slot and the scan values before j, where a
//             block's scan value is its slot if it goes on and (slot > 1 or nothing was pending)
//             -- exactly candidateBlock.SlotNumber() before block j: a block raises the maximum
//             only by becoming the candidate, and a block of slot <= 1 becomes it only first.
//   stop    = the first candidate with slot >= last_state_recalc + 64 (that block excluded), with
//             lag > 0 one past the first candidate, else nblocks -- whichever is smallest.
//   rank_j  = the candidates before j;  base_j = 1 - lag + rank_j.
// The log is the ring's 129 entries (entry 0 one hash of history, 1..128 the window) followed by
// the run's candidate hashes in order; block j's window is log[base_j, base_j + 128).
//
// No row of block j names a log position at or past 129 + rank_j: the checks ran with n_recent =
// 128, so a tallied row has end = start - m + 64 <= 128 (core.go:353; blockgate_dev.h bg_row) and
// reads window entries start + r for r < 64 - m, the last being end - 1 <= 127; its absolute
// position is base_j + end - 1 <= 1 - lag + rank_j + 127 < 129 + rank_j.  The log holds 129 + ncand
// hashes with rank_j <= ncand, so every position a row names was written.
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

// pz_block_walk_batch.walk (prysm_amd.blockchain WALK_*).
constexpr uint8_t kBwOff = 0, kBwSaved = 1, kBwCandidate = 2, kBwDeferred = 3;
// The ring: one hash of history, then the 128 of RecentBlockHashes (types/state.go:45-49).
constexpr uint64_t kBwWindow = 128, kBwRing = kBwWindow + 1;
// pz_block_walk_batch.result
enum { kBwStop = 0, kBwNcand, kBwHasCandidate, kBwCandidateSlot, kBwResultWords };
constexpr uint64_t kBwNone = ~uint64_t(0);

PZ_HD bool bw_go(uint8_t report) { return report != 0; }

// What block j adds to the max-scan (max_j above is the exclusive scan joined with the carry).
PZ_HD uint64_t bw_scan_value(bool go, bool pending, uint64_t slot) { return go && (slot > 1 || !pending) ? slot : 0; }

// service.go:320-333: updateHead clears the pending candidate iff slot > its slot and slot > 1.
PZ_HD bool bw_candidate(bool go, bool pending, uint64_t slot, uint64_t max_before) {
  return go && (!pending || (slot > 1 && slot > max_before));
}

// IsCycleTransition, core.go:181-183 (Go's uint64 sum wraps; so does this one).
PZ_HD bool bw_transition(uint64_t slot, uint64_t last_state_recalc) { return slot >= last_state_recalc + PZ_CYCLE_LENGTH; }

// The stop block j asks for (kBwNone: none): a transition candidate stops before itself; with lag
// the first candidate stops after itself, since from the next block on the CrystallizedState
// differs too.
PZ_HD uint64_t bw_stop_at(uint64_t j, bool cand, uint64_t rank, uint64_t slot, uint64_t last_state_recalc, uint64_t lag) {
  if (!cand) return kBwNone;
  if (bw_transition(slot, last_state_recalc)) return j;
  return lag && rank == 0 ? j + 1 : kBwNone;
}

PZ_HD uint8_t bw_walk(bool go, bool cand, bool deferred) {
  return deferred ? kBwDeferred : cand ? kBwCandidate : go ? kBwSaved : kBwOff;
}
PZ_HD uint64_t bw_base(uint64_t lag, uint64_t rank, bool deferred) { return deferred ? 0 : 1 - lag + rank; }

// ---- the same rules a tile at a time: what both scan kernels (blockwalk.hip, blockcycle.hip) and
// the sequential forms of tests/blockwalk_san.cpp and tests/blockcycle_san.cpp compile.  A tile is
// 1,024 consecutive blocks, a lane each, in 16 waves of 64; lane t of the tile at t0 is block t0 + t.
constexpr uint32_t kBwTile = 1024, kBwWaves = kBwTile / 64;

// The carry between tiles, the same in every lane: whether a candidate is pending, the largest scan
// value so far (candidateBlock's slot) and the candidates so far.
struct BwCarry {
  bool pending;
  uint64_t max, cnt;
};
PZ_HD BwCarry bw_carry(uint64_t has_candidate, uint64_t candidate_slot) {
  return BwCarry{has_candidate != 0, has_candidate ? candidate_slot : 0, 0};
}

// Round 1, once every wave has left its words: s_max[k] wave k's largest bw_scan_value(go, true,
// slot), s_fgo[k] its first lane that goes on (64: none) and s_fslot[k] that lane's slot.  `before`
// comes in as the lane's exclusive max over its own wave.  Gives the lane's max_j (before), pending
// and cand_j, and for the tile the carry's next max and the block that became the candidate with
// nothing pending (first; kBwNone: none, or something was carried in).
struct BwRound1 {
  uint64_t before, tile_max, first;
  bool pending, cand;
};
PZ_HD BwRound1 bw_round1(const BwCarry& c, const uint64_t* s_max, const uint32_t* s_fgo, const uint64_t* s_fslot, uint64_t before,
                         uint64_t t0, uint32_t w, uint64_t j, bool go, uint64_t slot) {
  BwRound1 r{before, c.max, kBwNone, false, false};
  uint64_t fslot = 0;
  if (c.max > r.before) r.before = c.max;
  for (uint32_t k = 0; k < kBwWaves; ++k) {
    const uint64_t m = s_max[k];
    if (k < w && m > r.before) r.before = m;
    if (m > r.tile_max) r.tile_max = m;
    if (!c.pending && r.first == kBwNone && s_fgo[k] < 64) r.first = t0 + 64 * k + s_fgo[k], fslot = s_fslot[k];
  }
  // with nothing carried in, the first block that goes on is the candidate whatever its slot
  r.pending = c.pending || r.first < j;  // (kBwNone < j never holds)
  if (r.first < j && fslot > r.before) r.before = fslot;
  if (r.first != kBwNone && bw_scan_value(true, false, fslot) > r.tile_max) r.tile_max = fslot;
  r.cand = bw_candidate(go, r.pending, slot, r.before);
  return r;
}

// Round 2, from the candidates' ballot words (bit l of cand[k]: lane 64 k + l is a candidate): the
// candidates before lane t of the tile, the carry's included, and the tile's count.
struct BwRank {
  uint64_t rank, tile_cnt;
};
PZ_HD BwRank bw_rank(const BwCarry& c, const uint64_t* cand, uint32_t t) {
  BwRank r{c.cnt + (uint64_t)__builtin_popcountll(cand[t >> 6] & ((1ull << (t & 63)) - 1)), 0};
  for (uint32_t k = 0; k < kBwWaves; ++k) {
    const uint64_t n = (uint64_t)__builtin_popcountll(cand[k]);
    if (k < t >> 6) r.rank += n;
    r.tile_cnt += n;
  }
  return r;
}

// The first set bit at or after tile lane `from` of a tile's ballot words (kBwTile: none).
PZ_HD uint32_t bw_first(const uint64_t* ballot, uint32_t from) {
  for (uint32_t k = from >> 6; k < kBwWaves; ++k) {
    uint64_t m = ballot[k];
    if (k == from >> 6) m &= ~uint64_t(0) << (from & 63);
    if (m) return 64 * k + (uint32_t)__builtin_ctzll(m);
  }
  return kBwTile;
}

// The walk's stop in this tile (kBwNone: none), the smallest bw_stop_at of its blocks: its first
// transition candidate (tr: the candidates with bw_transition(slot, last_state_recalc)), or with lag
// one past the run's first candidate.  tests/blockwalk_san.cpp holds it against bw_stop_at block by
// block.
PZ_HD uint64_t bw_tile_stop(const BwCarry& c, uint64_t t0, uint64_t lag, uint64_t n, const uint64_t* cand, const uint64_t* tr) {
  const uint32_t ftr = bw_first(tr, 0), fcand = bw_first(cand, 0);
  uint64_t stop = ftr == kBwTile ? kBwNone : t0 + ftr;
  if (lag && c.cnt == 0 && fcand != kBwTile && t0 + fcand + 1 < stop) stop = t0 + fcand + 1;
  return stop >= n ? kBwNone : stop;
}

PZ_HD void bw_advance(BwCarry& c, const BwRound1& r, uint64_t tile_cnt) {
  c.cnt += tile_cnt, c.max = r.tile_max, c.pending = c.pending || r.first != kBwNone;
}

// An attestation row of a block with walk code w and base `base`.
struct BwRow {
  uint64_t parents_start;
  uint8_t pend_take;
  int32_t vote_status;
};
PZ_HD BwRow bw_row(uint64_t parents_start, uint8_t pend_take, int32_t vote_status, uint8_t w, uint64_t base) {
  BwRow r;
  r.parents_start = parents_start + base;  // (a deferred block's base is 0: its rows stay as they were)
  r.pend_take = pend_take && w == kBwCandidate ? 1 : 0;  // processedAttestations reach the state with the candidate only
  r.vote_status = w == kBwDeferred && vote_status == PZ_ATT_PROCESSED ? PZ_ATT_NOT_PROCESSED : vote_status;
  return r;
}

// The roll: entry k of the new ring is log entry ncand + k.  The stored lengths: computeNewActiveState
// appends to RecentBlockHashes(), which has every entry under BytesToHash (types/state.go:189-195),
// and stores that list back (core.go:230-236): after ANY append every entry is stored with 32 bytes;
// only a ring that nothing was appended to keeps its lengths (the genesis ring's are 0).
// (panic: bit 0 of the gate's flag word, kBgPanic -- the caller lands nothing of the batch, so nothing rolls in.)
PZ_HD uint64_t bw_roll_count(uint64_t ncand, uint32_t gate_flags) { return gate_flags & 1 ? 0 : ncand; }
PZ_HD uint64_t bw_roll_src(uint64_t k, uint64_t ncand) { return ncand + k; }
PZ_HD uint8_t bw_roll_len(uint8_t old_len, uint64_t appended) { return appended ? 32 : old_len; }

// The append of `total` taken hashes: the one of rank r lands in entry 129 + r - total, or nowhere
// (< 0: more than 129 came after it); old entry k lands in k - total, or nowhere.
PZ_HD int64_t bw_append_dst(uint64_t rank, uint64_t total) { return (int64_t)(kBwRing + rank - total); }

}  // namespace pz
