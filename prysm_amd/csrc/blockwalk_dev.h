// The block walk's rules (blockwalk.hip), stated once as host/device inlines: the sequential
// decisions blockProcessing takes over a run of received blocks that go on (the candidate rule and
// updateHead, blockchain/service.go:320-333; IsCycleTransition, core.go:181-183) and the window of
// ActiveState.RecentBlockHashes each block of the run reads (getSignedParentHashes, core.go:348-360,
// after computeNewActiveState, core.go:223-237, has appended the earlier candidates' hashes in
// place on the chain's own ActiveState, service.go:346, :356).  The kernels and the stand-alone CPU
// check (tests/blockwalk_san.cpp, plain g++ under ASan+UBSan) compile the same text.  No HIP types.
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
