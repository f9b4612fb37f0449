// The rules of a block run that crosses a cycle transition (blockcycle.hip), stated once as
// host/device inlines over blockwalk_dev.h's: which blocks of a run of received blocks the chain takes
// when one of its candidates is a cycle transition (IsCycleTransition, core.go:181-183; stateRecalc,
// core.go:398-497, called from service.go:345-353), which of the two pairs of states each block is
// checked and tallied against, and on which side of stateRecalc its votes and its pending
// attestations land.  The kernels and the stand-alone CPU check (tests/blockcycle_san.cpp, plain g++
// under ASan+UBSan) compile the same text.  No HIP types.
//
// What the two pairs of states share.  stateRecalc builds a new CrystallizedState and a new
// ActiveState for the CANDIDATE (service.go:345-361); the chain keeps its own pair until the next
// block with a larger slot promotes the candidate's (updateHead, service.go:320-322, :170-227).  A
// block is checked and tallied against the chain's pair (service.go:281-318 run before :320).  But
// CalculateRewards writes validators[i].Balance in place (casper/incentives.go:22-28) on the slice
// stateRecalc hands to the new state (core.go:468): the chain's old CrystallizedState shows the
// rewarded balances from the transition block on, and only its scalars (LastStateRecalc,
// LastJustifiedSlot) stay old.  The vote cache is one map shared by every ActiveState
// (core.go:494-496).  So across a transition the chain's and the candidate's states differ in two
// host scalars, in one entry of RecentBlockHashes -- the ring's history entry -- and in where
// stateRecalc stands between two tallies and two pool appends.
//
// In block order (go, pending, cand_j, rank_j and the log as in blockwalk_dev.h; the candidate rule
// is unchanged), with last_state_recalc the value IsCycleTransition reads for the first candidate:
//   T       = with lag == 0 the first candidate with bw_transition(slot, last_state_recalc).  It is
//             INCLUDED: stateRecalc runs between the two phases below.
//   L       = with lag == 0 the first candidate after T; with lag == 1 the first candidate.  It is
//             the block that promotes the transition block's states, and IsCycleTransition reads
//             the promoted state for it: bc_lsr_after = last_state_recalc + 64 after a T of this run
//             (Go's uint64 sum wraps), last_state_recalc itself with lag == 1.
//   lag 0:  L not a transition: stop = L + 1, lag_out = 0.  L a transition (a slot jump of a cycle or
//           more): stop = L, deferred -- one stateRecalc a call --, lag_out = 1.  No L: stop =
//           nblocks, lag_out = 1.  No T: stop = nblocks, lag_out = 0.
//   lag 1:  L not a transition: stop = L + 1, lag_out = 0.  L a transition: it is taken as T, stop =
//           L + 1, lag_out = 1.  No L: stop = nblocks, lag_out = 1.
//   lagged_j = lag or j > T: the block reads the chain's old scalars and the ring as it was before
//             T's hash went in;  base_j = 1 - lagged_j + rank_j, 0 for a deferred block.
//
// No row of block j names a log position at or past 129 + rank_j, lagged or not: the checks ran with
// n_recent = 128, so a tallied row has end = start - m + 64 <= 128 (core.go:353; blockgate_dev.h
// bg_row) and reads window entries up to end - 1 <= 127; its absolute position is base_j + end - 1 <=
// 1 - lagged_j + rank_j + 127 <= 128 + rank_j < 129 + rank_j.  The log holds 129 + ncand hashes and
// rank_j <= ncand for every block before stop, so every position a row names was written; a lagged
// block's smallest position is rank_j >= 0, the history entry when nothing was appended before it.
//
// The promoted ActiveState's window -- what stateRecalc reads as RecentBlockHashes (core.go:413) --
// starts at log entry 1 + t_rank: with lag == 0 that is T's own window; with lag == 1 T's rows read
// the window one entry earlier (base 0), while stateRecalc runs after updateHead on the promoted
// state, whose ring holds the earlier transition block's hash.
#pragma once
#include "blockwalk_dev.h"

namespace pz {

// pz_block_cycle_batch.result: the walk's four words, then T and the lag to carry.
enum { kBcTIndex = kBwResultWords, kBcTRank, kBcTSlot, kBcLagOut, kBcResultWords };

// What IsCycleTransition reads for L (core.go:181-183 on the promoted state).
PZ_HD uint64_t bc_lsr_after(uint64_t last_state_recalc, uint64_t lag) {
  return lag ? last_state_recalc : last_state_recalc + PZ_CYCLE_LENGTH;
}

// The run's state between blocks; the same in every lane.  kBwNone: not met.
struct BcState {
  uint64_t t_index, l_index, stop, lag_out;
};
PZ_HD BcState bc_start(uint64_t lag) { return BcState{kBwNone, kBwNone, kBwNone, lag}; }

// The rule, candidate by candidate: what candidate j of slot `slot` does to the state.
PZ_HD void bc_candidate(BcState& s, uint64_t j, uint64_t slot, uint64_t last_state_recalc, uint64_t lag) {
  if (s.stop != kBwNone) return;
  if (!lag && s.t_index == kBwNone) {  // before T: the walk's blocks
    if (bw_transition(slot, last_state_recalc)) s.t_index = j, s.lag_out = 1;
    return;
  }
  const bool tr = bw_transition(slot, bc_lsr_after(last_state_recalc, lag));
  s.l_index = j, s.lag_out = tr;
  if (lag && tr) s.t_index = j;
  s.stop = lag || !tr ? j + 1 : j;
}

// The same rule a tile at a time, from the tile's ballots: cand (the candidates), tr (the candidates
// with bw_transition(slot, last_state_recalc)) and tr_after (those with bw_transition(slot,
// bc_lsr_after)).  tests/blockcycle_san.cpp holds it against bc_candidate block by block.
PZ_HD void bc_tile(BcState& s, uint64_t t0, uint64_t lag, const uint64_t* cand, const uint64_t* tr, const uint64_t* tr_after) {
  if (s.stop != kBwNone) return;
  uint32_t from = 0;
  if (!lag && s.t_index == kBwNone) {
    const uint32_t t = bw_first(tr, 0);
    if (t == kBwTile) return;
    s.t_index = t0 + t, s.lag_out = 1, from = t + 1;
  }
  const uint32_t l = bw_first(cand, from);
  if (l == kBwTile) return;
  const bool after = (tr_after[l >> 6] >> (l & 63)) & 1;
  s.l_index = t0 + l, s.lag_out = after;
  if (lag && after) s.t_index = s.l_index;
  s.stop = lag || !after ? s.l_index + 1 : s.l_index;
}

PZ_HD bool bc_deferred(const BcState& s, uint64_t j) { return j >= s.stop; }  // (kBwNone: nothing is)
PZ_HD bool bc_lagged(const BcState& s, uint64_t lag, uint64_t j) { return lag || (s.t_index != kBwNone && j > s.t_index); }
PZ_HD uint64_t bc_base(bool lagged, uint64_t rank, bool deferred) { return deferred ? 0 : 1 - (uint64_t)lagged + rank; }

// An attestation row of block b with walk code w and base `base`; t_index as the result record
// holds it (all ones: no T, and then every block is of phase 0).
struct BcRow {
  uint64_t parents_start;
  int32_t vote0, vote1;
  uint8_t take0, take1;
};
PZ_HD int32_t bc_narrow(int32_t vote_status) { return vote_status == PZ_ATT_PROCESSED ? PZ_ATT_NOT_PROCESSED : vote_status; }
PZ_HD BcRow bc_row(uint64_t parents_start, uint8_t pend_take, int32_t vote_status, uint8_t w, uint64_t base, uint64_t b, uint64_t t_index) {
  BcRow r;
  const bool live = w != kBwDeferred, cand = pend_take && w == kBwCandidate;
  r.parents_start = parents_start + base;  // (a deferred block's base is 0: its rows stay as they were)
  r.vote0 = live && b <= t_index ? vote_status : bc_narrow(vote_status);  // tallied before stateRecalc, T's own rows too (service.go:313-318)
  r.vote1 = live && b > t_index ? vote_status : bc_narrow(vote_status);   // after it, against the balances it left
  r.take0 = cand && b < t_index ? 1 : 0;   // into the chain's PendingAttestations, which stateRecalc reads and prunes
  r.take1 = cand && b >= t_index ? 1 : 0;  // into the new ActiveState (core.go:223-237 after :398-497), T's own rows first
  return r;
}

}  // namespace pz
