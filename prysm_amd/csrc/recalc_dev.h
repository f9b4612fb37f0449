// The pure rules of the resident cycle transition (recalc.hip), as host/device inlines: the
// justification loop of stateRecalc (blockchain/core.go:411-431) over a 64-bit mask, the commit's
// panic decision and its clamps.  The kernels and the stand-alone CPU check (tests/recalc_san.cpp,
// plain g++ under ASan+UBSan) compile the same text.
#pragma once
#include <stdint.h>

#include "../../include/prysm_hip.h"
#include "votecache_dev.h"

namespace pz {

// The sticky error word's bits.
constexpr uint64_t kRsErrPanic = 1;  // where stateRecalc panics (processCrosslinks / CalculateRewards)

constexpr uint32_t kRsNoWinner = 0xFFFFFFFFu;
constexpr uint32_t kRsMinStride = 32, kRsMaxStride = 256;

PZ_HD bool rs_stride_ok(uint32_t stride) { return stride >= kRsMinStride && stride <= kRsMaxStride && stride % 16 == 0; }

// core.go:419 for one slot: 3 * blockVoteBalance >= 2 * TotalDeposits, both products mod 2^64.
PZ_HD bool rs_slot_passes(uint64_t vote_total, uint64_t total_deposits) { return 3 * vote_total >= 2 * total_deposits; }

struct RsJustified {
  uint64_t streak, justified, finalized;  // JustifiedStreak, LastJustifiedSlot, LastFinalizedSlot
};

// core.go:411-431 over the mask whose bit i is rs_slot_passes of RecentBlockHashes()[i]:
// slot = lastStateRecalc - 64 + i and slot - 64 wrap as Go's uint64 does.
PZ_HD RsJustified rs_justify(uint64_t mask, uint64_t last_state_recalc, RsJustified s) {
  for (uint64_t i = 0; i < PZ_CYCLE_LENGTH; ++i) {
    const uint64_t slot = last_state_recalc - PZ_CYCLE_LENGTH + i;
    if ((mask >> i) & 1) {
      if (slot > s.justified) s.justified = slot;
      s.streak += 1;
    } else {
      s.streak = 0;
    }
    if (s.streak >= PZ_CYCLE_LENGTH + 1 && slot - PZ_CYCLE_LENGTH > s.finalized) s.finalized = slot - PZ_CYCLE_LENGTH;
  }
  return s;
}

// Where the reference is dead after the epoch kernels: processCrosslinks' index panics
// (core.go:549, :367), or CalculateRewards' CheckBit (incentives.go:23) once the attesters'
// deposit reaches two thirds (pop * 32 * 3 >= 2 * TotalDeposits mod 2^64) with an active validator.
PZ_HD bool rs_panics(const uint64_t scal[PZ_SCAL_COUNT], uint64_t total_deposits) {
  if (scal[PZ_SCAL_ERR_XL] != 0) return true;
  const bool thr = scal[PZ_SCAL_POP] * PZ_DEFAULT_BALANCE * 3 >= total_deposits * 2;
  return thr && scal[PZ_SCAL_NACT] > 0 && scal[PZ_SCAL_ERR_RWD] != 0;
}

// A winner names a row the pool holds (checked before anything is read through it).
PZ_HD bool rs_row_ok(uint32_t row, uint64_t rows) { return row != kRsNoWinner && row < rows; }

// The bytes of a ShardBlockHash range [lo, hi) a record of `stride` bytes takes: an inverted range
// is empty, a longer one is cut (the fit check refuses the call before that can happen).
PZ_HD uint32_t rs_hash_len(uint64_t lo, uint64_t hi, uint32_t stride) {
  if (hi <= lo) return 0;
  return hi - lo > stride ? stride : (uint32_t)(hi - lo);
}

// The fit check's predicate for one pending row.
PZ_HD bool rs_row_fits(uint64_t lo, uint64_t hi, uint32_t stride) { return hi <= lo || hi - lo <= stride; }

}  // namespace pz
