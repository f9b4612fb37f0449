// What the resident objects show each other inside the library: pz_dev_state_recalc (recalc.hip)
// reads the vote cache's table (votecache.hip) and the pool's live columns and counts (attpool.hip)
// where they lie.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/prysm_hip.h"

namespace pz {

// The vote cache's lookup side: device pointers, valid for the handle's lifetime.
struct VcView {
  int device;
  uint64_t nval;
  uint32_t slot_cap, cells;
  const uint32_t* table;
  const uint8_t* keys;
  const uint32_t* nslots;
  const uint64_t* totals;
};
// Fills *v and records s as the stream the cache's reads wait for.
int vote_cache_view(pz_vote_cache* h, VcView* v, hipStream_t s);

// The pool's live buffer set and its device counts ([7], rows first), valid until the next prune.
struct ApView {
  int device;
  uint64_t rows_cap, rows_ub;
  pz_attestation_cols cols;
  const uint32_t* committee;
  const uint32_t* shard32;
  const uint64_t* counts;
};
// Fills *v and records s as the stream the pool's reads wait for.
int att_pool_peek(pz_att_pool* h, ApView* v, hipStream_t s);
// The exact row count the host has just read: the next prune's grid.
void att_pool_note_rows(pz_att_pool* h, uint64_t rows);

}  // namespace pz
