// The parent check's rules (blockparents.hip), stated once as host/device inlines: blockProcessing's
// first decision per received block, hasBlock(block.ParentHash()) (blockchain/service.go:261-269,
// core.go:560-562), answered for a whole RUN of blocks from the set of saved block hashes
// (saveBlock, service.go:324, core.go:565-577) although the blocks of the run save each other as
// they go.  The kernels and the stand-alone CPU check (tests/blockparents_san.cpp, plain g++ under
// ASan+UBSan) compile the same text.  No HIP types.
//
// For block j of the run, in block order:
//   parent_j = BytesToHash of field 1 (the span bytes_beg[5j], bytes_len[5j] of pz_block_cols_out):
//              absent is the zero hash, a longer field keeps its last 32 bytes, a shorter one is
//              right-aligned (vc_bytes_to_hash).
//   hash_j   = Block.Hash().
//   free_j   = slot_j <= 1 (service.go:267).
//   open0_j  = the block gate would open block j if its parent were saved: block_status[j] == PZ_OK and
//              bg_report(...) != kBgRejected over the very columns the gate call that follows reads.
//              The gate's open decision looks at block j's own rows only (blockwalk_dev.h: "Which
//              blocks go on is the block gate's report"), so it can be taken before the parents are
//              known.  CanProcessBlock (service.go:272, :308) arrives folded into block_status.
//   link_j   = the largest i < j with hash_i == parent_j and open0_i, or none.
//   parent_ok_j = free_j or parent_j in the set or (link_j exists and saved_{link_j})       (:261-269)
//   saved_j     = open0_j and parent_ok_j                                                   (:324)
//
// Why the LARGEST open copy suffices.  Let i_1 < ... < i_k < j be the blocks before j whose hash is
// parent_j.  A copy with open0 false never reaches service.go:324, whatever its parent: it never
// saves.  The copies with open0 true hold the same bytes -- equal hashes are equal blocks -- so they
// share parent and slot, and differ only in what the caller folded into block_status, which open0
// already accounts for.  For such a copy i, saved_i = parent_ok_i, and parent_ok_i asks whether ONE
// fixed hash (their common parent) is in the DB before block i, or the slot is <= 1.  The DB only
// grows, so that answer is monotone in i: once one open copy is saved, every later open copy is.
// parent_j is in the DB before block j iff it was there before the run or some open copy before j
// was saved, and by monotonicity that is iff the LAST open copy before j was saved: link_j.
//
// Resolution.  Every block gets a word: kBpTrue, kBpFalse, or the index of the block whose word
// decides it (an index is < 2^31, so it never reads as either constant):
//   S_j = not open0_j -> false; free_j or in the set -> true; link_j exists -> link_j; else false.
//   P_j = the same without the first case: parent_ok_j, which is reported for closed blocks too.
// link_j < j, so the words form chains that end in a resolved word after at most j steps.  A round
// replaces every unresolved S_j by S_{S_j} (bp_jump): its state if that is resolved, else its
// pointer -- the distance covered doubles, so bp_rounds(nblocks) = ceil(log2 nblocks) rounds resolve
// every chain.  Rounds are double-buffered: round r reads one array and writes the other.  Then
// parent_ok_j = P_j if resolved, else S_{P_j}.
//
// The resident set (pz_block_set) is an open-addressing table of `cells` cells, a power of two:
// a state word a cell (so the all-zero hash is an ordinary key) beside 32 key bytes a cell; the
// home cell comes from the hash's first word (vc_home); linear probing, wrapping, at most `cells`
// steps.  The run table of launch 1 is the same shape with a block index a cell and no keys.
#pragma once
#include <stdint.h>

#include "blockgate_dev.h"
#include "blockwalk_dev.h"
#include "votecache_dev.h"

namespace pz {

// ---- the resolution words --------------------------------------------------------------------
constexpr uint32_t kBpTrue = 0xFFFFFFFFu, kBpFalse = 0xFFFFFFFEu;
constexpr uint32_t kBpNoLink = 0xFFFFFFFFu;

PZ_HD bool bp_resolved(uint32_t v) { return v >= kBpFalse; }
PZ_HD uint32_t bp_of(bool b) { return b ? kBpTrue : kBpFalse; }

// service.go:267: a block of slot 0 or 1 needs no parent.
PZ_HD bool bp_free(uint64_t slot) { return slot <= 1; }

// The span of field 1 names bytes of the buffer (len 0: absent, the zero hash).
PZ_HD bool bp_span_ok(uint64_t beg, uint32_t len, uint64_t nbytes) { return len == 0 || (beg <= nbytes && len <= nbytes - beg); }

PZ_HD Hash32 bp_parent(const uint8_t* bytes, uint64_t beg, uint32_t len) {
  return vc_bytes_to_hash(bytes, beg, beg + len);  // common.BytesToHash(block.data.ParentHash), types/block.go
}

// open0_j through the gate's own inlines, over the inputs the gate call that follows receives.
PZ_HD bool bp_open0(const uint64_t* att_first, const int32_t* block_status, const int32_t* rec_status,
                    const int32_t* att_status, uint64_t natt, uint64_t j) {
  const uint64_t f0 = att_first[j], f1 = att_first[j + 1];
  if (!bg_span_ok(f0, f1, natt)) return false;
  uint64_t nproc = 0;
  bool bad = false;
  for (uint64_t i = f0; i < f1; ++i) {
    if (rec_status && rec_status[i] != PZ_OK) bad = true;
    if (att_status[i] == PZ_ATT_PROCESSED) ++nproc;
  }
  const bool accepted = block_status[j] == PZ_OK && !bad;
  return bg_report(accepted, f1 - f0, nproc, f1 > f0 ? att_status[f1 - 1] : -1) != kBgRejected;
}

// P_j and S_j before the rounds.
PZ_HD uint32_t bp_parent_word(bool free, bool in_set, uint32_t link) {
  return free || in_set ? kBpTrue : link != kBpNoLink ? link : kBpFalse;
}
PZ_HD uint32_t bp_saved_word(bool open0, uint32_t parent_word) { return open0 ? parent_word : kBpFalse; }

PZ_HD uint32_t bp_rounds(uint64_t nblocks) {
  uint32_t r = 0;
  while ((1ull << r) < nblocks) ++r;
  return r;
}
// One round for one block: v = S_j, at_next = S_{S_j} (read only when v is unresolved).
PZ_HD uint32_t bp_jump(uint32_t v, uint32_t at_next) { return bp_resolved(v) ? v : at_next; }

// After the rounds: parent_ok_j from P_j and the resolved S (s_at_link = S_{P_j}, read only when
// P_j is a link).  A word the rounds left unresolved cannot exist; it would count as false.
PZ_HD bool bp_parent_ok(uint32_t parent_word, uint32_t s_at_link) {
  return bp_resolved(parent_word) ? parent_word == kBpTrue : s_at_link == kBpTrue;
}
PZ_HD int32_t bp_status_out(int32_t status_in, bool parent_ok) { return parent_ok ? status_in : PZ_ENOTFOUND; }

// ---- the run table -----------------------------------------------------------------------------
// cells = the smallest power of two >= 2 * nblocks, at least 2 and at most 2^31 (nblocks < 2^31, so
// an empty cell always exists); a cell holds kBpNoLink (empty) or a block index.  Launch 1 claims the first empty cell from the hash's home; equal hashes
// take cells of their own, so a probe for a hash walks on to the first empty cell and meets every
// copy.  At most nblocks cells are taken: an empty cell always ends the probe.  (One cell per hash
// holding its largest index would not do: block j needs the largest copy BEFORE j, which a copy
// after j would hide.  The price: a run of c copies of one block costs O(c) per probe.)
PZ_HD uint32_t bp_run_cells(uint64_t nblocks) {
  uint32_t c = 2;
  while (c < 2 * nblocks && c < (1u << 31)) c <<= 1;
  return c;
}
PZ_HD uint32_t bp_link(const uint32_t* run, uint32_t cells, const uint8_t* block_hash, const Hash32& parent, uint64_t j) {
  uint32_t link = kBpNoLink, c = vc_home(parent, cells);
  for (uint32_t step = 0; step < cells; ++step, c = vc_next(c, cells)) {
    const uint32_t i = run[c];
    if (i == kBpNoLink) break;
    if (i < j && (link == kBpNoLink || i > link) && vc_hash_eq(parent, vc_load_hash16(block_hash + 32ull * i))) link = i;
  }
  return link;
}

// ---- the resident set ---------------------------------------------------------------------------
// A cell's state word: empty, full, or -- only while an insert launch runs -- a tentative claim that
// carries the index of the input hash that made it (vc_claim).
constexpr uint32_t kBsEmpty = 0xFFFFFFFFu, kBsFull = 0;
constexpr uint32_t kBsMinCells = 8, kBsMaxKeys = 1u << 30;
constexpr uint64_t kBsErrCapacity = 2;  // the sticky error word's bit (as kVcErrCapacity)
enum { kBsCount = 0, kBsErr, kBsWords };  // the handle's words

PZ_HD uint32_t bs_cells(uint64_t min_keys) {
  uint32_t c = kBsMinCells;
  while (c < 2 * min_keys) c <<= 1;
  return c;
}
PZ_HD bool bs_is_claim(uint32_t v) { return v != kBsEmpty && (v & kVcTentative) != 0; }

// hasBlock (core.go:560-562) between calls (no launch writes the set meanwhile: plain loads).  At most
// `cells` steps; an empty cell ends the probe; a claim cannot exist between calls and is skipped.
PZ_HD bool bs_contains(const uint32_t* state, const uint8_t* keys, uint32_t cells, const Hash32& h) {
  uint32_t c = vc_home(h, cells);
  for (uint32_t step = 0; step < cells; ++step, c = vc_next(c, cells)) {
    const uint32_t v = state[c];
    if (v == kBsEmpty) return false;
    if (v == kBsFull && vc_hash_eq(h, vc_load_hash16(keys + 32ull * c))) return true;
  }
  return false;
}

// Which blocks pz_dev_block_set_insert_walked stores: the walk's saved and candidate blocks before
// `stop` (saveBlock, service.go:324, precedes the candidate rule), none when the gate's flag word
// says the reference panics in the run.
PZ_HD bool bp_insert_walked(uint8_t walk, uint32_t gate_flags) { return !(gate_flags & kBgPanic) && (walk == kBwSaved || walk == kBwCandidate); }

}  // namespace pz
