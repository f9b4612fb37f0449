// The attestation store's rule (blockstore.hip), stated once as host/device inlines: which rows of a
// run of received blocks blockProcessing writes to the database -- saveAttestation under
// Attestation.Key() (blockchain/service.go:288-290, core.go:650-658) and saveAttestationHash, which
// appends Attestation.Hash() to the block's AttestationHashes list (service.go:291-297,
// core.go:745-760) -- and how an appended list entry is encoded (messages.proto:128-130).
//
// Row r of block j = att_block[r] is SAVED when all of these hold:
//   1. j < stop: a deferred block is written by the call that processes it;
//   2. the block decoded: its status with every record's status folded in is PZ_OK.  A block with a
//      non-canonical block or record is refused whole, as everywhere in this library: the reference
//      would parse such bytes leniently, this library does not take them;
//   3. parent_ok[j]: hasBlock(block.ParentHash()) or slot <= 1 (service.go:261-269);
//   4. att_status[r] == PZ_ATT_PROCESSED and the row's record status is PZ_OK: processAttestation
//      returned nil (service.go:282-286).
// It does NOT depend on
//   * CanProcessBlock (`eligible`): its result is tested at service.go:308, after the saves at
//     :288-297 -- an ineligible block saves its accepted rows;
//   * the outcome of the block's last attestation: canProcessAttestations is tested at :304, after
//     the saves too -- a block whose last attestation fails saves the rows that passed before it.
// The kernels and the stand-alone CPU check (tests/blockstore_san.cpp, plain g++ under ASan+UBSan)
// compile the same text.  No HIP types.
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

// Conditions 1-3: block j writes its accepted rows.  A row whose att_block names no block of the
// run (j >= nblocks) is never saved.
PZ_HD bool bs_block_saves(uint64_t j, uint64_t nblocks, uint64_t stop, const int32_t* block_status, const uint8_t* parent_ok) {
  return j < nblocks && j < stop && block_status[j] == PZ_OK && parent_ok[j] != 0;
}

// Row r is saved (rec_status optional: NULL means every record decoded).
PZ_HD bool bs_row_saved(uint64_t r, uint64_t nblocks, uint64_t stop, const uint32_t* att_block, const int32_t* block_status,
                        const uint8_t* parent_ok, const int32_t* att_status, const int32_t* rec_status) {
  if (att_status[r] != PZ_ATT_PROCESSED || (rec_status && rec_status[r] != PZ_OK)) return false;
  return bs_block_saves(att_block[r], nblocks, stop, block_status, parent_ok);
}

// first[j], the rank at att_first[j]: rank[] holds every row's exclusive rank and the count at
// [natt].  An att_first past natt names no row and reads the count.
PZ_HD uint64_t bs_first(const uint32_t* rank, uint64_t att_first_j, uint64_t natt) { return rank[att_first_j < natt ? att_first_j : natt]; }

// ---- the appended list entries: entry i is 0a 20 | hash[i] (field 1, length 32) ----------------------
constexpr uint64_t kBsEntry = 34;
PZ_HD uint64_t bs_list_bytes(uint64_t m) { return kBsEntry * m; }
PZ_HD uint64_t bs_list_dwords(uint64_t m) { return (kBsEntry * m + 3) / 4; }
// The last dword of an odd m holds two entry bytes only: its lane stores a halfword.
PZ_HD bool bs_list_whole(uint64_t d, uint64_t m) { return 4 * d + 4 <= kBsEntry * m; }

PZ_HD uint32_t bs_load16(const uint8_t* p) {
  uint16_t v;
  __builtin_memcpy(&v, p, 2);
  return v;
}
PZ_HD uint32_t bs_load32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// Dword d (little-endian) of the entries' byte stream over hash[m][32].  34 and 4 are both even, so a
// dword starts at an even offset o of its entry e: o == 0 holds the two header bytes and two hash
// bytes, 2 <= o <= 30 four hash bytes, o == 32 the entry's last two hash bytes and the next entry's
// header.  Reads hash bytes of entry e only, all inside [32 e, 32 e + 32).
PZ_HD uint32_t bs_list_dword(const uint8_t* hash, uint64_t d) {
  const uint64_t at = 4 * d, e = at / kBsEntry;
  const uint32_t o = (uint32_t)(at - e * kBsEntry);
  const uint8_t* h = hash + 32 * e;
  if (o == 0) return 0x200au | bs_load16(h) << 16;
  if (o == 32) return bs_load16(h + 30) | 0x200au << 16;
  return bs_load32(h + (o - 2));
}

}  // namespace pz
