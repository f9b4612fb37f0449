// Attestation Key and processAttestation message digests from device columns, for gfx950.
//
//   Key      types/attestation.go:61-77   hdr10 | ShardBlockHash | copy32(e) per oblique hash e
//   message  blockchain/core.go:277-290   hdr10 | 64 x (parent | ' ') | ShardBlockHash
//
// Neither message exists in memory: one lane per attestation assembles each 128-byte block in
// its own LDS row (33-dword stride: conflict-free, and no workgroup barrier, since a lane only
// touches its row) from the columns pz_dev_unwire_attestations leaves on the device, then
// compresses it (blake2b_dev.h).  A block is a run of at most six "pieces", each at most 32
// source bytes with a place in the block: the element offsets of every piece are loaded first,
// then the aligned dwords under every piece, and only then is anything placed (two round
// trips per block, not one per byte).  A piece is shifted from its source alignment to its
// row alignment in registers (v_alignbit) and ORed into the zeroed row as whole dwords
// (ds_or_b32), so a piece costs 9 LDS operations whatever its alignment.
// Memory contract (the CSR hash form's): 4 readable bytes past the last byte of each bytes
// column; only aligned dwords that overlap a piece's own bytes are read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "att_cols.h"
#include "attdigest.h"
#include "blake2b_dev.h"
#include "resident.h"

namespace pz {
namespace {

constexpr int kThreads = 256;
constexpr int kRowWords = 33;
constexpr uint32_t kHdr = 10;

// len (<= 32) bytes at a source address, landing at byte `pos` of the current block
// (-32 .. 127: a piece may start before the block or run past it).
struct Piece {
  const uint32_t* base;  // the aligned dword that holds the first byte
  uint32_t sa;           // the first byte's bit offset in it (0, 8, 16, 24)
  uint32_t len;          // 0: nothing to load, nothing to place
  int pos;
};

__device__ __forceinline__ Piece make_piece(const uint8_t* src, uint32_t len, int pos) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(src);
  Piece p;
  p.base = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  p.sa = (uint32_t)(a & 3) * 8;
  p.len = len;
  p.pos = pos;
  return p;
}

__device__ __forceinline__ Piece no_piece() {
  Piece p;
  p.base = nullptr;
  p.sa = p.len = 0;
  p.pos = 0;
  return p;
}

// The (at most 9) aligned dwords that overlap the piece's bytes.
__device__ __forceinline__ void load_piece(const Piece& p, uint32_t w[9]) {
  const uint32_t ndw = p.len ? ((p.sa >> 3) + p.len + 3) >> 2 : 0u;
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = (uint32_t)k < ndw ? p.base[k] : 0u;
}

__device__ __forceinline__ void or_word(uint32_t* p, uint32_t v) {
  (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// OR the piece into the (zeroed) row: bytes past len are masked off, so pieces may share a dword.
__device__ __forceinline__ void place_piece(uint32_t* row, const Piece& p, const uint32_t w[9]) {
  if (!p.len) return;
  uint32_t d[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t x = p.sa ? __builtin_amdgcn_alignbit(w[k + 1], w[k], p.sa) : w[k];
    const uint32_t lo = 4u * k;
    const uint32_t valid = p.len <= lo ? 0u : (p.len >= lo + 4 ? 4u : p.len - lo);
    d[k] = x & (valid >= 4 ? 0xffffffffu : ((1u << (8 * valid)) - 1u));
  }
  const uint32_t s = (uint32_t)p.pos & 3u;
  const int w0 = p.pos >> 2;  // (arithmetic: a piece that starts before the block has w0 < 0)
  const uint32_t sh = (32u - 8u * s) & 31u;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const uint32_t lo = q > 0 ? d[q - 1] : 0u, hi = q < 8 ? d[q] : 0u;
    const uint32_t v = s ? __builtin_amdgcn_alignbit(hi, lo, sh) : hi;
    if ((unsigned)(w0 + q) < 32u) or_word(row + (w0 + q), v);
  }
}

// encoding/binary.PutUvarint(buf[0:10], x): bytes 0..7 in lo, 8..9 in hi, n of them.
__device__ __forceinline__ void uvarint10(uint64_t x, uint64_t& lo, uint32_t& hi, uint32_t& n) {
  lo = 0;
  hi = 0;
  n = 1;
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const uint64_t rest = x >> (7 * k);
    if (k > 0 && rest == 0) continue;
    uint32_t b = (uint32_t)rest & 0x7fu;
    if (k < 9 && (rest >> 7) != 0) b |= 0x80u;
    if (k < 8) lo |= (uint64_t)b << (8 * k);
    else hi |= b << (8 * (k - 8));
    n = (uint32_t)k + 1;
  }
}

// The 10-byte header both messages start with: PutUvarint(first) at offset 0, then
// PutUvarint(shard_id) at offset 0 over it (attestation.go:64-65, core.go:279,288): where the
// shard id's varint is the shorter one, the tail of the first one stays.
__device__ __forceinline__ void header10(uint64_t first, uint64_t shard_id, uint32_t hw[3]) {
  uint64_t flo, slo;
  uint32_t fhi, shi, fn, sn;
  uvarint10(first, flo, fhi, fn);
  uvarint10(shard_id, slo, shi, sn);
  const uint64_t mlo = sn >= 8 ? ~0ull : ((1ull << (8 * sn)) - 1ull);
  const uint32_t mhi = sn <= 8 ? 0u : (sn == 9 ? 0xffu : 0xffffu);
  const uint64_t lo = slo | (flo & ~mlo);
  hw[0] = (uint32_t)lo;
  hw[1] = (uint32_t)(lo >> 32);
  hw[2] = shi | (fhi & ~mhi);
}

__device__ __forceinline__ void zero_row(uint32_t* row) {
#pragma unroll
  for (int k = 0; k < 32; ++k) row[k] = 0;
}

__device__ __forceinline__ void compress_row(uint64_t h[8], const uint32_t* row, uint64_t ctr, bool last) {
  uint64_t mw[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) mw[k] = pack(row[2 * k], row[2 * k + 1]);
  compress(h, mw, ctr, last);
}

__device__ __forceinline__ void store_zero(uint8_t* out, uint32_t out_bytes) {
  const uint64_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  store_digest(out, z, out_bytes);
}

struct KeyArgs {
  const uint64_t *slot, *shard_id;
  const uint8_t* sbh;
  const uint64_t* sbh_offs;
  const uint8_t* obl;
  const uint64_t *ooffs, *first;
  const int32_t* rec_status;
  uint64_t n;
  uint8_t* out;
  uint32_t out_bytes;
};

// ------------------------------------------------------------------------------------------
// Key: hdr10 | ShardBlockHash (sl bytes, any length) | m x 32 bytes (copy32 of each element).
// Pieces: the ShardBlockHash in 32-byte chunks (nc = ceil(sl / 32), the last one short), then
// the elements; piece j < nc sits at 10 + 32 j, piece nc + e at 10 + sl + 32 e.  A 128-byte
// block overlaps at most six of them (every piece but the short chunk is 32 bytes wide).
// ------------------------------------------------------------------------------------------
constexpr int kKeyPieces = 6;

// kList false: output row o is the Key of row o of the columns (pz_[dev_]attestation_keys).  true: of
// row list[o] of the columns' nsrc rows (launch_att_keys_rows: the attestation store's saved rows,
// blockstore.hip); a list entry that names no row gets a zero key.  A template, so that both compile
// the one text and the plain form compiles to what it did as a plain kernel.
template <bool kList>
__global__ void __launch_bounds__(kThreads) pz_att_key_kernel(KeyArgs a, const uint32_t* list, uint64_t nsrc) {
  __shared__ uint32_t rows[kThreads * kRowWords];
  const uint64_t o = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (o >= a.n) return;  // no block-wide barrier below: lanes only touch their own row
  uint8_t* out = a.out + o * a.out_bytes;
  uint64_t i = o;
  if constexpr (kList) {
    i = list[o];
    if (i >= nsrc) {
      store_zero(out, a.out_bytes);
      return;
    }
  }
  if (a.rec_status && a.rec_status[i] != PZ_OK) {
    store_zero(out, a.out_bytes);
    return;
  }
  uint32_t* row = rows + threadIdx.x * kRowWords;
  uint64_t sbo = 0, sl = 0, f0 = 0, m = 0;
  if (a.sbh_offs) {
    sbo = a.sbh_offs[i];
    sl = a.sbh_offs[i + 1] - sbo;
  }
  if (a.first) {
    f0 = a.first[i];
    m = a.first[i + 1] - f0;
  }
  uint32_t hw[3];
  header10(a.slot ? a.slot[i] : 0, a.shard_id ? a.shard_id[i] : 0, hw);
  const uint64_t nc = (sl + 31) >> 5;
  const uint64_t el0 = kHdr + sl;  // where the elements start
  const uint64_t len = el0 + 32 * m;
  const uint64_t nblocks = (len + 127) / 128;
  uint64_t h[8];
  init_h(h);
  for (uint64_t t = 0; t < nblocks; ++t) {
    const uint64_t base = t * 128;
    // the first piece that ends after base
    uint64_t ja;
    if (base < el0) {
      ja = base < kHdr + 32 ? 0 : (base - (kHdr + 32)) / 32 + 1;
    } else {
      const uint64_t eb = base - el0;
      ja = nc + (eb < 32 ? 0 : (eb - 32) / 32 + 1);
    }
    // round trip 1: the element offsets of every piece in the block
    bool on[kKeyPieces], is_el[kKeyPieces];
    uint64_t at[kKeyPieces], lo[kKeyPieces], hi[kKeyPieces];
#pragma unroll
    for (int q = 0; q < kKeyPieces; ++q) {
      const uint64_t j = ja + q;
      is_el[q] = j >= nc;
      at[q] = is_el[q] ? el0 + 32 * (j - nc) : kHdr + 32 * j;
      on[q] = j < nc + m && at[q] < base + 128;
      lo[q] = hi[q] = 0;
      if (on[q] && is_el[q]) {
        lo[q] = a.ooffs[f0 + (j - nc)];
        hi[q] = a.ooffs[f0 + (j - nc) + 1];
      }
    }
    Piece pc[kKeyPieces];
#pragma unroll
    for (int q = 0; q < kKeyPieces; ++q) {
      const uint64_t j = ja + q;
      if (!on[q]) {
        pc[q] = no_piece();
      } else if (is_el[q]) {  // copy32: the first min(len, 32) bytes, zero-padded on the right
        const uint64_t l = hi[q] - lo[q];
        pc[q] = make_piece(a.obl + lo[q], l < 32 ? (uint32_t)l : 32u, (int)(int64_t)(at[q] - base));
      } else {
        const uint64_t l = sl - 32 * j;
        pc[q] = make_piece(a.sbh + sbo + 32 * j, l < 32 ? (uint32_t)l : 32u, (int)(int64_t)(at[q] - base));
      }
    }
    // round trip 2: every dword under every piece
    uint32_t w[kKeyPieces][9];
#pragma unroll
    for (int q = 0; q < kKeyPieces; ++q) load_piece(pc[q], w[q]);
    zero_row(row);
    if (t == 0) {
      row[0] = hw[0];
      row[1] = hw[1];
      row[2] = hw[2];
    }
#pragma unroll
    for (int q = 0; q < kKeyPieces; ++q) place_piece(row, pc[q], w[q]);
    const bool last = (t + 1 == nblocks);
    compress_row(h, row, last ? len : base + 128, last);
  }
  store_digest(out, h, a.out_bytes);
}

// ------------------------------------------------------------------------------------------
// processAttestation message: hdr10 | 64 x (parent_r | ' ') | ShardBlockHash, for the rows
// whose check status is PZ_ATT_PROCESSED.  Parent r < 64 - m is recent[parents_start + r]; the
// last m are the record's oblique elements under common.BytesToHash (right-aligned: the last
// 32 bytes of a longer one, zeros before a shorter one).  Pieces: parent r at 10 + 33 r (its
// separator at + 32), then the ShardBlockHash in 32-byte chunks from 2,122 on; a 128-byte
// block overlaps at most five (every piece before the last chunk is at least 32 bytes wide).
// ------------------------------------------------------------------------------------------
constexpr int kMsgPieces = 5;
constexpr uint64_t kParents = 64, kParentRec = 33;
constexpr uint64_t kSbhAt = kHdr + kParents * kParentRec;  // 2,122

extern "C" __global__ void __launch_bounds__(kThreads) pz_att_msg_kernel(pz_att_msg_batch b) {
  __shared__ uint32_t rows[kThreads * kRowWords];
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= b.natt) return;  // no block-wide barrier below
  uint8_t* out = b.out + i * 64;
  bool proc = b.status[i] == PZ_ATT_PROCESSED;
  uint64_t f0 = 0, m = 0, ps = 0;
  if (proc) {
    ps = b.parents_start[i];
    if (b.oblique_first) {
      f0 = b.oblique_first[i];
      m = b.oblique_first[i + 1] - f0;
    }
    // (what the checks guarantee for a PROCESSED row, core.go:348-360; a row that breaks it
    // is treated as not processed, so nothing outside recent[] is ever read)
    if (m > kParents || ps > b.n_recent || kParents - m > b.n_recent - ps) proc = false;
  }
  if (!proc) {
    store_zero(out, 64);
    if (b.msg_len) b.msg_len[i] = 0;
    return;
  }
  uint32_t* row = rows + threadIdx.x * kRowWords;
  const uint64_t nrec = kParents - m;  // parents taken from recent[]
  uint64_t sbo = 0, sl = 0;
  if (b.shard_block_hash_offs) {
    sbo = b.shard_block_hash_offs[i];
    sl = b.shard_block_hash_offs[i + 1] - sbo;
  }
  uint32_t hw[3];
  header10((b.slot ? b.slot[i] : 0) % kParents, b.shard_id ? b.shard_id[i] : 0, hw);
  const uint64_t nc = (sl + 31) >> 5;
  const uint64_t len = kSbhAt + sl;
  const uint64_t nblocks = (len + 127) / 128;
  uint64_t h[8];
  init_h(h);
  for (uint64_t t = 0; t < nblocks; ++t) {
    const uint64_t base = t * 128;
    uint64_t ja;  // the first piece whose 33- or 32-byte slot ends after base
    if (base < kSbhAt) {
      ja = base < kHdr + kParentRec ? 0 : (base - (kHdr + kParentRec)) / kParentRec + 1;
    } else {
      const uint64_t cb = base - kSbhAt;
      ja = kParents + (cb < 32 ? 0 : (cb - 32) / 32 + 1);
    }
    // round trip 1: the offsets of the oblique elements among the block's parents
    bool on[kMsgPieces], is_par[kMsgPieces], is_el[kMsgPieces];
    uint64_t at[kMsgPieces], lo[kMsgPieces], hi[kMsgPieces];
#pragma unroll
    for (int q = 0; q < kMsgPieces; ++q) {
      const uint64_t j = ja + q;
      is_par[q] = j < kParents;
      at[q] = is_par[q] ? kHdr + kParentRec * j : kSbhAt + 32 * (j - kParents);
      on[q] = (is_par[q] || j - kParents < nc) && at[q] < base + 128;
      is_el[q] = on[q] && is_par[q] && j >= nrec;
      lo[q] = hi[q] = 0;
      if (is_el[q]) {
        lo[q] = b.oblique_offs[f0 + (j - nrec)];
        hi[q] = b.oblique_offs[f0 + (j - nrec) + 1];
      }
    }
    Piece pc[kMsgPieces];
#pragma unroll
    for (int q = 0; q < kMsgPieces; ++q) {
      const uint64_t j = ja + q;
      const int pos = (int)(int64_t)(at[q] - base);
      if (!on[q]) {
        pc[q] = no_piece();
      } else if (is_el[q]) {  // BytesToHash: right-aligned in its 32 bytes
        const uint64_t l = hi[q] - lo[q];
        if (l >= 32) pc[q] = make_piece(b.oblique_parent_hashes + (hi[q] - 32), 32u, pos);
        else pc[q] = make_piece(b.oblique_parent_hashes + lo[q], (uint32_t)l, pos + 32 - (int)l);
      } else if (is_par[q]) {
        pc[q] = make_piece(b.recent + (ps + j) * 32, 32u, pos);
      } else {
        const uint64_t c = j - kParents, l = sl - 32 * c;
        pc[q] = make_piece(b.shard_block_hash + sbo + 32 * c, l < 32 ? (uint32_t)l : 32u, pos);
      }
    }
    // round trip 2: every dword under every piece
    uint32_t w[kMsgPieces][9];
#pragma unroll
    for (int q = 0; q < kMsgPieces; ++q) load_piece(pc[q], w[q]);
    zero_row(row);
    if (t == 0) {
      row[0] = hw[0];
      row[1] = hw[1];
      row[2] = hw[2];
    }
#pragma unroll
    for (int q = 0; q < kMsgPieces; ++q) {
      place_piece(row, pc[q], w[q]);
      const int sp = (int)(int64_t)(at[q] - base) + 32;  // the parent's ' '
      if (on[q] && is_par[q] && (unsigned)sp < 128u) or_word(row + (sp >> 2), 0x20u << (8 * (sp & 3)));
    }
    const bool last = (t + 1 == nblocks);
    compress_row(h, row, last ? len : base + 128, last);
  }
  store_digest(out, h, 64);
  if (b.msg_len) b.msg_len[i] = (uint32_t)len;
}

// ---- launchers and argument checks -----------------------------------------------------------
// Both forms; 1: nothing to do.
int check_key_args(const pz_attestation_cols* a, uint64_t n, const uint8_t* out, uint32_t out_bytes) {
  if (out_bytes != 32 && out_bytes != 64) return fail(PZ_EINVAL, "out_bytes must be 32 or 64");
  if (n == 0) return 1;
  if (!a || !out) return fail(PZ_EINVAL, "null pointer");
  if (a->shard_block_hash_offs && !a->shard_block_hash) return fail(PZ_EINVAL, "shard_block_hash is null");
  if (a->oblique_first && (!a->oblique_offs || !a->oblique_parent_hashes))
    return fail(PZ_EINVAL, "oblique_first without oblique_offs / oblique_parent_hashes");
  return PZ_OK;
}

hipError_t launch_att_keys(const pz_attestation_cols& a, uint64_t n, const int32_t* rec_status, uint8_t* out,
                           uint32_t out_bytes, hipStream_t s) {
  KeyArgs k{a.slot, a.shard_id, a.shard_block_hash, a.shard_block_hash_offs, a.oblique_parent_hashes,
            a.oblique_offs, a.oblique_first, rec_status, n, out, out_bytes};
  hipLaunchKernelGGL(pz_att_key_kernel<false>, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, k,
                     (const uint32_t*)nullptr, (uint64_t)0);
  return hipGetLastError();
}

// Both forms, what can be told without reading a column; 1: nothing to do.
int check_msg_args(const pz_att_msg_batch* b) {
  if (!b) return fail(PZ_EINVAL, "batch is null");
  if (b->natt == 0) return 1;
  if (!b->status || !b->parents_start || !b->out) return fail(PZ_EINVAL, "null status / parents_start / out");
  if (b->shard_block_hash_offs && !b->shard_block_hash) return fail(PZ_EINVAL, "shard_block_hash is null");
  if (b->oblique_first && (!b->oblique_offs || !b->oblique_parent_hashes))
    return fail(PZ_EINVAL, "oblique_first without oblique_offs / oblique_parent_hashes");
  return PZ_OK;
}

hipError_t launch_att_msgs(const pz_att_msg_batch& b, hipStream_t s) {
  hipLaunchKernelGGL(pz_att_msg_kernel, dim3((uint32_t)((b.natt + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                     b);
  return hipGetLastError();
}

// The host forms' validation of the columns both messages read (kAttKeyCols), before they are staged.
int check_key_cols(const pz_attestation_cols& a, uint64_t n) {
  int rc;
  if (a.shard_block_hash_offs && (rc = check_csr(a.shard_block_hash_offs, n, "shard_block_hash"))) return rc;
  if (a.oblique_first) {
    if ((rc = check_csr(a.oblique_first, n, "oblique_first"))) return rc;
    if ((rc = check_csr(a.oblique_offs + a.oblique_first[0], a.oblique_first[n] - a.oblique_first[0], "oblique"))) return rc;
  }
  return PZ_OK;
}

}  // namespace

// attdigest.h: Key through a row list, for the attestation store (blockstore.hip).
hipError_t launch_att_keys_rows(const pz_attestation_cols& a, uint64_t nsrc, const uint32_t* list, uint64_t n, uint8_t* out,
                                hipStream_t s) {
  KeyArgs k{a.slot, a.shard_id, a.shard_block_hash, a.shard_block_hash_offs, a.oblique_parent_hashes,
            a.oblique_offs, a.oblique_first, nullptr, n, out, 32};
  hipLaunchKernelGGL(pz_att_key_kernel<true>, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, k, list, nsrc);
  return hipGetLastError();
}

int check_att_key_cols(const pz_attestation_cols* a, uint64_t n, bool host_form) {
  if (!a) return fail(PZ_EINVAL, "columns are null");
  if (a->shard_block_hash_offs && !a->shard_block_hash) return fail(PZ_EINVAL, "shard_block_hash is null");
  if (a->oblique_first && (!a->oblique_offs || !a->oblique_parent_hashes))
    return fail(PZ_EINVAL, "oblique_first without oblique_offs / oblique_parent_hashes");
  return host_form ? check_key_cols(*a, n) : PZ_OK;
}

}  // namespace pz

using namespace pz;

extern "C" {

int pz_dev_attestation_keys(const pz_attestation_cols* a, uint64_t n, const int32_t* d_rec_status, uint8_t* d_out,
                            uint32_t out_bytes, void* stream) {
  int rc = check_key_args(a, n, d_out, out_bytes);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!aligned16(d_out)) return fail(PZ_EINVAL, "d_out must be 16-B aligned");
  hipError_t e = launch_att_keys(*a, n, d_rec_status, d_out, out_bytes, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_att_key_kernel");
}

int pz_attestation_keys(const pz_attestation_cols* a, uint64_t n, uint8_t* out, uint32_t out_bytes) {
  int rc = check_key_args(a, n, out, out_bytes);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if ((rc = check_key_cols(*a, n))) return rc;
  HostForm f;  // (no handle: the current device's context)
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_attestation_cols dc;
  stage_att_cols(st, *a, n, kAttKeyCols, &dc);
  uint8_t* d_out = st.up<uint8_t>(nullptr, n * out_bytes);
  if (st.rc) return st.rc;
  st.check(launch_att_keys(dc, n, nullptr, d_out, out_bytes, st.s), "pz_att_key_kernel");
  st.down(out, d_out, n * out_bytes);
  return st.sync();
}

int pz_dev_attestation_messages(const pz_att_msg_batch* b, void* stream) {
  int rc = check_msg_args(b);
  if (rc) return rc < 0 ? rc : PZ_OK;
  // (the statuses are on the device: the rule "n_recent >= 64 where a row is PROCESSED" is
  // applied to the whole batch here, before the launch)
  if (b->n_recent < kParents) return fail(PZ_EINVAL, "n_recent %llu < 64", (unsigned long long)b->n_recent);
  if (!b->recent) return fail(PZ_EINVAL, "recent is null");
  if (!aligned16(b->out)) return fail(PZ_EINVAL, "out must be 16-B aligned");
  hipError_t e = launch_att_msgs(*b, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_att_msg_kernel");
}

int pz_attestation_messages(const pz_att_msg_batch* hb) {
  int rc = check_msg_args(hb);
  if (rc) return rc < 0 ? rc : PZ_OK;
  const uint64_t n = hb->natt;
  bool any = false;
  for (uint64_t i = 0; i < n && !any; ++i) any = hb->status[i] == PZ_ATT_PROCESSED;
  if (any && hb->n_recent < kParents)
    return fail(PZ_EINVAL, "n_recent %llu < 64 with a PROCESSED row", (unsigned long long)hb->n_recent);
  if (any && !hb->recent) return fail(PZ_EINVAL, "recent is null");
  pz_attestation_cols hc{}, d;  // the batch's same-named members
  hc.slot = hb->slot, hc.shard_id = hb->shard_id;
  hc.shard_block_hash = hb->shard_block_hash, hc.shard_block_hash_offs = hb->shard_block_hash_offs;
  hc.oblique_parent_hashes = hb->oblique_parent_hashes, hc.oblique_offs = hb->oblique_offs, hc.oblique_first = hb->oblique_first;
  if ((rc = check_key_cols(hc, n))) return rc;
  HostForm f;  // (no handle: the current device's context)
  if (f.rc) return f.rc;
  Stager& st = f.st;
  stage_att_cols(st, hc, n, kAttKeyCols, &d);
  pz_att_msg_batch db = *hb;
  db.slot = d.slot, db.shard_id = d.shard_id;
  db.shard_block_hash = d.shard_block_hash, db.shard_block_hash_offs = d.shard_block_hash_offs;
  db.oblique_parent_hashes = d.oblique_parent_hashes, db.oblique_offs = d.oblique_offs, db.oblique_first = d.oblique_first;
  db.status = st.up(hb->status, n);
  db.parents_start = st.up(hb->parents_start, n);
  db.recent = st.up(hb->recent, hb->recent ? hb->n_recent * 32 : 0);
  db.out = st.up<uint8_t>(nullptr, n * 64);
  db.msg_len = hb->msg_len ? st.up<uint32_t>(nullptr, n) : nullptr;
  if (st.rc) return st.rc;
  st.check(launch_att_msgs(db, st.s), "pz_att_msg_kernel");
  st.down(hb->out, db.out, n * 64);
  if (hb->msg_len) st.down(hb->msg_len, db.msg_len, n);
  return st.sync();
}

}  // extern "C"
