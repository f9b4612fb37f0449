// proto3 decoding of AttestationRecords and BeaconBlocks on the device: the inverse of
// wire_att.hip.
//
// Replaces golang/protobuf `proto.Unmarshal` at sync/service.go:147-164 (the received block,
// messages.pb.go:224-232) with the records inside it (messages.pb.go:889-896), under the
// engine's canonical-form rule.  proto3_canon.h is the single statement of that rule; the walks
// here are its visitors over the offset cursor, the engine's parser (chain.hip) its visitors
// over the pointer cursor.  A record that fails gets PZ_EINVAL and contributes nothing.
//
// Each decode is three launches, one lane per record, 256 records per workgroup (a tile):
//   size   walks the record, applies every rule, writes the fixed-size columns (scalars, status,
//          n_oblique, last_byte), the record's variable sizes and the tile's sums;
//   scan   one workgroup turns the tiles' sums into the tiles' bases (and the totals);
//   write  scans the tile's sizes again in the workgroup, adds the tile's base -- these are the
//          offsets columns, written once -- walks the record a second time and copies.
// No workgroup waits for another inside a launch (the encoder's size kernel orders its tiles by
// ticket and looks back; here the order between tiles is the order between launches), and the
// second walk reads the bytes the first one judged, so it stays inside the record.
//
// Reads: only bytes of [begs[i], ends[i]).  Writes: only inside the ranges the scans assign.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "att_cols.h"
#include "proto3_canon.h"
#include "resident.h"
#include "tile_scan.h"

namespace pz {
namespace {

constexpr int kAttCols = 7;  // d_totals' order: three bytes fields, elements, element bytes, sig values, bad records

// Launch 2 of both decodes: column c's tile sums tiles[c * ntiles ..] become the tiles'
// exclusive bases, totals[c] the column's sum.  One workgroup; a column is walked kScanThreads
// tiles at a time with a carry.
extern "C" __global__ void __launch_bounds__(kScanThreads) pz_unwire_scan_kernel(uint64_t* tiles, uint64_t ntiles,
                                                                                 uint32_t ncols, uint64_t* totals) {
  __shared__ uint64_t s_inc[kScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (uint32_t c = 0; c < ncols; ++c) {
    uint64_t* col = tiles + c * ntiles;
    uint64_t carry = 0;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += kScanThreads) {
      const uint64_t t = t0 + tid;
      const uint64_t x = t < ntiles ? col[t] : 0;
      const uint64_t inc = wscan(x);
      if (lane == 63) s_inc[w] = inc;
      __syncthreads();
      uint64_t before = 0, all = 0;
      for (int k = 0; k < kScanThreads / 64; ++k) {
        before += k < w ? s_inc[k] : 0;
        all += s_inc[k];
      }
      __syncthreads();  // (s_inc is rewritten by the next round)
      if (t < ntiles) col[t] = carry + before + inc - x;
      carry += all;
    }
    if (tid == 0) totals[c] = carry;
  }
}

// ---- AttestationRecord ------------------------------------------------------------------------
struct AttArgs {
  const uint8_t* d;
  const uint64_t* begs;
  const uint64_t* ends;
  uint64_t n, ntiles;
  uint32_t field;
  pz_attestation_cols_out o;
  uint64_t* sizes;  // [6][n]: columns 0-5 of d_totals' order
  uint64_t* tiles;  // [7][ntiles]
};

struct AttRec {
  uint64_t v[3];            // slot, shard_id, justified_slot
  uint64_t pos[3], len[3];  // fields 4-6: where the bytes are
  uint64_t nel, elb, nsig;  // elements, their bytes, packed values
};

// Where the second walk writes: the record's first element / element byte / sig value.
struct AttDst {
  uint64_t el, elb, sig;
};

// The record's visitor: fields into AttRec.  W: also write the elements and the sig values.
template <bool W>
struct AttVisit {
  const AttArgs& a;
  AttRec& r;
  const AttDst& dst;
  __device__ __forceinline__ bool scalar(uint32_t f, uint64_t v) {
#pragma unroll
    for (int k = 0; k < 3; ++k)  // (constant indices: the record stays in registers)
      if (f == 1u + k) r.v[k] = v;
    return true;
  }
  __device__ __forceinline__ bool bytes(uint32_t f, uint64_t q, uint64_t len) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (f == 4u + k) {
        r.pos[k] = q;
        r.len[k] = len;
      }
    return true;
  }
  __device__ __forceinline__ bool oblique(uint64_t q, uint64_t len) {
    if (W) {
      a.o.oblique_offs[dst.el + r.nel] = dst.elb + r.elb;
      copy_span(a.o.oblique_parent_hashes + dst.elb + r.elb, a.d + q, len);
    }
    ++r.nel;
    r.elb += len;
    return true;
  }
  __device__ __forceinline__ bool sig(uint64_t x) {
    if (W) a.o.aggregate_sig[dst.sig + r.nsig] = x;
    ++r.nsig;
    return true;
  }
};

template <bool W>
__device__ __forceinline__ bool walk_att(const AttArgs& a, uint64_t beg, uint64_t end, AttRec& r, const AttDst& dst) {
  r = AttRec{};
  if (end < beg) return false;
  canon::OffsetCursor<true> c = canon::OffsetCursor<true>::over(a.d, beg, end);
  if (a.field) {  // the frame: that field's key and a length that covers exactly the rest
    const uint64_t k = canon::get_varint(c);
    if (!c.ok || k != (((uint64_t)a.field << 3) | 2)) return false;
    const uint64_t len = canon::get_varint(c);
    if (!c.ok || len != c.left()) return false;
  }
  return canon::walk_attestation(c, AttVisit<W>{a, r, dst});
}

// (The two kernels' bodies stay functions of their own, inlined into the kernels: written into the
// kernels directly, the same statements compile to a different schedule.)
__device__ __forceinline__ void att_size_body(const AttArgs& a) {
  const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  uint64_t sz[kAttCols] = {0, 0, 0, 0, 0, 0, 0};
  if (i < a.n) {
    AttRec r;
    const bool ok = walk_att<false>(a, a.begs[i], a.ends[i], r, AttDst{});
    if (!ok) r = AttRec{};  // a record that fails contributes nothing
    a.o.slot[i] = r.v[0];
    a.o.shard_id[i] = r.v[1];
    a.o.justified_slot[i] = r.v[2];
    a.o.status[i] = ok ? PZ_OK : PZ_EINVAL;
    if (a.o.n_oblique) a.o.n_oblique[i] = r.nel;
    if (a.o.last_byte) a.o.last_byte[i] = r.len[2] ? a.d[r.pos[2] + r.len[2] - 1] : 0;
    sz[0] = r.len[0];
    sz[1] = r.len[1];
    sz[2] = r.len[2];
    sz[3] = r.nel;
    sz[4] = r.elb;
    sz[5] = r.nsig;
    sz[6] = !ok;
#pragma unroll
    for (int c = 0; c < kAttCols - 1; ++c) a.sizes[c * a.n + i] = sz[c];
  }
  tile_sums<kAttCols>(sz, a.tiles, a.ntiles);
}

extern "C" __global__ void __launch_bounds__(kTile) pz_unwire_att_size_kernel(AttArgs a) { att_size_body(a); }

__device__ __forceinline__ void att_write_body(const AttArgs& a) {
  const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  uint64_t sz[kAttCols - 1], at[kAttCols - 1];
#pragma unroll
  for (int c = 0; c < kAttCols - 1; ++c) sz[c] = i < a.n ? a.sizes[c * a.n + i] : 0;
  tile_excl<kAttCols - 1>(sz, at);
  if (i >= a.n) return;
#pragma unroll
  for (int c = 0; c < kAttCols - 1; ++c) at[c] += a.tiles[c * a.ntiles + blockIdx.x];
  uint64_t* const offs[kAttCols - 1] = {a.o.justified_block_hash_offs, a.o.shard_block_hash_offs,
                                        a.o.attester_bitfield_offs,    a.o.oblique_first,
                                        nullptr,                       a.o.aggregate_sig_first};
#pragma unroll
  for (int c = 0; c < kAttCols - 1; ++c) {
    if (!offs[c]) continue;
    offs[c][i] = at[c];
    if (i + 1 == a.n) offs[c][a.n] = at[c] + sz[c];
  }
  if (i + 1 == a.n) a.o.oblique_offs[at[3] + sz[3]] = at[4] + sz[4];  // the element CSR's end
  if (a.o.status[i] != PZ_OK) return;
  AttRec r;
  walk_att<true>(a, a.begs[i], a.ends[i], r, AttDst{at[3], at[4], at[5]});
  uint8_t* const dat[3] = {a.o.justified_block_hash, a.o.shard_block_hash, a.o.attester_bitfield};
#pragma unroll
  for (int k = 0; k < 3; ++k) copy_span(dat[k] + at[k], a.d + r.pos[k], r.len[k]);
}

extern "C" __global__ void __launch_bounds__(kTile) pz_unwire_att_write_kernel(AttArgs a) { att_write_body(a); }

int att_out_args(const pz_attestation_cols_out* o, uint64_t n, uint32_t field_num) {
  if (!o) return fail(PZ_EINVAL, "columns are null");
  if (field_num >= (1u << 29)) return fail(PZ_EINVAL, "field number %u out of range", field_num);
  if (n >> 38) return fail(PZ_EINVAL, "more than 2^38 records");  // (a tile per workgroup: the grid's limit)
  if (!o->justified_block_hash_offs || !o->shard_block_hash_offs || !o->attester_bitfield_offs || !o->oblique_offs ||
      !o->oblique_first || !o->aggregate_sig_first)
    return fail(PZ_EINVAL, "null offsets column");
  if (n && (!o->slot || !o->shard_id || !o->justified_slot || !o->justified_block_hash || !o->shard_block_hash ||
            !o->attester_bitfield || !o->oblique_parent_hashes || !o->aggregate_sig || !o->status))
    return fail(PZ_EINVAL, "null output column");
  return PZ_OK;
}


hipError_t launch_unwire_att(AttArgs a, uint64_t* totals, void* scratch, hipStream_t s) {
  hipError_t e;
  if (!a.n) {  // every offsets column is its first entry
    uint64_t* const first[] = {a.o.justified_block_hash_offs, a.o.shard_block_hash_offs, a.o.attester_bitfield_offs,
                               a.o.oblique_offs,              a.o.oblique_first,         a.o.aggregate_sig_first};
    for (uint64_t* p : first)
      if ((e = hipMemsetAsync(p, 0, 8, s)) != hipSuccess) return e;
    return hipMemsetAsync(totals, 0, kAttCols * 8, s);
  }
  a.ntiles = tiles_of(a.n);
  a.sizes = static_cast<uint64_t*>(scratch);
  a.tiles = a.sizes + (kAttCols - 1) * a.n;
  hipLaunchKernelGGL(pz_unwire_att_size_kernel, dim3((uint32_t)a.ntiles), dim3(kTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_tile_scan(a.tiles, a.ntiles, (uint32_t)kAttCols, totals, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(pz_unwire_att_write_kernel, dim3((uint32_t)a.ntiles), dim3(kTile), 0, s, a);
  return hipGetLastError();
}

// ---- BeaconBlock: the top level only ----------------------------------------------------------
struct BlockArgs {
  const uint8_t* d;
  const uint64_t* offs;
  uint64_t n, ntiles, att_cap;
  pz_block_cols_out o;
  uint64_t* counts;  // [n]
  uint64_t* tiles;   // [ntiles]
};

struct BlockRec {
  uint64_t slot;
  int64_t ts_seconds, ts_nanos;
  bool has_ts;
  uint64_t beg[5];  // fields 1, 3, 4, 5, 6
  uint32_t len[5];
  uint64_t natt;
};

// The block's visitor: the top level into BlockRec.  W: also the records' spans, rows first + j.
template <bool W>
struct BlockVisit {
  const BlockArgs& a;
  BlockRec& r;
  uint64_t i, first;
  __device__ __forceinline__ bool scalar(uint32_t, uint64_t v) {
    r.slot = v;
    return true;
  }
  __device__ __forceinline__ bool bytes(uint32_t f, uint64_t q, uint64_t len) {
    // Not part of the shared rule: bytes_len is a 32-bit column of this decoder alone (the
    // engine's parser holds a block's length in a size_t and keeps no such column).
    if (len > 0xffffffffull) return false;
#pragma unroll
    for (int s = 0; s < 5; ++s)  // fields 1, 3, 4, 5, 6 (constant indices: no private array)
      if (f == (s ? s + 2u : 1u)) {
        r.beg[s] = q;
        r.len[s] = (uint32_t)len;
      }
    return true;
  }
  __device__ __forceinline__ bool timestamp(int64_t seconds, int64_t nanos) {
    r.has_ts = true;
    r.ts_seconds = seconds;
    r.ts_nanos = nanos;
    return true;
  }
  __device__ __forceinline__ bool record(const canon::OffsetCursor<true>&, uint64_t q, uint64_t len) {
    const uint64_t row = first + r.natt;
    if (W && row < a.att_cap) {
      a.o.att_beg[row] = q;
      a.o.att_end[row] = q + len;
      a.o.att_block_slot[row] = r.slot;
      a.o.att_block[row] = (uint32_t)i;
    }
    ++r.natt;
    return true;
  }
};

template <bool W>
__device__ __forceinline__ bool walk_block(const BlockArgs& a, uint64_t i, uint64_t beg, uint64_t end, BlockRec& r,
                                           uint64_t first) {
  r = BlockRec{};
  if (end < beg) return false;
  canon::OffsetCursor<true> c = canon::OffsetCursor<true>::over(a.d, beg, end);
  return canon::walk_block(c, BlockVisit<W>{a, r, i, first});
}

extern "C" __global__ void __launch_bounds__(kTile) pz_unwire_block_size_kernel(BlockArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  uint64_t cnt[1] = {0};
  if (i < a.n) {
    BlockRec r;
    const bool ok = walk_block<false>(a, i, a.offs[i], a.offs[i + 1], r, 0);
    if (!ok) r = BlockRec{};  // a block that fails has no fields and no attestations
    a.o.slot_number[i] = r.slot;
    a.o.ts_seconds[i] = r.ts_seconds;
    a.o.ts_nanos[i] = r.ts_nanos;
    a.o.has_timestamp[i] = r.has_ts;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      a.o.bytes_beg[i * 5 + s] = r.beg[s];
      a.o.bytes_len[i * 5 + s] = r.len[s];
    }
    a.o.status[i] = ok ? PZ_OK : PZ_EINVAL;
    a.counts[i] = cnt[0] = r.natt;
  }
  tile_sums<1>(cnt, a.tiles, a.ntiles);
}

extern "C" __global__ void __launch_bounds__(kTile) pz_unwire_block_write_kernel(BlockArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  uint64_t cnt[1] = {i < a.n ? a.counts[i] : 0}, at[1];
  tile_excl<1>(cnt, at);
  if (i >= a.n) return;
  const uint64_t first = at[0] + a.tiles[blockIdx.x];
  a.o.att_first[i] = first;
  if (i + 1 == a.n) a.o.att_first[a.n] = first + cnt[0];
  if (!cnt[0]) return;
  BlockRec r;
  walk_block<true>(a, i, a.offs[i], a.offs[i + 1], r, first);
}

int block_out_args(const pz_block_cols_out* o, uint64_t n, uint64_t att_cap) {
  if (!o) return fail(PZ_EINVAL, "columns are null");
  if (n >> 32) return fail(PZ_EINVAL, "more than 2^32 blocks");
  if (!o->att_first) return fail(PZ_EINVAL, "att_first is null");
  if (n && (!o->slot_number || !o->ts_seconds || !o->ts_nanos || !o->has_timestamp || !o->bytes_beg || !o->bytes_len ||
            !o->status))
    return fail(PZ_EINVAL, "null output column");
  if (att_cap && (!o->att_beg || !o->att_end || !o->att_block_slot || !o->att_block))
    return fail(PZ_EINVAL, "null attestation column");
  return PZ_OK;
}

hipError_t launch_unwire_blocks(BlockArgs a, uint64_t* natt, void* scratch, hipStream_t s) {
  hipError_t e;
  if (!a.n) {
    if ((e = hipMemsetAsync(a.o.att_first, 0, 8, s)) != hipSuccess) return e;
    return hipMemsetAsync(natt, 0, 8, s);
  }
  a.ntiles = tiles_of(a.n);
  a.counts = static_cast<uint64_t*>(scratch);
  a.tiles = a.counts + a.n;
  hipLaunchKernelGGL(pz_unwire_block_size_kernel, dim3((uint32_t)a.ntiles), dim3(kTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_tile_scan(a.tiles, a.ntiles, 1u, natt, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(pz_unwire_block_write_kernel, dim3((uint32_t)a.ntiles), dim3(kTile), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_tile_scan(uint64_t* tiles, uint64_t ntiles, uint32_t ncols, uint64_t* totals, hipStream_t s) {
  hipLaunchKernelGGL(pz_unwire_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, tiles, ntiles, ncols, totals);
  return hipGetLastError();
}

}  // namespace pz

using namespace pz;

extern "C" {

uint64_t pz_unwire_attestations_scratch_bytes(uint64_t n) {
  return pad256(((kAttCols - 1) * n + kAttCols * tiles_of(n)) * 8 + 8);
}

int pz_dev_unwire_attestations(const uint8_t* d_bytes, const uint64_t* d_begs, const uint64_t* d_ends, uint64_t n,
                               uint32_t field_num, const pz_attestation_cols_out* out, uint64_t* d_totals,
                               void* d_scratch, void* stream) {
  int rc = att_out_args(out, n, field_num);
  if (rc) return rc;
  if (!d_totals || !d_scratch || (n && (!d_bytes || !d_begs || !d_ends))) return fail(PZ_EINVAL, "null device pointer");
  AttArgs a{};
  a.d = d_bytes;
  a.begs = d_begs;
  a.ends = d_ends;
  a.n = n;
  a.field = field_num;
  a.o = *out;
  const hipError_t e = launch_unwire_att(a, d_totals, d_scratch, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_unwire_att kernels");
}

int pz_unwire_attestations(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint32_t field_num,
                           const pz_attestation_cols_out* out, const uint64_t caps[6], uint64_t totals[7]) {
  int rc = att_out_args(out, n, field_num);
  if (rc) return rc;
  if (!caps || !totals) return fail(PZ_EINVAL, "caps or totals is null");
  if ((rc = check_csr(offsets, n, "record"))) return rc;
  if (n && !bytes) return fail(PZ_EINVAL, "bytes is null");
  const uint64_t nbytes = n ? offsets[n] - offsets[0] : 0;
  HostForm f;  // (no handle: the current device's context)
  if (f.rc) return f.rc;
  Stager& st = f.st;
  const std::vector<uint64_t> rb = rebase(offsets, n);
  AttArgs a{};
  a.d = st.up(n ? bytes + offsets[0] : nullptr, nbytes);
  a.begs = st.up(rb.data(), n + 1);
  a.ends = a.begs + 1;
  a.n = n;
  a.field = field_num;
  // every column at its bound: bytes columns and sig values the input's byte count, elements half
  pz_attestation_cols_out d{};
  const uint64_t bound[kAttTotals] = {nbytes, nbytes, nbytes, nbytes / 2, nbytes, nbytes};
  for (int k = 0; k < kAttNCols; ++k)
    att_set_out(&d, k, st.put(nullptr, att_col_len(kAttTable[k], n, bound) * kAttTable[k].width));
  d.n_oblique = out->n_oblique ? st.up<uint64_t>(nullptr, n) : nullptr;
  d.last_byte = out->last_byte ? st.up<uint8_t>(nullptr, n) : nullptr;
  d.status = st.up<int32_t>(nullptr, n);
  uint64_t* d_totals = st.up<uint64_t>(nullptr, kAttCols);
  void* scratch = st.up<uint8_t>(nullptr, pz_unwire_attestations_scratch_bytes(n));
  if (st.rc) return st.rc;
  a.o = d;
  st.check(launch_unwire_att(a, d_totals, scratch, st.s), "pz_unwire_att kernels");
  st.down(totals, d_totals, kAttCols);
  if (st.sync()) return st.rc;
  for (int c = 0; c < kAttTotals; ++c)
    if (totals[c] > caps[c])
      return fail(PZ_ERANGE, "%s needs %llu, capacity %llu", att_total_name(c), (unsigned long long)totals[c],
                  (unsigned long long)caps[c]);
  for (int k = 0; k < kAttNCols; ++k)
    st.down(static_cast<uint8_t*>(att_out(*out, k)), static_cast<const uint8_t*>(att_out(d, k)),
            att_col_len(kAttTable[k], n, totals) * kAttTable[k].width);
  if (out->n_oblique) st.down(out->n_oblique, d.n_oblique, n);
  if (out->last_byte) st.down(out->last_byte, d.last_byte, n);
  st.down(out->status, d.status, n);
  return st.sync();
}

uint64_t pz_unwire_blocks_scratch_bytes(uint64_t n) { return pad256((n + tiles_of(n)) * 8 + 8); }

int pz_dev_unwire_blocks(const uint8_t* d_blocks, const uint64_t* d_offsets, uint64_t n, uint64_t att_cap,
                         const pz_block_cols_out* out, uint64_t* d_natt, void* d_scratch, void* stream) {
  int rc = block_out_args(out, n, att_cap);
  if (rc) return rc;
  if (!d_natt || !d_scratch || (n && (!d_blocks || !d_offsets))) return fail(PZ_EINVAL, "null device pointer");
  BlockArgs a{};
  a.d = d_blocks;
  a.offs = d_offsets;
  a.n = n;
  a.att_cap = att_cap;
  a.o = *out;
  const hipError_t e = launch_unwire_blocks(a, d_natt, d_scratch, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_unwire_block kernels");
}

int pz_unwire_blocks(const uint8_t* blocks, const uint64_t* offsets, uint64_t n, uint64_t att_cap,
                     const pz_block_cols_out* out, uint64_t* natt) {
  int rc = block_out_args(out, n, att_cap);
  if (rc) return rc;
  if (!natt) return fail(PZ_EINVAL, "natt is null");
  *natt = 0;
  if ((rc = check_csr(offsets, n, "block"))) return rc;
  if (n && !blocks) return fail(PZ_EINVAL, "blocks is null");
  const uint64_t nbytes = n ? offsets[n] - offsets[0] : 0, base = n ? offsets[0] : 0;
  HostForm f;  // (no handle: the current device's context)
  if (f.rc) return f.rc;
  Stager& st = f.st;
  const std::vector<uint64_t> rb = rebase(offsets, n);
  BlockArgs a{};
  a.d = st.up(n ? blocks + base : nullptr, nbytes);
  a.offs = st.up(rb.data(), n + 1);
  a.n = n;
  a.att_cap = att_cap;
  pz_block_cols_out d{};
  d.slot_number = st.up<uint64_t>(nullptr, n);
  d.ts_seconds = st.up<int64_t>(nullptr, n);
  d.ts_nanos = st.up<int64_t>(nullptr, n);
  d.has_timestamp = st.up<uint8_t>(nullptr, n);
  d.bytes_beg = st.up<uint64_t>(nullptr, n * 5);
  d.bytes_len = st.up<uint32_t>(nullptr, n * 5);
  d.att_first = st.up<uint64_t>(nullptr, n + 1);
  d.att_beg = st.up<uint64_t>(nullptr, att_cap);
  d.att_end = st.up<uint64_t>(nullptr, att_cap);
  d.att_block_slot = st.up<uint64_t>(nullptr, att_cap);
  d.att_block = st.up<uint32_t>(nullptr, att_cap);
  d.status = st.up<int32_t>(nullptr, n);
  uint64_t* d_natt = st.up<uint64_t>(nullptr, 1);
  void* scratch = st.up<uint8_t>(nullptr, pz_unwire_blocks_scratch_bytes(n));
  if (st.rc) return st.rc;
  a.o = d;
  st.check(launch_unwire_blocks(a, d_natt, scratch, st.s), "pz_unwire_block kernels");
  st.down(natt, d_natt, 1);
  if (st.sync()) return st.rc;
  if (*natt > att_cap)
    return fail(PZ_ERANGE, "%llu attestations, capacity %llu", (unsigned long long)*natt, (unsigned long long)att_cap);
  st.down(out->slot_number, d.slot_number, n);
  st.down(out->ts_seconds, d.ts_seconds, n);
  st.down(out->ts_nanos, d.ts_nanos, n);
  st.down(out->has_timestamp, d.has_timestamp, n);
  st.down(out->bytes_beg, d.bytes_beg, n * 5);
  st.down(out->bytes_len, d.bytes_len, n * 5);
  st.down(out->att_first, d.att_first, n + 1);
  st.down(out->att_beg, d.att_beg, *natt);
  st.down(out->att_end, d.att_end, *natt);
  st.down(out->att_block_slot, d.att_block_slot, *natt);
  st.down(out->att_block, d.att_block, *natt);
  st.down(out->status, d.status, n);
  if (st.sync()) return st.rc;
  // the spans are positions in the caller's buffer
  for (uint64_t k = 0; base && k < n * 5; ++k)
    if (out->bytes_len[k]) out->bytes_beg[k] += base;
  for (uint64_t k = 0; base && k < *natt; ++k) {
    out->att_beg[k] += base;
    out->att_end[k] += base;
  }
  return PZ_OK;
}

}  // extern "C"
