// The attestation store batch of a run of received blocks, for gfx950: the rows blockProcessing
// writes to the database (saveAttestation and saveAttestationHash, blockchain/service.go:288-297 over
// core.go:650-658 and :745-760), selected, hashed and encoded on the device from the columns the run
// already left there.  The rule is blockstore_dev.h's; this file is its kernels and entry points.
//
// pz_dev_block_store_select is four dependent launches on the caller's stream, the reduce-then-scan of
// tile_scan.h; no workgroup waits for another and the host reads nothing:
//   size   a lane per row forms the flag; a tile of 256 rows leaves its count;
//   scan   one workgroup turns the tiles' counts into their bases and the total m (pz_unwire_scan_kernel);
//   write  a lane per row forms the flag again, ranks it in its tile, and a saved row writes its index
//          to rows[rank] and its (att_beg, att_end) to span[rank]; every row leaves its rank in
//          scratch, lane 0 the count m behind them and in *count;
//   first  a lane per block reads the rank at att_first[j]: nblocks + 1 entries, so that empty blocks
//          and blocks past stop repeat the running value.
// pz_dev_block_store_digests is three independent launches over the m compacted rows: Attestation.Hash
// by the span hash (blake2b.hip) over the pairs, Attestation.Key by the key kernel (attdigest.hip)
// through the row list, and the list entries 0a 20 | hash as whole dwords, a lane per output dword.
#include <hip/hip_runtime.h>

#include "att_cols.h"
#include "attdigest.h"
#include "blake2b_kernels.h"
#include "blockstore_dev.h"
#include "resident.h"
#include "tile_scan.h"

namespace pz {
namespace {

constexpr int kBsThreads = 256;

struct BsArgs {
  pz_block_store_batch b;
  uint64_t ntiles;
  uint64_t* tiles;   // [ntiles]
  uint64_t* totals;  // [1]
  uint32_t* rank;    // [natt + 1]
};

__device__ __forceinline__ bool bs_flag(const pz_block_store_batch& b, uint64_t r) {
  const uint64_t stop = b.stop ? *b.stop : b.nblocks;
  return r < b.natt && bs_row_saved(r, b.nblocks, stop, b.att_block, b.block_status, b.parent_ok, b.att_status, b.rec_status);
}

extern "C" __global__ void __launch_bounds__(kTile) pz_block_store_size_kernel(BsArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  const uint64_t v[1] = {bs_flag(a.b, r) ? 1ull : 0ull};
  tile_sums<1>(v, a.tiles, a.ntiles);
}

extern "C" __global__ void __launch_bounds__(kTile) pz_block_store_write_kernel(BsArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  const uint64_t v[1] = {bs_flag(a.b, r) ? 1ull : 0ull};
  uint64_t ex[1];
  tile_excl<1>(v, ex);
  const uint64_t at = ex[0] + a.tiles[blockIdx.x];  // fewer than natt rows are saved before row r
  if (r < a.b.natt) {
    a.rank[r] = (uint32_t)at;
    if (v[0]) {
      a.b.rows[at] = (uint32_t)r;
      *reinterpret_cast<ulonglong2*>(a.b.span + 2 * at) = make_ulonglong2(a.b.att_beg[r], a.b.att_end[r]);
    }
  }
  if (r == 0) {
    a.rank[a.b.natt] = (uint32_t)a.totals[0];
    *a.b.count = a.totals[0];
  }
}

extern "C" __global__ void __launch_bounds__(kBsThreads) pz_block_store_first_kernel(BsArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * kBsThreads + threadIdx.x;
  if (j <= a.b.nblocks) a.b.first[j] = bs_first(a.rank, a.b.att_first[j], a.b.natt);
}

// lists is 4-byte aligned and holds 34 m bytes: the last dword of an odd m is a halfword store.
extern "C" __global__ void __launch_bounds__(kBsThreads) pz_block_store_lists_kernel(const uint8_t* hash, uint64_t m, uint8_t* lists) {
  const uint64_t d = (uint64_t)blockIdx.x * kBsThreads + threadIdx.x;
  if (d >= bs_list_dwords(m)) return;
  const uint32_t v = bs_list_dword(hash, d);
  if (bs_list_whole(d, m)) *reinterpret_cast<uint32_t*>(lists + 4 * d) = v;
  else *reinterpret_cast<uint16_t*>(lists + 4 * d) = (uint16_t)v;
}

uint64_t scratch_bytes(uint64_t natt) { return pad256((tiles_of(natt) + 1) * 8 + (natt + 1) * 4); }

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// Both forms, before any launch.  1: nothing to launch.
int check_select(const pz_block_store_batch* b, bool device_form, const void* d_scratch) {
  if (!b) return fail(PZ_EINVAL, "block store: null batch");
  if (b->nblocks >= (1ull << 31)) return fail(PZ_EINVAL, "nblocks %llu: 2^31 blocks or more", (unsigned long long)b->nblocks);
  if (b->natt >= (1ull << 32)) return fail(PZ_EINVAL, "natt %llu: 2^32 rows or more", (unsigned long long)b->natt);
  if (b->nblocks == 0 || b->natt == 0) return 1;
  if (!b->att_first || !b->block_status || !b->parent_ok)
    return fail(PZ_EINVAL, "block store: null att_first / block_status / parent_ok");
  if (!b->att_block || !b->att_status || !b->att_beg || !b->att_end)
    return fail(PZ_EINVAL, "block store: null att_block / att_status / att_beg / att_end");
  if (!b->rows || !b->span || !b->first || !b->count) return fail(PZ_EINVAL, "block store: null rows / span / first / count");
  if (!device_form) return PZ_OK;
  if (!d_scratch || !aligned16(d_scratch)) return fail(PZ_EINVAL, "block store: d_scratch must be a 16-B aligned device pointer");
  if (!aligned16(b->span)) return fail(PZ_EINVAL, "block store: span must be 16-B aligned");
  if (misaligned(b->att_first, 8) || misaligned(b->att_beg, 8) || misaligned(b->att_end, 8) || misaligned(b->stop, 8) ||
      misaligned(b->first, 8) || misaligned(b->count, 8))
    return fail(PZ_EINVAL, "block store: att_first, att_beg, att_end, stop, first and count must be 8-B aligned");
  if (misaligned(b->block_status, 4) || misaligned(b->att_block, 4) || misaligned(b->att_status, 4) ||
      misaligned(b->rec_status, 4) || misaligned(b->rows, 4))
    return fail(PZ_EINVAL, "block store: block_status, att_block, att_status, rec_status and rows must be 4-B aligned");
  return PZ_OK;
}

// ev (the A/B library's timed entry; null in the product): one event pair around the four launches.
hipError_t launch_select(const pz_block_store_batch& b, void* d_scratch, hipStream_t s, Events* ev) {
  BsArgs a;
  a.b = b;
  a.ntiles = tiles_of(b.natt);
  a.tiles = static_cast<uint64_t*>(d_scratch);
  a.totals = a.tiles + a.ntiles;
  a.rank = reinterpret_cast<uint32_t*>(a.totals + 1);
  hipError_t e;
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_block_store_size_kernel, dim3((uint32_t)a.ntiles), dim3(kTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = launch_tile_scan(a.tiles, a.ntiles, 1u, a.totals, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(pz_block_store_write_kernel, dim3((uint32_t)a.ntiles), dim3(kTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(pz_block_store_first_kernel, dim3((uint32_t)((b.nblocks + kBsThreads) / kBsThreads)), dim3(kBsThreads), 0, s, a);
  e = hipGetLastError();
  stamp(ev, 1, s);
  return e;
}

// Both forms, before any launch.  1: nothing to launch.
int check_digests(const pz_block_store_batch* b, const pz_attestation_cols* a, uint64_t m, bool device_form) {
  if (!b) return fail(PZ_EINVAL, "block store: null batch");
  if (m > b->natt) return fail(PZ_EINVAL, "block store: m %llu exceeds natt %llu", (unsigned long long)m, (unsigned long long)b->natt);
  if (b->natt >= (1ull << 32)) return fail(PZ_EINVAL, "natt %llu: 2^32 rows or more", (unsigned long long)b->natt);
  if (m == 0) return 1;
  if (!b->bytes || !b->rows || !b->span) return fail(PZ_EINVAL, "block store: null bytes / rows / span");
  if (!b->key || !b->hash || !b->lists) return fail(PZ_EINVAL, "block store: null key / hash / lists");
  int rc = check_att_key_cols(a, b->natt, !device_form);
  if (rc || !device_form) return rc;
  if (!aligned16(b->span) || !aligned16(b->key) || !aligned16(b->hash))
    return fail(PZ_EINVAL, "block store: span, key and hash must be 16-B aligned");
  if (misaligned(b->rows, 4) || misaligned(b->lists, 4)) return fail(PZ_EINVAL, "block store: rows and lists must be 4-B aligned");
  return PZ_OK;
}

// ev: four events, one before the first launch and one after each.
hipError_t launch_digests(const pz_block_store_batch& b, const pz_attestation_cols& a, uint64_t m, hipStream_t s, Events* ev) {
  hipError_t e;
  stamp(ev, 0, s);
  if ((e = launch_b2b_span_pairs(b.bytes, b.span, m, b.hash, 32, s)) != hipSuccess) return e;
  stamp(ev, 1, s);
  if ((e = launch_att_keys_rows(a, b.natt, b.rows, m, b.key, s)) != hipSuccess) return e;
  stamp(ev, 2, s);
  hipLaunchKernelGGL(pz_block_store_lists_kernel, dim3((uint32_t)((bs_list_dwords(m) + kBsThreads - 1) / kBsThreads)), dim3(kBsThreads),
                     0, s, b.hash, m, b.lists);
  e = hipGetLastError();
  stamp(ev, 3, s);
  return e;
}

}  // namespace
}  // namespace pz

using namespace pz;

extern "C" {

uint64_t pz_block_store_scratch_bytes(uint64_t nblocks, uint64_t natt) {
  (void)nblocks;  // (first is the caller's column)
  return scratch_bytes(natt);
}

int pz_dev_block_store_select(const pz_block_store_batch* b, void* d_scratch, void* stream) {
  int rc = check_select(b, true, d_scratch);
  if (rc) return rc < 0 ? rc : PZ_OK;
  hipError_t e = launch_select(*b, d_scratch, static_cast<hipStream_t>(stream), nullptr);
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_block_store select kernels");
}

int pz_block_store_select(const pz_block_store_batch* hb) {
  int rc = check_select(hb, false, nullptr);
  if (rc < 0) return rc;
  if (rc) {  // no block or no row: nothing is saved, every rank is 0
    if (hb->count) *hb->count = 0;
    for (uint64_t j = 0; hb->first && j <= hb->nblocks; ++j) hb->first[j] = 0;
    return PZ_OK;
  }
  const uint64_t nb = hb->nblocks, n = hb->natt;
  HostForm f;  // (no handle: the current device's context)
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_block_store_batch d = *hb;
  d.att_first = st.up(hb->att_first, nb + 1);
  d.block_status = st.up(hb->block_status, nb);
  d.parent_ok = st.up(hb->parent_ok, nb);
  if (hb->stop) d.stop = st.up(hb->stop, 1);
  d.att_block = st.up(hb->att_block, n);
  d.att_status = st.up(hb->att_status, n);
  if (hb->rec_status) d.rec_status = st.up(hb->rec_status, n);
  d.att_beg = st.up(hb->att_beg, n);
  d.att_end = st.up(hb->att_end, n);
  d.rows = st.up<uint32_t>(nullptr, n);
  d.span = st.up<uint64_t>(nullptr, 2 * n);
  d.first = st.up<uint64_t>(nullptr, nb + 1);
  d.count = st.up<uint64_t>(nullptr, 1);
  void* scr = st.up<uint8_t>(nullptr, scratch_bytes(n));
  if (st.rc) return st.rc;
  st.check(launch_select(d, scr, st.s, nullptr), "pz_block_store select kernels");
  st.down(hb->count, d.count, 1);
  st.down(hb->first, d.first, nb + 1);
  if ((rc = st.sync())) return rc;
  const uint64_t m = *hb->count;  // entries past m stay as the caller left them
  st.down(hb->rows, d.rows, m);
  st.down(hb->span, d.span, 2 * m);
  return st.sync();
}

int pz_dev_block_store_digests(const pz_block_store_batch* b, const pz_attestation_cols* a, uint64_t m, void* stream) {
  int rc = check_digests(b, a, m, true);
  if (rc) return rc < 0 ? rc : PZ_OK;
  hipError_t e = launch_digests(*b, *a, m, static_cast<hipStream_t>(stream), nullptr);
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_block_store digest kernels");
}

int pz_block_store_digests(const pz_block_store_batch* hb, const pz_attestation_cols* a, uint64_t m) {
  int rc = check_digests(hb, a, m, false);
  if (rc) return rc < 0 ? rc : PZ_OK;
  const uint64_t n = hb->natt;
  for (uint64_t i = 0; i < m; ++i) {  // what the device form takes on trust
    if (hb->rows[i] >= n) return fail(PZ_EINVAL, "block store: rows[%llu] names no row", (unsigned long long)i);
    if (hb->span[2 * i] > hb->span[2 * i + 1] || hb->span[2 * i + 1] > hb->nbytes)
      return fail(PZ_EINVAL, "block store: span %llu leaves the bytes", (unsigned long long)i);
  }
  HostForm f;  // (no handle: the current device's context)
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_attestation_cols dc;
  stage_att_cols(st, *a, n, kAttKeyCols, &dc);
  pz_block_store_batch d = *hb;
  d.bytes = st.up(hb->bytes, hb->nbytes);  // (a slot's allocation has the 4 readable bytes behind it)
  d.rows = st.up(hb->rows, m);
  d.span = st.up(hb->span, 2 * m);
  d.key = st.up<uint8_t>(nullptr, 32 * m);
  d.hash = st.up<uint8_t>(nullptr, 32 * m);
  d.lists = st.up<uint8_t>(nullptr, 4 * bs_list_dwords(m));
  if (st.rc) return st.rc;
  st.check(launch_digests(d, dc, m, st.s, nullptr), "pz_block_store digest kernels");
  st.down(hb->key, d.key, 32 * m);
  st.down(hb->hash, d.hash, 32 * m);
  st.down(hb->lists, d.lists, bs_list_bytes(m));
  return st.sync();
}

#ifdef PZ_AB_BUILD
// (tools/blockstore_probe.py) The device forms with event pairs: ms[0] the four launches of select;
// ms[0..3) the three launches of digests.  Both synchronise the stream.
int pz_debug_block_store_select_timed(const pz_block_store_batch* b, void* d_scratch, void* stream, float ms[1]) {
  int rc = check_select(b, true, d_scratch);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!ms) return fail(PZ_EINVAL, "block store: null ms");
  Events ev;
  if ((rc = ev.create(2))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t e = launch_select(*b, d_scratch, s, &ev);
  return ev.elapsed(e == hipSuccess ? PZ_OK : hip_fail(e, "pz_block_store select kernels"), ms, nullptr, 1, s, "block store select");
}

int pz_debug_block_store_digests_timed(const pz_block_store_batch* b, const pz_attestation_cols* a, uint64_t m, void* stream,
                                       float ms[3]) {
  int rc = check_digests(b, a, m, true);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!ms) return fail(PZ_EINVAL, "block store: null ms");
  Events ev;
  if ((rc = ev.create(4))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t e = launch_digests(*b, *a, m, s, &ev);
  return ev.elapsed(e == hipSuccess ? PZ_OK : hip_fail(e, "pz_block_store digest kernels"), ms, nullptr, 3, s, "block store digests");
}
#endif

}  // extern "C"
