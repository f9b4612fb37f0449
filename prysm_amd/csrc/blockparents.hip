// The saved-block set resident on the device and the parent check over a run of received blocks,
// for gfx950: hasBlock(block.ParentHash()) (blockchain/service.go:261-269, core.go:560-562) answered
// from the blocks saveBlock stored (service.go:324, core.go:565-577), the blocks of the run saving
// each other as the reference's loop would.  The rules are blockparents_dev.h's; this file is their
// kernels and entry points.
//
// pz_dev_block_parents is a memset of the run table and three dependent launches on the caller's
// stream; no workgroup waits for another and the host reads nothing:
//   open     a lane per block: open0 through the gate's inlines, and the open blocks' indices into the
//            run table (scratch), keyed by block_hash: atomicCAS on the first empty cell of the probe,
//            a lost CAS moves on -- equal hashes take cells of their own.  Only atomics touch a cell.
//   link     a lane per block: BytesToHash of field 1, the probe of the resident set (plain loads: no
//            launch writes it meanwhile) and of the run table (written by the launch before) for the
//            largest open copy before the block; the words P_j and S_j.
//   resolve  ONE workgroup of 1,024 lanes, tiles of 1,024 blocks: ceil(log2 nblocks) pointer-jumping
//            rounds over S, double-buffered in scratch with a barrier a round, then parent_ok, saved0
//            and block_status_out.  Words another wave of the workgroup wrote are read and written
//            with relaxed agent-scope atomics, as votecache.hip's commit does.
// pz_dev_block_set_insert[_walked] is one launch of one workgroup, the vote cache's claim idiom a tile
// at a time: claim with the input index, compare against the claimant's input hash, barrier, the
// standing claim's lane writes the key and turns the cell full, barrier.  During a tile a cell only
// goes empty -> claimed -> claimed lower; keys and full cells appear only between the barriers.
// pz_dev_block_set_reserve rehashes the distinct keys into the other buffer set: a lane per old cell,
// CAS empty -> full, then the key (nobody reads a key in that launch).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "blockparents_dev.h"
#include "resident.h"

struct pz_block_set : pz::Resident {
  pz::DevBuf state[2], keys[2], words, stage;  // words: count, error; stage: pz_block_set_new's upload
  uint32_t cells = 0;
  int live = 0;
  ~pz_block_set() {
    drain();
    for (pz::DevBuf* b : {&state[0], &state[1], &keys[0], &keys[1], &words, &stage}) b->release();
  }
};

namespace pz {
namespace {

constexpr int kThreads = 256, kWgThreads = 1024;
constexpr uint32_t kNoCell = 0xFFFFFFFFu;

#define PZ_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct BsTable {
  uint32_t* state;
  uint8_t* keys;
  uint64_t* words;
  uint32_t cells;
};

struct BpScratch {
  uint32_t* run;  // bp_run_cells(nblocks)
  uint32_t run_cells;
  uint32_t* p;    // nblocks: P_j
  uint32_t* sa;   // nblocks: S_j, the rounds' two buffers
  uint32_t* sb;
  uint8_t* open0;  // nblocks
};

__device__ __forceinline__ uint32_t ld(const uint32_t* p) { return __hip_atomic_load(p, PZ_RLX_AGENT); }
__device__ __forceinline__ void st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, PZ_RLX_AGENT); }

// A key that a lane of this launch may have written a tile ago.
__device__ __forceinline__ Hash32 ld_key(const uint8_t* keys, uint32_t c) {
  const uint32_t* k = reinterpret_cast<const uint32_t*>(keys + 32ull * c);
  Hash32 h;
#pragma unroll
  for (int w = 0; w < 8; ++w) h.w[w] = ld(k + w);
  return h;
}

// ---- the set ---------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kThreads) pz_bs_contains_kernel(BsTable t, const uint8_t* hashes, uint64_t n, uint8_t* out) {
  const uint64_t q = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  out[q] = bs_contains(t.state, t.keys, t.cells, vc_load_hash16(hashes + 32 * q)) ? 1 : 0;
}

// walk != NULL: the walked form (take unused); else take (NULL: all).
extern "C" __global__ void __launch_bounds__(kWgThreads) pz_bs_insert_kernel(BsTable t, const uint8_t* hashes, const uint8_t* take,
                                                                             const uint8_t* walk, const uint32_t* flags, uint64_t n,
                                                                             uint64_t* count_out) {
  __shared__ uint32_t s_new, s_over;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  if (tid == 0) s_new = 0, s_over = 0;
  __syncthreads();
  const uint32_t gate_flags = walk && flags ? *flags : 0;  // (the same word in every lane)
  for (uint64_t t0 = 0; t0 < n; t0 += kWgThreads) {        // (block-uniform)
    const uint64_t j = t0 + tid;
    const bool want = j < n && (walk ? bp_insert_walked(walk[j], gate_flags) : (!take || take[j] != 0));
    const uint32_t mine = vc_claim((uint32_t)j);
    uint32_t cell = kNoCell;
    Hash32 h;
    if (want) {
      h = vc_load_hash16(hashes + 32 * j);
      bool done = false;
      uint32_t c = vc_home(h, t.cells);
      for (uint32_t step = 0; step < t.cells && !done; ++step, c = vc_next(c, t.cells)) {
        uint32_t v = ld(&t.state[c]);
        if (v == kBsEmpty) {
          v = atomicCAS(&t.state[c], kBsEmpty, mine);  // a lost CAS returns the winner's claim
          if (v == kBsEmpty) {
            cell = c;
            break;
          }
        }
        if (v == kBsFull) {
          done = vc_hash_eq(h, ld_key(t.keys, c));  // already a key
        } else if (bs_is_claim(v)) {
          const uint32_t src = vc_claim_source(v);
          if (src == (uint32_t)j || (src < n && vc_hash_eq(h, vc_load_hash16(hashes + 32ull * src)))) {
            if (mine < v) atomicMin(&t.state[c], mine);
            cell = c;
            done = true;
          }
        }
      }
      if (!done && cell == kNoCell) atomicOr(&s_over, 1u);  // every cell holds another hash
    }
    __syncthreads();  // the tile's claims stand
    const bool lead = cell != kNoCell && ld(&t.state[cell]) == mine;
    if (lead) {
      uint32_t* k = reinterpret_cast<uint32_t*>(t.keys + 32ull * cell);
#pragma unroll
      for (int w = 0; w < 8; ++w) st(k + w, h.w[w]);
    }
    const uint64_t leaders = __ballot(lead);
    if (lane == 0 && leaders) atomicAdd(&s_new, (uint32_t)__builtin_popcountll(leaders));
    __syncthreads();  // every claim of the tile has been read and every key written: the cells turn full
    if (lead) st(&t.state[cell], kBsFull);
    __syncthreads();
  }
  if (tid == 0) {
    const uint64_t c = t.words[kBsCount] + s_new;
    t.words[kBsCount] = c;
    if (s_over) t.words[kBsErr] |= kBsErrCapacity;
    if (count_out) *count_out = c;
  }
}

extern "C" __global__ void __launch_bounds__(kThreads) pz_bs_rehash_kernel(BsTable from, BsTable to) {
  const uint64_t c0 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c0 >= from.cells || from.state[c0] != kBsFull) return;
  const Hash32 h = vc_load_hash16(from.keys + 32 * c0);
  uint32_t c = vc_home(h, to.cells);
  for (uint32_t step = 0; step < to.cells; ++step, c = vc_next(c, to.cells)) {
    if (atomicCAS(&to.state[c], kBsEmpty, kBsFull) != kBsEmpty) continue;  // (the keys are distinct: no compare)
    uint32_t* k = reinterpret_cast<uint32_t*>(to.keys + 32ull * c);
#pragma unroll
    for (int w = 0; w < 8; ++w) k[w] = h.w[w];
    return;
  }
  atomicOr((unsigned long long*)&to.words[kBsErr], (unsigned long long)kBsErrCapacity);  // (to.cells > from.cells: unreachable)
}

// ---- the parent check --------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(kThreads) pz_bp_open_kernel(pz_block_parents_batch b, BpScratch s) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= b.nblocks) return;
  const bool open0 = bp_open0(b.att_first, b.block_status, b.rec_status, b.att_status, b.natt, j);
  s.open0[j] = open0 ? 1 : 0;
  if (!open0) return;
  uint32_t c = vc_home(vc_load_hash16(b.block_hash + 32 * j), s.run_cells);
  for (uint32_t step = 0; step < s.run_cells; ++step, c = vc_next(c, s.run_cells))
    if (atomicCAS(&s.run[c], kBpNoLink, (uint32_t)j) == kBpNoLink) return;
}

extern "C" __global__ void __launch_bounds__(kThreads) pz_bp_link_kernel(pz_block_parents_batch b, BpScratch s, BsTable t) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= b.nblocks) return;
  const uint64_t beg = b.bytes_beg[5 * j];
  const uint32_t len = b.bytes_len[5 * j];
  uint32_t pw = kBpFalse, sw = kBpFalse;
  if (bp_span_ok(beg, len, b.nbytes)) {
    const bool free = bp_free(b.slot_number[j]);
    bool in_set = false;
    uint32_t link = kBpNoLink;
    if (!free) {
      const Hash32 parent = bp_parent(b.bytes, beg, len);
      in_set = bs_contains(t.state, t.keys, t.cells, parent);
      if (!in_set) link = bp_link(s.run, s.run_cells, b.block_hash, parent, j);
    }
    pw = bp_parent_word(free, in_set, link);
    sw = bp_saved_word(s.open0[j] != 0, pw);
  }
  s.p[j] = pw;
  s.sa[j] = sw;
}

extern "C" __global__ void __launch_bounds__(kWgThreads) pz_bp_resolve_kernel(pz_block_parents_batch b, BpScratch s) {
  const uint64_t n = b.nblocks;
  uint32_t* a = s.sa;
  uint32_t* o = s.sb;
  const uint32_t rounds = bp_rounds(n);
  for (uint32_t r = 0; r < rounds; ++r) {  // (block-uniform)
    for (uint64_t j = threadIdx.x; j < n; j += kWgThreads) {
      const uint32_t v = ld(a + j);
      st(o + j, bp_jump(v, !bp_resolved(v) && v < n ? ld(a + v) : kBpFalse));
    }
    __syncthreads();
    uint32_t* x = a;
    a = o, o = x;
  }
  for (uint64_t j = threadIdx.x; j < n; j += kWgThreads) {
    const uint32_t pw = s.p[j];
    const bool ok = bp_parent_ok(pw, !bp_resolved(pw) && pw < n ? ld(a + pw) : kBpFalse);
    b.parent_ok[j] = ok ? 1 : 0;
    b.saved0[j] = ok && s.open0[j] ? 1 : 0;
    b.block_status_out[j] = bp_status_out(b.block_status[j], ok);
  }
}

// ---- host side -----------------------------------------------------------------------------------------
BsTable table_of(pz_block_set* h) {
  return BsTable{static_cast<uint32_t*>(h->state[h->live].ptr), static_cast<uint8_t*>(h->keys[h->live].ptr),
                 static_cast<uint64_t*>(h->words.ptr), h->cells};
}

uint64_t scratch_bytes(uint64_t n) { return r16(4ull * bp_run_cells(n)) + 3 * r16(4 * n) + r16(n); }

BpScratch scratch_of(void* d_scratch, uint64_t n) {
  uint8_t* p = static_cast<uint8_t*>(d_scratch);
  BpScratch s;
  s.run_cells = bp_run_cells(n);
  s.run = reinterpret_cast<uint32_t*>(p), p += r16(4ull * s.run_cells);
  s.p = reinterpret_cast<uint32_t*>(p), p += r16(4 * n);
  s.sa = reinterpret_cast<uint32_t*>(p), p += r16(4 * n);
  s.sb = reinterpret_cast<uint32_t*>(p), p += r16(4 * n);
  s.open0 = p;
  return s;
}

uint32_t grid(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

int check_set(const pz_block_set* h) { return h ? PZ_OK : fail(PZ_EINVAL, "the block set is null"); }

// 1: nothing to launch.
int check_hashes(const pz_block_set* h, const uint8_t* hashes, uint64_t n, const char* what) {
  if (!h) return fail(PZ_EINVAL, "%s: the block set is null", what);
  if (n >= (1ull << 31)) return fail(PZ_EINVAL, "%s: n %llu: 2^31 hashes or more", what, (unsigned long long)n);
  if (n && !hashes) return fail(PZ_EINVAL, "%s: null hashes", what);
  return n ? PZ_OK : 1;
}

int check_parents(const pz_block_set* h, const pz_block_parents_batch* b) {
  if (!h || !b) return fail(PZ_EINVAL, "block parents: null set or batch");
  if (b->nblocks >= (1ull << 31)) return fail(PZ_EINVAL, "nblocks %llu: 2^31 blocks or more", (unsigned long long)b->nblocks);
  if (b->nblocks == 0) return 1;
  if (!b->bytes_beg || !b->bytes_len || !b->slot_number || !b->block_hash || !b->att_first || !b->block_status)
    return fail(PZ_EINVAL, "block parents: null bytes_beg / bytes_len / slot_number / block_hash / att_first / block_status");
  if (!b->parent_ok || !b->saved0 || !b->block_status_out)
    return fail(PZ_EINVAL, "block parents: null parent_ok / saved0 / block_status_out");
  if (b->nbytes && !b->bytes) return fail(PZ_EINVAL, "block parents: nbytes %llu with null bytes", (unsigned long long)b->nbytes);
  if (b->natt && !b->att_status) return fail(PZ_EINVAL, "block parents: natt %llu with null att_status", (unsigned long long)b->natt);
  return PZ_OK;
}

hipError_t launch_contains(pz_block_set* h, const uint8_t* d_hashes, uint64_t n, uint8_t* d_out, hipStream_t s) {
  hipLaunchKernelGGL(pz_bs_contains_kernel, dim3(grid(n)), dim3(kThreads), 0, s, table_of(h), d_hashes, n, d_out);
  h->last = s;
  return hipGetLastError();
}

hipError_t launch_insert(pz_block_set* h, const uint8_t* d_hashes, const uint8_t* d_take, const uint8_t* d_walk,
                         const uint32_t* d_flags, uint64_t n, uint64_t* d_count_out, hipStream_t s, Events* ev = nullptr) {
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_bs_insert_kernel, dim3(1), dim3(kWgThreads), 0, s, table_of(h), d_hashes, d_take, d_walk, d_flags, n, d_count_out);
  stamp(ev, 1, s);
  h->last = s;
  return hipGetLastError();
}

// Room for min_keys keys, on s.
int reserve(pz_block_set* h, uint64_t min_keys, hipStream_t s) {
  if (min_keys > kBsMaxKeys) return fail(PZ_EINVAL, "a block set of %llu keys: above 2^30", (unsigned long long)min_keys);
  if (2 * min_keys <= h->cells) return PZ_OK;
  const uint32_t cells = bs_cells(min_keys);
  const int other = h->live ^ 1;
  int rc;
  if ((rc = h->state[other].reserve((size_t)cells * 4)) || (rc = h->keys[other].reserve((size_t)cells * 32))) return rc;
  hipError_t e = hipMemsetAsync(h->state[other].ptr, 0xFF, (size_t)cells * 4, s);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
  const BsTable from = table_of(h);
  const BsTable to{static_cast<uint32_t*>(h->state[other].ptr), static_cast<uint8_t*>(h->keys[other].ptr), from.words, cells};
  hipLaunchKernelGGL(pz_bs_rehash_kernel, dim3(grid(from.cells)), dim3(kThreads), 0, s, from, to);
  h->last = s;
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_bs_rehash_kernel");
  h->live = other, h->cells = cells;
  return PZ_OK;
}

int launch_parents(pz_block_set* h, const pz_block_parents_batch& b, void* d_scratch, hipStream_t s, Events* ev = nullptr) {
  const BpScratch scr = scratch_of(d_scratch, b.nblocks);
  hipError_t e = hipMemsetAsync(scr.run, 0xFF, r16(4ull * scr.run_cells), s);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
  h->last = s;
  const uint32_t g = grid(b.nblocks);
  stamp(ev, 0, s);
  hipLaunchKernelGGL(pz_bp_open_kernel, dim3(g), dim3(kThreads), 0, s, b, scr);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_bp_open_kernel");
  stamp(ev, 1, s);
  hipLaunchKernelGGL(pz_bp_link_kernel, dim3(g), dim3(kThreads), 0, s, b, scr, table_of(h));
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_bp_link_kernel");
  stamp(ev, 2, s);
  hipLaunchKernelGGL(pz_bp_resolve_kernel, dim3(1), dim3(kWgThreads), 0, s, b, scr);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "pz_bp_resolve_kernel");
  stamp(ev, 3, s);
  return PZ_OK;
}

// Waits for the set's last call and reads its words; the sticky code to report.
int settle(pz_block_set* h, uint64_t* count, int* sticky) {
  uint64_t w[kBsWords] = {0, 0};
  int rc = h->settle(w, h->words, sizeof w, "block set read");
  if (rc) return rc;
  *count = w[kBsCount];
  *sticky = (w[kBsErr] & kBsErrCapacity) ? PZ_ERANGE : PZ_OK;
  return PZ_OK;
}

int report(int sticky) {
  return sticky == PZ_ERANGE ? fail(PZ_ERANGE, "an insert found no cell for a key: reserve before inserting") : PZ_OK;
}

}  // namespace
}  // namespace pz

using namespace pz;

extern "C" {

int pz_block_set_new(const uint8_t* hashes, uint64_t n, uint64_t min_keys, int device, pz_block_set** out) {
  if (!out) return fail(PZ_EINVAL, "out is null");
  *out = nullptr;
  if (n > kBsMaxKeys || min_keys > kBsMaxKeys)
    return fail(PZ_EINVAL, "a block set of %llu hashes and %llu keys: above 2^30", (unsigned long long)n, (unsigned long long)min_keys);
  if (n && !hashes) return fail(PZ_EINVAL, "hashes is null");
  int rc = Resident::open(device);
  if (rc) return rc;
  auto* h = new pz_block_set();
  h->device = device;
  h->cells = bs_cells(n > min_keys ? n : min_keys);
  const char* what = "block set init";
  hipError_t e = hipSuccess;
  if ((rc = h->state[0].fill((size_t)h->cells * 4, 0xFF, what)) || (rc = h->keys[0].fill((size_t)h->cells * 32, 0, what)) ||
      (rc = h->words.fill(sizeof(uint64_t) * kBsWords, 0, what)) || (n && (rc = h->stage.fill(n * 32, 0, what, hashes, n * 32)))) {
    delete h;
    return rc;
  }
  if (n) e = launch_insert(h, static_cast<const uint8_t*>(h->stage.ptr), nullptr, nullptr, nullptr, n, nullptr, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  h->stage.release();
  if (e != hipSuccess) {
    delete h;
    return hip_fail(e, what);
  }
  *out = h;
  return PZ_OK;
}

void pz_block_set_free(pz_block_set* h) { delete h; }

int pz_block_set_count(pz_block_set* h, uint64_t* count) {
  if (!h || !count) return fail(PZ_EINVAL, "block set / count is null");
  int rc = h->use();
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  int sticky;
  if ((rc = settle(h, count, &sticky))) return rc;
  return report(sticky);
}

int pz_block_set_read(pz_block_set* h, uint8_t* hashes, uint64_t cap, uint64_t* count) {
  if (!h || !count) return fail(PZ_EINVAL, "block set / count is null");
  int rc = h->use();
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  int sticky;
  if ((rc = settle(h, count, &sticky))) return rc;
  if (hashes && *count && cap >= *count) {  // (a read-side walk of the table on the host)
    std::vector<uint32_t> state(h->cells);
    std::vector<uint8_t> keys((size_t)h->cells * 32);
    if ((rc = down(state.data(), h->state[h->live].ptr, h->cells, "block set read")) ||
        (rc = down(keys.data(), h->keys[h->live].ptr, (uint64_t)h->cells * 32, "block set read")))
      return rc;
    uint64_t k = 0;
    for (uint32_t c = 0; c < h->cells && k < cap; ++c)
      if (state[c] == kBsFull) std::memcpy(hashes + 32 * k++, keys.data() + 32ull * c, 32);
    *count = k;
  }
  return report(sticky);
}

int pz_dev_block_set_contains(pz_block_set* h, const uint8_t* d_hashes, uint64_t n, uint8_t* d_out, void* stream) {
  int rc = check_hashes(h, d_hashes, n, "block set contains");
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!d_out || !aligned16(d_hashes)) return fail(PZ_EINVAL, "block set contains: null out, or hashes not 16-B aligned");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  hipError_t e = launch_contains(h, d_hashes, n, d_out, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_bs_contains_kernel");
}

int pz_block_set_contains(pz_block_set* h, const uint8_t* hashes, uint64_t n, uint8_t* out) {
  int rc = check_hashes(h, hashes, n, "block set contains");
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!out) return fail(PZ_EINVAL, "block set contains: null out");
  HostForm f(h, "block set contains");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  const uint8_t* d_hashes = st.up(hashes, n * 32);
  uint8_t* d_out = st.up<uint8_t>(nullptr, n);
  if (st.rc) return st.rc;
  st.check(launch_contains(h, d_hashes, n, d_out, st.s), "pz_bs_contains_kernel");
  st.down(out, static_cast<const uint8_t*>(d_out), n);
  return st.sync();
}

int pz_dev_block_set_insert(pz_block_set* h, const uint8_t* d_hashes, const uint8_t* d_take, uint64_t n, void* stream) {
  int rc = check_hashes(h, d_hashes, n, "block set insert");
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!aligned16(d_hashes)) return fail(PZ_EINVAL, "block set insert: hashes must be a 16-B aligned device pointer");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  hipError_t e = launch_insert(h, d_hashes, d_take, nullptr, nullptr, n, nullptr, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_bs_insert_kernel");
}

int pz_block_set_insert(pz_block_set* h, const uint8_t* hashes, const uint8_t* take, uint64_t n) {
  int rc = check_hashes(h, hashes, n, "block set insert");
  if (rc) return rc < 0 ? rc : PZ_OK;
  HostForm f(h, "block set insert");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  uint64_t w[kBsWords] = {0, 0};  // (the handle's last call has been waited for: the count is final)
  if ((rc = down(reinterpret_cast<uint8_t*>(w), h->words.ptr, sizeof w, "block set insert"))) return rc;
  if ((rc = reserve(h, w[kBsCount] + n > kBsMaxKeys ? kBsMaxKeys : w[kBsCount] + n, st.s))) return rc;
  const uint8_t* d_hashes = st.up(hashes, n * 32);
  const uint8_t* d_take = take ? st.up(take, n) : nullptr;
  if (st.rc) return st.rc;
  st.check(launch_insert(h, d_hashes, d_take, nullptr, nullptr, n, nullptr, st.s), "pz_bs_insert_kernel");
  return st.sync();
}

int pz_dev_block_set_reserve(pz_block_set* h, uint64_t min_keys, void* stream) {
  int rc = check_set(h);
  if (rc) return rc;
  if (min_keys > kBsMaxKeys) return fail(PZ_EINVAL, "a block set of %llu keys: above 2^30", (unsigned long long)min_keys);
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  return reserve(h, min_keys, static_cast<hipStream_t>(stream));
}

int pz_block_set_reserve(pz_block_set* h, uint64_t min_keys) {
  int rc = check_set(h);
  if (rc) return rc;
  if (min_keys > kBsMaxKeys) return fail(PZ_EINVAL, "a block set of %llu keys: above 2^30", (unsigned long long)min_keys);
  HostForm f(h, "block set reserve");
  if (f.rc) return f.rc;
  if ((rc = reserve(h, min_keys, f.st.s))) return rc;
  return f.st.sync();
}

uint64_t pz_block_parents_scratch_bytes(uint64_t nblocks) { return scratch_bytes(nblocks); }

int pz_dev_block_parents(pz_block_set* h, const pz_block_parents_batch* b, void* d_scratch, void* stream) {
  int rc = check_parents(h, b);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!d_scratch || !aligned16(d_scratch) || !aligned16(b->block_hash))
    return fail(PZ_EINVAL, "block parents: d_scratch and block_hash must be 16-B aligned device pointers");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  return launch_parents(h, *b, d_scratch, static_cast<hipStream_t>(stream));
}

int pz_block_parents(pz_block_set* h, const pz_block_parents_batch* hb) {
  int rc = check_parents(h, hb);
  if (rc) return rc < 0 ? rc : PZ_OK;
  const uint64_t nb = hb->nblocks, n = hb->natt;
  HostForm f(h, "block parents");
  if (f.rc) return f.rc;
  Stager& st = f.st;
  pz_block_parents_batch d = *hb;
  if (hb->nbytes) d.bytes = st.up(hb->bytes, hb->nbytes);
  d.bytes_beg = st.up(hb->bytes_beg, nb * 5);
  d.bytes_len = st.up(hb->bytes_len, nb * 5);
  d.slot_number = st.up(hb->slot_number, nb);
  d.block_hash = st.up(hb->block_hash, nb * 32);
  d.att_first = st.up(hb->att_first, nb + 1);
  d.block_status = st.up(hb->block_status, nb);
  if (n) {
    d.att_status = st.up(hb->att_status, n);
    if (hb->rec_status) d.rec_status = st.up(hb->rec_status, n);
  }
  d.parent_ok = st.up<uint8_t>(nullptr, nb);
  d.saved0 = st.up<uint8_t>(nullptr, nb);
  d.block_status_out = st.up<int32_t>(nullptr, nb);
  uint8_t* scr = st.up<uint8_t>(nullptr, scratch_bytes(nb));
  if (st.rc) return st.rc;
  if ((rc = launch_parents(h, d, scr, st.s))) return rc;
  st.down(hb->parent_ok, static_cast<const uint8_t*>(d.parent_ok), nb);
  st.down(hb->saved0, static_cast<const uint8_t*>(d.saved0), nb);
  st.down(hb->block_status_out, static_cast<const int32_t*>(d.block_status_out), nb);
  return st.sync();
}

int pz_dev_block_set_insert_walked(pz_block_set* h, const uint8_t* d_block_hash, const uint8_t* d_walk, const uint32_t* d_flags,
                                   uint64_t nblocks, uint64_t* d_count_out, void* stream) {
  int rc = check_hashes(h, d_block_hash, nblocks, "block set insert walked");
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!d_walk || !aligned16(d_block_hash))
    return fail(PZ_EINVAL, "block set insert walked: null walk, or block_hash not a 16-B aligned device pointer");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  hipError_t e = launch_insert(h, d_block_hash, nullptr, d_walk, d_flags, nblocks, d_count_out, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? PZ_OK : hip_fail(e, "pz_bs_insert_kernel");
}

#ifdef PZ_AB_BUILD
// (tools/blockparents_probe.py) pz_dev_block_parents and pz_dev_block_set_insert_walked with one event
// pair on each launch; each synchronises and returns its launches' milliseconds.
int pz_debug_block_parents_timed(pz_block_set* h, const pz_block_parents_batch* b, void* d_scratch, void* stream, float ms[3]) {
  int rc = check_parents(h, b);
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!ms || !d_scratch || !aligned16(d_scratch) || !aligned16(b->block_hash)) return fail(PZ_EINVAL, "null ms or misaligned pointers");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  Events ev;
  if ((rc = ev.create(4))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return ev.elapsed(launch_parents(h, *b, d_scratch, s, &ev), ms, nullptr, 3, s, "timed block parents");
}

int pz_debug_block_set_insert_walked_timed(pz_block_set* h, const uint8_t* d_block_hash, const uint8_t* d_walk, const uint32_t* d_flags,
                                           uint64_t nblocks, uint64_t* d_count_out, void* stream, float ms[1]) {
  int rc = check_hashes(h, d_block_hash, nblocks, "block set insert walked");
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!ms || !d_walk || !aligned16(d_block_hash)) return fail(PZ_EINVAL, "null ms / walk or misaligned block_hash");
  if ((rc = h->use())) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  Events ev;
  if ((rc = ev.create(2))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = launch_insert(h, d_block_hash, nullptr, d_walk, d_flags, nblocks, d_count_out, s, &ev);
  return ev.elapsed(e == hipSuccess ? PZ_OK : hip_fail(e, "pz_bs_insert_kernel"), ms, nullptr, 1, s, "timed insert walked");
}
#endif

}  // extern "C"
