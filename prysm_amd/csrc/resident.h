// What the resident objects show each other inside the library: pz_dev_state_recalc (recalc.hip)
// reads the vote cache's table (votecache.hip) and the pool's live columns and counts (attpool.hip)
// where they lie.  Not part of the C ABI.
#pragma once
#include "runtime.h"

namespace pz {

// What every resident handle is: a device, a lock, and the stream of its last call, which its
// reads, its host-pointer forms and its destructor wait for.
struct Resident {
  int device = 0;
  std::mutex mu;
  hipStream_t last = nullptr;
  // Before a handle is made: the device checked (gfx950, its context) and current.
  static int open(int device) {
    DeviceCtx* c;
    int rc = device_ctx(device, &c);
    if (rc) return rc;
    hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? PZ_OK : hip_fail(e, "hipSetDevice");
  }
  int use() const {
    hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? PZ_OK : hip_fail(e, "hipSetDevice");
  }
  int wait(const char* what) const {
    hipError_t e = hipStreamSynchronize(last);
    return e == hipSuccess ? PZ_OK : hip_fail(e, what);
  }
  // Waits for the last call and reads the handle's words (its counts and sticky error word).
  int settle(void* host, const DevBuf& words, size_t bytes, const char* what) const {
    int rc = wait(what);
    return rc ? rc : down(static_cast<uint8_t*>(host), words.ptr, bytes, what);
  }
  // A handle's destructor starts here, before it releases what a call in flight may still touch.
  void drain() const {
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(last);
  }
};

// A host-pointer form on a handle, in this order: use the device, lock the handle, wait for its
// last stream (the staging stream is the library's own, non-blocking: the caller cannot order a
// call on it against the handle's earlier calls, so the library does), take the device context,
// lock it, make its stream, hand out a Stager.  rc != PZ_OK: the call ends with it.  A host form
// of an entry point without a handle (h NULL) is the same from "take the device context" on.
struct HostForm {
  int rc;
  std::unique_lock<std::mutex> handle, ctx;
  Stager st{nullptr, nullptr};
  explicit HostForm(Resident* h = nullptr, const char* what = "") {
    DeviceCtx* c;
    if (h) {
      if ((rc = h->use())) return;
      handle = std::unique_lock<std::mutex>(h->mu);
      if ((rc = h->wait(what))) return;
    }
    if ((rc = h ? device_ctx(h->device, &c) : acquire(&c))) return;
    ctx = std::unique_lock<std::mutex>(c->mu);
    if ((rc = c->ensure_stream())) return;
    st.c = c, st.s = c->stream;
  }
};

// A handle as its Resident base, for a host-pointer form written outside the handle's own file
// (wire_state.hip); defined beside each struct.
Resident* resident_of(pz_att_pool* h);
Resident* resident_of(pz_recalc_state* h);
Resident* resident_of(pz_recent_hashes* h);

// The recent-hashes ring for a launch sequence written outside its file (blockcycle.hip), under the
// handle's lock: the live set's 129 x 32 bytes, and the walk's roll (blockwalk.hip) -- the other set
// becomes log entries [ncand, ncand + 129) with ncand = result[1], unless bit 0 of *flags is set --
// after which the sets are swapped and s is the stream the ring's reads wait for.
const uint8_t* recent_hashes_live(pz_recent_hashes* h);
hipError_t recent_hashes_roll(pz_recent_hashes* h, const uint8_t* log, const uint64_t* result, const uint32_t* flags, uint64_t nblocks,
                              hipStream_t s);

// The two entry families over a run of blocks against the ring, pz_block_walk (blockwalk.hip) and
// pz_block_cycle (blockcycle.hip): what their batch structs B share by name -- nblocks, slot_number,
// report, block_hash, lag, natt, att_block, vote_status, pend_take, parents_start, walk, base,
// result, log, flags -- checked and staged once.  `what` is "block walk" or "block cycle"; a family
// adds only its own members, its result's width and its empty run's record.

// Before any launch.  1: an empty run, nothing to launch.
template <class B>
int check_block_run(const pz_recent_hashes* h, const B* b, bool device_form, const char* what) {
  if (!h || !b) return fail(PZ_EINVAL, "%s: null handle or batch", what);
  if (b->nblocks >= (1ull << 31)) return fail(PZ_EINVAL, "nblocks %llu: 2^31 blocks or more", (unsigned long long)b->nblocks);
  if (b->lag > 1) return fail(PZ_EINVAL, "lag %llu: 0 or 1", (unsigned long long)b->lag);
  if (b->nblocks == 0) return 1;
  if (!b->slot_number || !b->report || !b->block_hash || !b->walk || !b->base || !b->result)
    return fail(PZ_EINVAL, "%s: null slot_number / report / block_hash / walk / base / result", what);
  if (device_form && !b->log) return fail(PZ_EINVAL, "%s: null log", what);
  if (device_form && (!aligned16(b->block_hash) || !aligned16(b->log)))
    return fail(PZ_EINVAL, "%s: block_hash and log must be 16-B aligned device pointers", what);
  if (b->natt && (!b->att_block || !b->vote_status || !b->parents_start))
    return fail(PZ_EINVAL, "%s: null att_block / vote_status / parents_start", what);
  return PZ_OK;
}

// The device form behind its check's rc: the family's launches (launch(h, batch, stream, events))
// on the caller's stream, under the handle's lock.
template <class B, class Launch>
int enqueue_block_run(int rc, pz_recent_hashes* h, const B* b, void* stream, const char* what, Launch launch) {
  if (rc) return rc < 0 ? rc : PZ_OK;
  Resident* r = resident_of(h);
  if ((rc = r->use())) return rc;
  std::lock_guard<std::mutex> lk(r->mu);
  const hipError_t e = launch(h, *b, static_cast<hipStream_t>(stream), nullptr);
  return e == hipSuccess ? PZ_OK : hip_fail(e, what);
}

#ifdef PZ_AB_BUILD
// (tools/blockwalk_probe.py, tools/blockcycle_probe.py) The same with one event pair on each of the
// three launches; synchronises and returns the milliseconds of scan, rows and roll in ms[0..3).
template <class B, class Launch>
int timed_block_run(int rc, pz_recent_hashes* h, const B* b, void* stream, float ms[3], const char* what, Launch launch) {
  if (rc) return rc < 0 ? rc : PZ_OK;
  if (!ms) return fail(PZ_EINVAL, "%s: null ms", what);
  Resident* r = resident_of(h);
  if ((rc = r->use())) return rc;
  std::lock_guard<std::mutex> lk(r->mu);
  Events ev;
  if ((rc = ev.create(4))) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const hipError_t e = launch(h, *b, s, &ev);
  return ev.elapsed(e == hipSuccess ? PZ_OK : hip_fail(e, what), ms, nullptr, 3, s, what);
}
#endif

// The host form's staging: d = *hb with the shared members on the device (result_words words of
// result, log_bytes of log), and after the launches the shared outputs back (log where hb has one).
template <class B>
void stage_block_run(Stager& st, const B* hb, B& d, uint64_t result_words, uint64_t log_bytes) {
  const uint64_t nb = hb->nblocks, n = hb->natt;
  d = *hb;
  d.slot_number = st.up(hb->slot_number, nb);
  d.report = st.up(hb->report, nb);
  d.block_hash = st.up(hb->block_hash, nb * 32);
  if (n) {
    d.att_block = st.up(hb->att_block, n);
    d.vote_status = st.up(hb->vote_status, n);
    d.parents_start = st.up(hb->parents_start, n);
    if (hb->pend_take) d.pend_take = st.up(hb->pend_take, n);
  }
  d.walk = st.up<uint8_t>(nullptr, nb);
  d.base = st.up<uint64_t>(nullptr, nb);
  d.result = st.up<uint64_t>(nullptr, result_words);
  d.log = st.up<uint8_t>(nullptr, log_bytes);
  if (hb->flags) d.flags = st.up(hb->flags, 1);
}
template <class B>
void unstage_block_run(Stager& st, const B* hb, const B& d, uint64_t result_words, uint64_t log_bytes) {
  st.down(hb->walk, d.walk, hb->nblocks);
  st.down(hb->base, d.base, hb->nblocks);
  st.down(hb->result, d.result, result_words);
  if (hb->log) st.down(hb->log, d.log, log_bytes);
  st.down(hb->parents_start, d.parents_start, hb->natt);
}

// The vote cache's lookup side: device pointers into its live buffer set, valid until the cache's
// next reserve or retain (stream-ordered like every call on the handle).
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

// The pool's live buffer set and its device counts ([7], rows first), valid until the next prune or reserve.
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

// The recalc state's words (scalars[PZ_RS_COUNT], then the sticky error word) and record columns,
// valid for the handle's lifetime.
struct RsView {
  int device;
  uint32_t nrec, stride;
  const uint64_t* words;
  const uint64_t* rec_dynasty;
  const uint64_t* rec_slot;
  const uint8_t* rec_hash;
  const uint32_t* rec_hash_len;
};
// Fills *v; with record, s becomes the stream the handle's reads wait for (wire_state.hip).
int recalc_state_view(pz_recalc_state* h, RsView* v, hipStream_t s, bool record);

}  // namespace pz
