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
