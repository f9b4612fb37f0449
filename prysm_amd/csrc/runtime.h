// Internal runtime helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/prysm_hip.h"

namespace pz {

int fail(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

// Grow-only device allocation (padded by 256 B so CSR readers may over-read 4 bytes).
struct DevBuf {
  void* ptr = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes);
  void release();
  // A handle's creation, synchronous: `bytes` set to `byte`, then the first host_bytes from host.
  int fill(size_t bytes, int byte, const char* what, const void* host = nullptr, size_t host_bytes = 0) {
    int rc = reserve(bytes);
    if (rc) return rc;
    hipError_t e = hipMemset(ptr, byte, bytes);
    if (e == hipSuccess && host && host_bytes) e = hipMemcpy(ptr, host, host_bytes, hipMemcpyHostToDevice);
    return e == hipSuccess ? PZ_OK : hip_fail(e, what);
  }
};

struct DeviceCtx {
  int device = 0;
  bool checked = false;  // gfx950 verified
  std::mutex mu;
  hipStream_t stream = nullptr;
  DevBuf in, out, aux;
  DevBuf slot[24];  // staging for the T/R host-pointer entry points
  static DeviceCtx* get(int dev);
  int ensure_stream();
};

int acquire(DeviceCtx** out);
int device_ctx(int device, DeviceCtx** out);

constexpr uint64_t r16(uint64_t x) { return (x + 15) & ~15ull; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Copies host arrays into the context's staging slots and tracks the stream.
struct Stager {
  DeviceCtx* c;
  hipStream_t s;
  int next = 0;
  int rc = PZ_OK;
  std::vector<uint64_t> kept[8];  // host arrays built for an upload: they live until sync()
  int nkept = 0;

  // The next slot, holding `bytes` (16 at least): copied from host (NULL: left as they are) or,
  // with byte >= 0, set to it.  Fails the call when the context's slots have run out.
  void* put(const void* host, size_t bytes, int byte = -1) {
    constexpr int kSlots = sizeof c->slot / sizeof c->slot[0];
    if (!rc && next >= kSlots) rc = fail(PZ_EINVAL, "a call staged more than the %d slots of its device context", kSlots);
    if (rc || (rc = c->slot[next].reserve(bytes ? bytes : 16))) return nullptr;
    void* d = c->slot[next++].ptr;
    hipError_t e = hipSuccess;
    if (bytes && byte >= 0) e = hipMemsetAsync(d, byte, bytes, s);
    else if (bytes && host) e = hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) rc = hip_fail(e, byte >= 0 ? "hipMemsetAsync" : "hipMemcpyAsync H2D");
    return rc ? nullptr : d;
  }
  template <typename T>
  T* up(const T* host, size_t count) { return static_cast<T*>(put(host, count * sizeof(T))); }
  template <typename T>
  T* zeros(size_t count, int byte = 0) { return static_cast<T*>(put(nullptr, count * sizeof(T), byte)); }
  std::vector<uint64_t>& keep() {
    if (nkept == 8) rc = fail(PZ_EINVAL, "a call kept more than 8 host arrays"), --nkept;
    return kept[nkept++];
  }
  template <typename T>
  int down(T* host, const T* dev, size_t count) {
    if (rc || !count) return rc;
    hipError_t e = hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync D2H");
    return rc;
  }
  int sync() {
    if (rc) return rc;
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    return rc;
  }
  int check(hipError_t e, const char* what) {
    if (!rc && e != hipSuccess) rc = hip_fail(e, what);
    return rc;
  }
};

// A plain synchronous read of count values (a NULL host or no value: nothing).
template <typename T>
int down(T* host, const void* dev, uint64_t count, const char* what) {
  if (!host || !count) return PZ_OK;
  hipError_t e = hipMemcpy(host, dev, (size_t)(count * sizeof(T)), hipMemcpyDeviceToHost);
  return e == hipSuccess ? PZ_OK : hip_fail(e, what);
}

// The events of a timed entry of the A/B library (tools/*_probe.py): created together, destroyed
// together, also when a create fails half-way.  The product's enqueues take a null set.
#ifdef PZ_AB_BUILD
struct Events {
  hipEvent_t ev[8];
  int n = 0;
  int create(int count) {
    for (; n < count; ++n)
      if (hipEventCreate(&ev[n]) != hipSuccess) return fail(PZ_EDEVICE, "hipEventCreate");
    return PZ_OK;
  }
  ~Events() {
    for (int k = 0; k < n; ++k) (void)hipEventDestroy(ev[k]);
  }
  // Drains s; after an enqueue that returned PZ_OK, ms[k] = from event pairs[k] (NULL: k) to the
  // one after it.  The timed entry's return value.
  int elapsed(int rc, float* ms, const int* pairs, int npairs, hipStream_t s, const char* what) {
    hipError_t e = hipStreamSynchronize(s);
    for (int k = 0; k < npairs && !rc && e == hipSuccess; ++k) {
      const int from = pairs ? pairs[k] : k;
      e = hipEventElapsedTime(&ms[k], ev[from], ev[from + 1]);
    }
    return rc ? rc : e == hipSuccess ? PZ_OK : hip_fail(e, what);
  }
};
inline void stamp(Events* ev, int k, hipStream_t s) {
  if (ev) (void)hipEventRecord(ev->ev[k], s);
}
#else
struct Events;
inline void stamp(Events*, int, hipStream_t) {}
#endif

// Host CSR offsets rebased to 0 (so device buffers hold only the referenced bytes).
inline std::vector<uint64_t> rebase(const uint64_t* offs, uint64_t n) {
  std::vector<uint64_t> r(n + 1);
  for (uint64_t i = 0; i <= n; ++i) r[i] = offs[i] - offs[0];
  return r;
}

inline int check_csr(const uint64_t* offs, uint64_t n, const char* what) {
  if (!offs) return fail(PZ_EINVAL, "%s offsets are null", what);
  for (uint64_t i = 0; i < n; ++i)
    if (offs[i + 1] < offs[i]) return fail(PZ_EINVAL, "%s offsets not monotone at %llu", what, (unsigned long long)i);
  return PZ_OK;
}

}  // namespace pz
