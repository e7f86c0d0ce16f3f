// sf_scratch.h -- what owns a context's scratch memory: device and pinned buffers that only grow, the pinned/device pair behind
// a per-item read-back, the pinned table that one copy uploads, and HIP events and streams.  Each frees what it holds when the
// context is deleted (sfh_destroy: the device set, the context's stream idle), so a new buffer is one member of sfh_ctx.
// Part of sf_capi.hip's translation unit, which defines the three functions declared first.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/starflate_hip.h"

namespace {
int fail(sfh_ctx* c, int code, const char* what, hipError_t e);  // the message into the context; returns code
int wait_idle(sfh_ctx* ctx);                                     // the host waits for the last call's device work
int order_behind_last_call(sfh_ctx* ctx, hipStream_t s);         // s waits for it, on the device
}  // namespace

#define SF_HIP(call, what)                                       \
  do {                                                           \
    hipError_t _e = (call);                                      \
    if (_e != hipSuccess) return fail(ctx, SFH_E_HIP, what, _e); \
  } while (0)

namespace sf {
namespace scratch {

// A grow-only array of T on the device, or (Pinned) in pinned host memory.  No over-allocation, and grow() waits for nothing:
// whoever may still read the old block is the caller's to wait for.
template <class T, bool Pinned = false>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }
  operator T*() const { return p; }
  void release() {
    if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  // p holds at least n elements afterwards.  The old block is freed first (the peak never holds both); on failure the buffer is empty.
  int grow(sfh_ctx* ctx, size_t n, const char* what) {
    if (cap >= n) return SFH_OK;
    release();
    const hipError_t e = Pinned ? hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, n * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return fail(ctx, SFH_E_NOMEM, what, e);
    }
    cap = n;
    return SFH_OK;
  }
};
template <class T>
using Pinned = Buf<T, true>;

// A device array with its pinned twin: what a call reads back per item.
template <class T>
struct Pair {
  Buf<T> d;
  Pinned<T> h;
  int grow(sfh_ctx* ctx, size_t n, const char* what) {
    if (int rc = d.grow(ctx, n, what)) return rc;
    return h.grow(ctx, n, what);
  }
};

// An event or a stream, created where it is first needed (into .h) and destroyed with the context.
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  ~Handle() {
    if (h) (void)Destroy(h);
  }
  operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

// The descriptor tables of a call, built in pinned memory (h) and uploaded to their device twin (d) with one copy; the next
// call refills the pinned rows only once that copy (ev) has read them.
struct Stager {
  Pinned<uint8_t> h;
  Buf<uint8_t> d;
  Event ev;
  bool pending = false;
  const char *what_h, *what_d;
  Stager(const char* pinned, const char* device) : what_h(pinned), what_d(device) {}
  ~Stager() {
    if (ev) (void)hipEventSynchronize(ev);  // (the copy reads h)
  }
  // h holds `bytes` and d `bytes + device_only` afterwards, and the previous call's copy has read h -- and, when d had to grow,
  // its kernels have read d.
  int stage(sfh_ctx* ctx, size_t bytes, size_t device_only = 0) {
    if (!ev) SF_HIP(hipEventCreateWithFlags(&ev.h, hipEventDisableTiming), "event");
    if (pending) SF_HIP(hipEventSynchronize(ev), "wait for the previous call's table copy");
    pending = false;
    if (int rc = h.grow(ctx, bytes, what_h)) return rc;
    if (d.cap < bytes + device_only)
      if (int rc = wait_idle(ctx)) return rc;
    return d.grow(ctx, bytes + device_only, what_d);
  }
  // ... and once h is filled: the call takes its place behind the previous one and the first `bytes` go up
  int upload(sfh_ctx* ctx, size_t bytes, hipStream_t s) {
    if (int rc = order_behind_last_call(ctx, s)) return rc;
    SF_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s), what_d);
    SF_HIP(hipEventRecord(ev, s), "event");
    pending = true;
    return SFH_OK;
  }
};

}  // namespace scratch
}  // namespace sf
