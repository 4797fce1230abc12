// vvcx_host.h — what the host code of the library (vvcx_api*.hip and the files behind them, vvcx_lmcs.hip) shares: how an entry point selects its device, how a failed HIP call becomes
// VVCX_ERR_DEVICE, and the one type that owns device memory.  Host only: nothing here is seen by a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include "vvcx.h"

// vvcx_api.hip: sets what vvcx_last_error returns
extern "C" __attribute__((visibility("hidden"))) int vvcx_fail_msg_(int code, const char *msg);

static inline int vvcx_hip_fail_(const char *what, hipError_t e)
{
  char msg[512]; snprintf(msg, sizeof msg, "%s: %s", what, hipGetErrorString(e));
  return vvcx_fail_msg_(VVCX_ERR_DEVICE, msg);
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return vvcx_hip_fail_(#x, e_); } while (0)

// every entry point works on the device of its handle / its argument and leaves the caller's current device as it found it
struct DevGuard {
  int prev; bool ok;
  explicit DevGuard(int dev) : prev(-1), ok(false) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; ok = hipSetDevice(dev) == hipSuccess; }
  ~DevGuard() { if (prev >= 0) (void) hipSetDevice(prev); }
  DevGuard(const DevGuard &) = delete; DevGuard &operator=(const DevGuard &) = delete;
};
static inline int vvcx_no_device_(int dev)
{
  char msg[64]; snprintf(msg, sizeof msg, "hipSetDevice(%d) failed", dev);
  return vvcx_fail_msg_(VVCX_ERR_DEVICE, msg);
}
// first statement of an entry point (returning int) that touches the device: the rest of the function runs on `dev`
#define ON_DEVICE(dev) DevGuard dev_guard_(dev); if (!dev_guard_.ok) return vvcx_no_device_(dev)

// Owning device buffer of `cap` elements of T; freed by the destructor.  A failed allocation leaves it empty (null, capacity 0), so the next reserve tries again
// and nothing is ever launched on a pointer whose allocation failed.
template <typename T> struct DevBuf {
  T *p = nullptr; size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() { if (p) (void) hipFree(p); p = nullptr; cap = 0; }
  // exactly n elements (a block of its own also for n = 0); what was held before is freed first: the peak is the larger of the two, not their sum
  hipError_t alloc(size_t n)
  {
    release();
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, (n ? n : 1) * sizeof(T));
    if (e == hipSuccess) { p = (T *) q; cap = n; }
    return e;
  }
  // grow on demand: nothing to do while n fits; *grew tells the caller that the contents are new (uninitialised) memory
  hipError_t reserve(size_t n, bool *grew = nullptr)
  {
    if (grew) *grew = false;
    if (n <= cap) return hipSuccess;
    const hipError_t e = alloc(n);
    if (grew) *grew = e == hipSuccess;
    return e;
  }
};
