// host_common.h — what the host sides of libdmenv.so's units (dmenv.hip, views.hip, learner.hip) share: the error report behind dm_last_error and a few
// helpers of argument checking and scratch layout.  Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "dmenv.h"

// the text dm_last_error returns: ONE object per thread for the whole library (defined in dmenv.hip), whichever unit's entry point failed
extern thread_local std::string g_err;
inline int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(DM_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool have_device() { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return false; } return n > 0; }
// make the device that owns `p` current: an entry point without a batch launches on the device of its arrays (the caller's stream belongs to it),
// whatever the thread's current device is
inline int set_device_of(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) == hipSuccess) { if (hipSetDevice(at.device) != hipSuccess) return DM_EHIP; }
  else (void)hipGetLastError();
  return DM_OK;
}
