// view_stage.h — the layout of a view call's staging block (views.hip Stage).  Plain C++ without a HIP call or an allocation:
// the CPU tests build it with a host compiler under the sanitizers (tests/stage_host.cpp).  Private to csrc/.
#pragma once
#include <cstddef>

namespace dmst {
enum Dir { COPY_IN, COPY_OUT, SCRATCH };     // copied to the device before the launch | copied back after it | device-only
struct Region { Dir dir; void* user; size_t bytes, off; bool staged; };

struct Layout {
  static constexpr int MAX = 8;    // (render declares seven)
  bool host;                       // the caller's arrays are host arrays (DM_PTR_HOST)
  Region r[MAX]; int n = 0;
  bool full = false;               // an array was declared beyond MAX: the call must not go on (Stage::commit refuses it)
  size_t total = 0;                // bytes of the block: the staged regions in the order declared, each at a multiple of 256
  explicit Layout(bool host_caller) : host(host_caller) {}
  // declare an array -> its index (-1 and `full` when the table has no room).  A host caller's array and scratch are staged; a device caller's own array and an absent one (NULL) are not
  int add(Dir dir, const void* user, size_t bytes) {
    if (n == MAX) { full = true; return -1; }
    const bool staged = dir == SCRATCH || (host && user);
    r[n] = Region{dir, const_cast<void*>(user), bytes, total, staged};
    if (staged) total += (bytes + 255) / 256 * 256;
    return n++;
  }
  // what the kernel gets for array i once the block is at `base`: its region, or the caller's pointer as given
  void* at(int i, unsigned char* base) const { return r[i].staged ? base + r[i].off : r[i].user; }
};
}  // namespace dmst
