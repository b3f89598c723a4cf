// wave_fibres.h — TEST INFRASTRUCTURE: the fibre runner of the wave testbench (wave_testbench.h), once.  It defines dmw::bench() and the 64 ucontext
// fibres that a wavefront's lanes run on, so exactly one translation unit of a program includes it: emu_main.cpp (and with it emu_clips.cpp and
// emu_push.cpp) and the two horizon twins through host_batch.h, tests/terms_host.cpp directly.
//
// DM_FIBRE_STACK, set ahead of the include, is a fibre's stack in bytes (default 1 << 20, the libraries loaded into Python and terms_host).  The programs built
// with the sanitizers set 1 << 18 (host_rollout.h): the sanitizer's swapcontext clears the shadow of the whole stack at every switch, so it is kept small — and
// its high-water mark is checked at the end, since one fibre's overflow would land in its neighbour's stack, where the sanitizer does not look.  Every stack is
// filled with a pattern when it is allocated, so any program can ask for the deepest one used (stack_high_water).
#pragma once
#include <ucontext.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "wave_testbench.h"

#ifndef DM_FIBRE_STACK
#define DM_FIBRE_STACK (1 << 20)
#endif

namespace dmw {
static WaveBench g_bench;
WaveBench& bench() { return g_bench; }
}  // namespace dmw

namespace {
constexpr size_t STACK = DM_FIBRE_STACK;
constexpr unsigned char STACK_FILL = 0xA5;
ucontext_t g_main, g_fib[64];
bool g_done[64];
std::function<void(int)>* g_body;
char* g_stacks;                      // all 64 stacks, allocated by the first run_wave; a stand-alone program may free() it at exit

void yield_to_main() { swapcontext(&g_fib[dmw::g_bench.cur_lane], &g_main); }
void fibre_entry() {
  const int l = dmw::g_bench.cur_lane;
  (*g_body)(l);
  g_done[l] = true;
  swapcontext(&g_fib[l], &g_main);
}
// run body(lane) on 64 fibres to completion
void run_wave(std::function<void(int)> body) {
  if (!g_stacks) { g_stacks = (char*)malloc(STACK * 64); std::memset(g_stacks, STACK_FILL, STACK * 64); }
  g_body = &body;
  dmw::g_bench.arrived = 0; dmw::g_bench.gen = 0; dmw::g_bench.yield_fn = yield_to_main;
  for (int l = 0; l < 64; l++) {
    g_done[l] = false;
    getcontext(&g_fib[l]);
    g_fib[l].uc_stack.ss_sp = g_stacks + STACK * l; g_fib[l].uc_stack.ss_size = STACK; g_fib[l].uc_link = &g_main;
    makecontext(&g_fib[l], fibre_entry, 0);
  }
  for (;;) {
    bool all = true;
    for (int l = 0; l < 64; l++) if (!g_done[l]) { all = false; dmw::g_bench.cur_lane = l; swapcontext(&g_main, &g_fib[l]); }
    if (all) break;
  }
}

// bytes of the deepest fibre stack ever used (stacks grow downwards: the first byte from the bottom that lost the fill pattern)
[[maybe_unused]] size_t stack_high_water() {
  size_t worst = 0;
  for (int l = 0; l < 64 && g_stacks; l++) {
    const unsigned char* p = (const unsigned char*)g_stacks + STACK * l;
    size_t k = 0;
    while (k < STACK && p[k] == STACK_FILL) k++;
    worst = std::max(worst, STACK - k);
  }
  return worst;
}
}  // namespace
