// Host build of csrc/view_stage.h for tests/test_views.py: the layout of a view call's staging block, compiled with a host C++ compiler under
// -fsanitize=address,undefined and driven through every combination of present and absent arrays that the three views (csrc/views.hip) can
// declare, for host and for device callers.  Test infrastructure only (libdmenv.so has no CPU path).
//
// usage: stage_host      (no arguments; exit status 0 and one summary line when every layout holds, else the first failure on stderr and 1)
//   Per layout: every region starts at a multiple of 256 and ends inside the block, no two regions overlap, absent arrays and a device caller's
//   own arrays take no region and are handed back as given, scratch always takes one.  Then the block is allocated with exactly `total` bytes
//   and every region filled through the pointer its caller gets: a byte outside the block is the sanitizer's to report, a byte in
//   another region shows in the read-back.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "view_stage.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "stage_host: %s fails (view %d, host %d, mask %u, n %zu)\n", #cond, view, (int)host, mask, n); return 1; } } while (0)

struct Arr { dmst::Dir dir; size_t bytes; };

int main() {
  const size_t ns[] = {1, 2, 6, 18, 863};
  size_t layouts = 0;
  for (int view = 0; view < 3; view++)
    for (size_t n : ns) {
      const size_t npix = n * 8 * 8;
      std::vector<Arr> arrs;
      if (view == 0) arrs = {{dmst::SCRATCH, n * 200}, {dmst::COPY_IN, n * 35 * 8}, {dmst::COPY_IN, n * 4}, {dmst::COPY_OUT, npix * 3}, {dmst::COPY_OUT, npix * 4}, {dmst::COPY_OUT, npix * 4}, {dmst::COPY_OUT, n * 16 * 12 * 8}};
      if (view == 1) arrs = {{dmst::COPY_IN, n * 35 * 8}, {dmst::COPY_IN, n * 34 * 8}, {dmst::COPY_IN, n * 8}, {dmst::COPY_IN, n * 4}, {dmst::COPY_OUT, n * 171 * 8}};
      if (view == 2) arrs = {{dmst::COPY_IN, n * 35 * 8}, {dmst::COPY_IN, n * 4}, {dmst::COPY_OUT, n * 4}};
      const size_t na = arrs.size();
      for (int host = 0; host < 2; host++)
        for (unsigned mask = 0; mask < 1u << na; mask++) {        // bit i: array i is given
          std::vector<std::vector<unsigned char>> user(na);
          dmst::Layout lay(host != 0);
          size_t sum = 0;
          for (size_t i = 0; i < na; i++) {
            const bool given = arrs[i].dir != dmst::SCRATCH && (mask >> i & 1);
            if (given) user[i].resize(arrs[i].bytes);
            CHECK(lay.add(arrs[i].dir, given ? user[i].data() : nullptr, arrs[i].bytes) == (int)i);
            const bool st = arrs[i].dir == dmst::SCRATCH || (host && given);
            CHECK(lay.r[i].staged == st && lay.r[i].dir == arrs[i].dir && lay.r[i].bytes == arrs[i].bytes);
            if (st) sum += (arrs[i].bytes + 255) / 256 * 256;
          }
          CHECK(lay.n == (int)na && lay.total == sum);
          size_t end = 0;                                          // staged regions: aligned, in the order declared, disjoint, inside the block
          for (size_t i = 0; i < na; i++) {
            const dmst::Region& x = lay.r[i];
            if (!x.staged) continue;
            CHECK(x.off % 256 == 0 && x.bytes > 0 && x.off >= end && x.off + x.bytes <= lay.total);
            end = x.off + x.bytes;
          }
          if (mask == 0) {                                         // a table that is full refuses, writes nothing and stays as it was
            dmst::Layout big = lay;
            while (big.n < dmst::Layout::MAX) CHECK(big.add(dmst::SCRATCH, nullptr, 1) == big.n - 1 && !big.full);
            const size_t t = big.total;
            CHECK(big.add(dmst::SCRATCH, nullptr, 1) == -1 && big.full && big.n == dmst::Layout::MAX && big.total == t);
          }
          unsigned char* base = (unsigned char*)std::malloc(lay.total ? lay.total : 1);
          CHECK(base != nullptr);
          for (size_t i = 0; i < na; i++) {
            unsigned char* p = (unsigned char*)lay.at((int)i, base);
            if (!lay.r[i].staged) { CHECK(p == (user[i].empty() ? nullptr : user[i].data())); continue; }      // as given: the caller's own array, or none
            CHECK(p == base + lay.r[i].off && lay.r[i].user == (user[i].empty() ? nullptr : (void*)user[i].data()));
            std::memset(p, (int)(i + 1), arrs[i].bytes);
          }
          for (size_t i = 0; i < na; i++)
            if (lay.r[i].staged) for (size_t j = 0; j < lay.r[i].bytes; j++) CHECK(base[lay.r[i].off + j] == (unsigned char)(i + 1));
          std::free(base);
          layouts++;
        }
    }
  std::printf("stage_host: %zu layouts hold\n", layouts);
  return 0;
}
