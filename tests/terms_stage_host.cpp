// Host build of csrc/view_stage.h for tests/test_imitation_terms.py: the staging block of the fourth view (csrc/views.hip
// dm_batch_imitation_terms: qpos, qvel, frame, cycle, env_ids in, the terms rows out), compiled with a host C++ compiler under
// -fsanitize=address,undefined and driven through every combination of present and absent arrays, for host and for device callers.
// Test infrastructure only (libdmenv.so has no CPU path).
//
// usage: terms_stage_host      (no arguments; exit status 0 and one summary line when every layout holds, else the first failure on stderr and 1)
//   Per layout: every staged region starts at a multiple of 256 and ends inside the block, no two overlap, absent arrays and a device
//   caller's own arrays take no region and are handed back as given.  Then the block is allocated with exactly `total` bytes and every region
//   filled through the pointer its caller gets: a byte outside the block is the sanitizer's to report, a byte in another region shows in the
//   read-back.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "view_stage.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "terms_stage_host: %s fails (host %d, mask %u, n %zu)\n", #cond, (int)host, mask, n); return 1; } } while (0)

struct Arr { dmst::Dir dir; size_t bytes; };

int main() {
  const size_t ns[] = {1, 5, 66, 863, 8192};
  size_t layouts = 0;
  for (size_t n : ns) {
    const std::vector<Arr> arrs = {{dmst::COPY_IN, n * 35 * 8}, {dmst::COPY_IN, n * 34 * 8}, {dmst::COPY_IN, n * 4}, {dmst::COPY_IN, n * 4}, {dmst::COPY_IN, n * 4},
                                   {dmst::COPY_OUT, n * 28 * 8}};
    const size_t na = arrs.size();
    for (int host = 0; host < 2; host++)
      for (unsigned mask = 0; mask < 1u << na; mask++) {          // bit i: array i is given
        std::vector<std::vector<unsigned char>> user(na);
        dmst::Layout lay(host != 0);
        size_t sum = 0;
        for (size_t i = 0; i < na; i++) {
          const bool given = mask >> i & 1;
          if (given) user[i].resize(arrs[i].bytes);
          CHECK(lay.add(arrs[i].dir, given ? user[i].data() : nullptr, arrs[i].bytes) == (int)i);
          const bool st = host && given;
          CHECK(lay.r[i].staged == st && lay.r[i].dir == arrs[i].dir && lay.r[i].bytes == arrs[i].bytes);
          if (st) sum += (arrs[i].bytes + 255) / 256 * 256;
        }
        CHECK(lay.n == (int)na && !lay.full && lay.total == sum && (host || lay.total == 0));
        size_t end = 0;                                            // staged regions: aligned, in the order declared, disjoint, inside the block
        for (size_t i = 0; i < na; i++) {
          const dmst::Region& x = lay.r[i];
          if (!x.staged) continue;
          CHECK(x.off % 256 == 0 && x.bytes > 0 && x.off >= end && x.off + x.bytes <= lay.total);
          end = x.off + x.bytes;
        }
        unsigned char* base = (unsigned char*)std::malloc(lay.total ? lay.total : 1);
        CHECK(base != nullptr);
        for (size_t i = 0; i < na; i++) {
          unsigned char* p = (unsigned char*)lay.at((int)i, base);
          if (!lay.r[i].staged) { CHECK(p == (user[i].empty() ? nullptr : user[i].data())); continue; }      // as given: the caller's own array, or none
          CHECK(p == base + lay.r[i].off && lay.r[i].user == (void*)user[i].data());
          std::memset(p, (int)(i + 1), arrs[i].bytes);
        }
        for (size_t i = 0; i < na; i++)
          if (lay.r[i].staged) for (size_t j = 0; j < lay.r[i].bytes; j++) CHECK(base[lay.r[i].off + j] == (unsigned char)(i + 1));
        std::free(base);
        layouts++;
      }
  }
  std::printf("terms_stage_host: %zu layouts hold\n", layouts);
  return 0;
}
