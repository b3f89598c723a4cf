// rng.h — the counter-based Gaussian noise of the policy: the rollout's action sample (policy_kernel.h, dm_policy_act) and the stochastic
// action of behaviour cloning (pg_kernel.h MODE_BC) draw from this one definition.  normal_from(seed, counter, idx) is a pure function of
// its arguments: a launch may compute any element in any thread, and tests/bc_numpy.py restates it bit for bit up to the float32 Box-Muller.
#pragma once
#include <hip/hip_runtime.h>

namespace dmr {

// splitmix64's finaliser
__device__ inline unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// standard normal from a counter: two 24-bit uniforms, Box-Muller
__device__ inline float normal_from(unsigned long long seed, unsigned long long counter, unsigned idx) {
  const unsigned long long h = mix64(mix64(seed ^ (counter * 0xD1342543DE82EF95ull)) + idx);
  const float u1 = ((float)((h >> 40) & 0xFFFFFF) + 1.0f) * (1.0f / 16777216.0f);     // (0, 1]
  const float u2 = (float)((h >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

}  // namespace dmr
