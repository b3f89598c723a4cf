// policy_wave_launch_order.h — the policy step for the four environments of a packed wave (policy_kernel.h policy_wave4: the same lane -> hidden-unit map,
// scratch layout and weight stream) with every sum formed in the order of the policy LAUNCH (k_policy_act / dm_policy_act): inputs four at a time,
// acc += x0 w0 + x1 w1 + x2 w2 + x3 w3 — dense32's and the output layer's own expression — where policy_wave4 adds one product after the other.
// For k_rollout_packed_term (DM_OPT_HORIZON_TERMINATION): with early termination on, the step launches run the policy as that launch behind the termination
// launch, and the horizon kernel's actions and values are to be theirs bit for bit, not to float32 rounding.
#pragma once
#include "policy_kernel.h"

namespace dmp {

// x.x w0 + x.y w1 + x.z w2 + x.w w3 as the launch's code objects form it (the compiler's contraction of that expression, read from
// k_policy_act's instructions: one product, three fused multiply-adds onto it, and the caller adds the group to its accumulator unfused).  Written out
// with contraction off so that no other context can fuse it another way.
// This pins THIS file, not the launch: a compiler that contracts dense32's expression another way, or an edit to dense32 / the launch's output layer, breaks
// the identity, and tests/test_gpu_horizon_termination.py (the fused-policy and collector tests, float64 and float32 libraries) is what notices.  The float32
// library contracts inside one source expression (-ffp-contract=on), which gives dense32's expression the same shape: fma(x.x, w0, x.y w1), two more, an add.
__device__ inline float dot4_launch(const float4 x, float w0, float w1, float w2, float w3) {
#pragma clang fp contract(off)
  float t = x.y * w1;
  t = __builtin_fmaf(x.x, w0, t);
  t = __builtin_fmaf(x.z, w2, t);
  t = __builtin_fmaf(x.w, w3, t);
  return t;
}
// acc + group, unfused
__device__ inline float add_group(float acc, float t) {
#pragma clang fp contract(off)
  return acc + t;
}

template <int K, int UNROLL>
__device__ inline void dense4_wave4_by4(const float* __restrict__ W, const float* __restrict__ bias, const float* (&in)[4], float4 (&acc)[4]) {
  static_assert(K % UNROLL == 0 && UNROLL % 4 == 0, "whole groups of four inputs");
  const float4 b = *reinterpret_cast<const float4*>(bias);
#pragma unroll
  for (int e = 0; e < 4; e++) acc[e] = b;
#pragma unroll 1
  for (int k0 = 0; k0 < K; k0 += UNROLL) {
    float4 w[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) w[u] = *reinterpret_cast<const float4*>(W + (size_t)(k0 + u) * HID);
#pragma unroll
    for (int u = 0; u < UNROLL; u += 4) {
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const float4 x = *reinterpret_cast<const float4*>(in[e] + k0 + u);
        acc[e].x = add_group(acc[e].x, dot4_launch(x, w[u].x, w[u + 1].x, w[u + 2].x, w[u + 3].x));
        acc[e].y = add_group(acc[e].y, dot4_launch(x, w[u].y, w[u + 1].y, w[u + 2].y, w[u + 3].y));
        acc[e].z = add_group(acc[e].z, dot4_launch(x, w[u].z, w[u + 1].z, w[u + 2].z, w[u + 3].z));
        acc[e].w = add_group(acc[e].w, dot4_launch(x, w[u].w, w[u + 1].w, w[u + 2].w, w[u + 3].w));
      }
    }
  }
}

// arguments as policy_wave4's (scratch blocks of >= 464 floats, 16-byte aligned: z[64] | h1[200] | h2[200])
template <class T>
__device__ inline void policy_wave4_launch_order(const PolicyArgs& pa, const int (&env)[4], const bool (&write)[4], int lane, char* slot0, unsigned stride, unsigned off_q, unsigned off_v,
                                                 unsigned off_scr) {
  const float* __restrict__ P = pa.P;
  const T* ob_q[4]; const T* ob_v[4]; float* scr[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    ob_q[e] = reinterpret_cast<const T*>(slot0 + e * stride + off_q); ob_v[e] = reinterpret_cast<const T*>(slot0 + e * stride + off_v);
    scr[e] = reinterpret_cast<float*>(slot0 + e * stride + off_scr);
  }
  {
    const int slot = lane >> 4, sl = lane & 15;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int i = sl + 16 * c;
      if (i < OB) {
        const float o = i < 28 ? (float)ob_q[slot][i] : (float)ob_v[slot][i - 28];
        float v = (o - P[O_MEAN + i]) / P[O_STD + i]; v = fminf(fmaxf(v, -5.0f), 5.0f);
        scr[slot][i] = v;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
  const bool hid = lane < 2 * (HID / 4);
  const int net = lane >= HID / 4 ? 1 : 0, j4 = 4 * (lane - net * (HID / 4));
  const int jj = hid ? j4 : 0;
  {
    const float* in[4] = {scr[0], scr[1], scr[2], scr[3]};
    float4 a[4];
    dense4_wave4_by4<OB, 8>(P + (net ? O_VW1 : O_PW1) + jj, P + (net ? O_VB1 : O_PB1) + jj, in, a);
    if (hid) {
#pragma unroll
      for (int e = 0; e < 4; e++) *reinterpret_cast<float4*>(scr[e] + 64 + net * HID + j4) = make_float4(tanhf(a[e].x), tanhf(a[e].y), tanhf(a[e].z), tanhf(a[e].w));
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
  {
    const float* in[4] = {scr[0] + 64 + net * HID, scr[1] + 64 + net * HID, scr[2] + 64 + net * HID, scr[3] + 64 + net * HID};
    float4 a[4];
    dense4_wave4_by4<HID, 20>(P + (net ? O_VW2 : O_PW2) + jj, P + (net ? O_VB2 : O_PB2) + jj, in, a);
    if (hid) {
#pragma unroll
      for (int e = 0; e < 4; e++) *reinterpret_cast<float4*>(scr[e] + 264 + net * HID + j4) = make_float4(tanhf(a[e].x), tanhf(a[e].y), tanhf(a[e].z), tanhf(a[e].w));
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier();
  {
    const bool isv = lane == AC, on = lane <= AC;
    const float* W = P + (isv ? O_VW3 : O_PW3);
    const int ws = isv ? 1 : AC, wo = (isv || !on) ? 0 : lane;
    const int ho = 264 + (isv ? HID : 0);
#pragma unroll 1
    for (int e = 0; e < 4; e++) {
      const float* h = scr[e] + ho;
      float s = isv ? P[O_VB3] : P[O_PB3 + wo];
      for (int k = 0; k < HID; k += 4) {
        const float4 x = *reinterpret_cast<const float4*>(h + k);
        s = add_group(s, dot4_launch(x, W[(k + 0) * ws + wo], W[(k + 1) * ws + wo], W[(k + 2) * ws + wo], W[(k + 3) * ws + wo]));
      }
      if (!write[e]) continue;
      if (isv) pa.vpred[env[e]] = s;
      else if (on) {
        if (pa.stochastic) s = __builtin_fmaf(expf(P[O_LOGSTD + lane]), normal_from(pa.seed, pa.counter, (unsigned)(env[e] * AC + lane)), s);      // (fused in the launch)
        pa.action[(size_t)env[e] * AC + lane] = (double)s;
      }
    }
  }
}

}  // namespace dmp
