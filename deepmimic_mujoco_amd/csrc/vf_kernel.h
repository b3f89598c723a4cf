// vf_kernel.h — the value fit of the TRPO learner (src/trpo.py:288-296) as three kernels per minibatch instead of ~60 library
// launches.  One minibatch step of the reference is
//     pi.ob_rms.update(mbob);  g = grad of mean((vpred(mbob) - mbret)^2) w.r.t. the value net;  vfadam.update(g, vf_stepsize)
// with the 56-100-100-1 tanh value net of src/mlp_policy_trpo.py:43-48, the obs filter of src/utils/misc_util.py:32-70 and the
// MpiAdam rule of src/mpi_adam.py:21-35.  Here:
//   k_vf_rms   column sums / sums of squares of the minibatch in float64 (fixed reduction order), the LAST block to finish adds
//              them to the filter's state and refreshes its float32 mean / std,
//   k_vf_grad  a block takes 32 samples: normalise + clip, forward, backward as fp32 MFMA tiles out of LDS (theta staged once per block), and
//              writes its partial gradient of the 15 901 parameters,
//   k_vf_adam  partial gradients summed in a fixed order (four quarters of the blocks, each in block order), Adam moments, step.
// fp32 like the reference's TF graph (sums of the filter in float64 like its numpy arrays).  A whole epoch of minibatches is
// enqueued by one C call (dm_vf_fit_epoch); nothing comes back to the host.  There the filter sums of all minibatches are taken up front
// (k_vf_rms_part / k_vf_rms_scan below): two launches per minibatch remain.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mlp_tile.h"

namespace dmv {
using namespace dml;

constexpr int OB = 56;                              // k_vf_grad takes SB = 32 samples per block (a 4 096-sample minibatch is 128 blocks: the policy step can have the other CUs)
using VfShared = MlpShared<OB>;
constexpr int NP = VfShared::NP, NPAD = VfShared::NPAD;
constexpr int RMS_BLOCKS = 64;

// ---- obs filter ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vf_rms(const float* __restrict__ ob, int bs, double* __restrict__ part /*[RMS_BLOCKS][2*OB]*/,
                                                unsigned* __restrict__ ticket, double* __restrict__ sum, double* __restrict__ sumsq,
                                                double* __restrict__ count, float* __restrict__ mean, float* __restrict__ stdv) {
  __shared__ double red[4][2 * OB];
  __shared__ bool last;
  const int tid = threadIdx.x, col = tid % OB, rg = tid / OB;            // 224 working threads: 4 row groups x 56 columns
  const int rows = (bs + (int)gridDim.x - 1) / (int)gridDim.x, r0 = blockIdx.x * rows, r1 = min(bs, r0 + rows);
  if (rg < 4) {
    double s = 0.0, q = 0.0;
    int r = r0 + rg;
    for (; r + 12 < r1; r += 16) {                   // four rows of this row group in flight
      const float x0 = ob[(size_t)r * OB + col], x1 = ob[(size_t)(r + 4) * OB + col], x2 = ob[(size_t)(r + 8) * OB + col], x3 = ob[(size_t)(r + 12) * OB + col];
      s += (double)x0; q += (double)x0 * (double)x0; s += (double)x1; q += (double)x1 * (double)x1;
      s += (double)x2; q += (double)x2 * (double)x2; s += (double)x3; q += (double)x3 * (double)x3;
    }
    for (; r < r1; r += 4) { const double x = (double)ob[(size_t)r * OB + col]; s += x; q += x * x; }
    red[rg][col] = s; red[rg][OB + col] = q;
  }
  __syncthreads();
  if (tid < 2 * OB) part[blockIdx.x * 2 * OB + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  __threadfence();
  __syncthreads();
  if (tid == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();
  if (tid < 2 * OB) {
    double a = 0.0;
    for (int b = 0; b < (int)gridDim.x; b += 8) {                               // fixed order: results do not depend on block timing
      double x[8];
#pragma unroll
      for (int u = 0; u < 8; u++) x[u] = b + u < (int)gridDim.x ? part[(b + u) * 2 * OB + tid] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; u++) a += x[u];
    }
    if (tid < OB) sum[tid] += a; else sumsq[tid - OB] += a;
  }
  __syncthreads();
  if (tid == 0) { *count += (double)bs; *ticket = 0u; }
  __syncthreads();
  if (tid < OB) {                                                               // RunningMeanStd._refresh (policy.py)
    const double c = *count;
    const float m = (float)(sum[tid] / c);
    const float var = (float)(sumsq[tid] / c) - m * m;
    mean[tid] = m; stdv[tid] = sqrtf(fmaxf(var, 1e-2f));
  }
}

// ---- forward + backward of 32 samples ------------------------------------------------------------------------------------------
// The tile layout of mlp_tile.h, on 128 blocks of a 4 096-sample minibatch.  (Rounds 2-3: 4 x 4 / 2 x 4 register tiles of FMAs on 16-sample
// blocks, 28 us per 4 096-sample minibatch.)
static_assert(SB * OB % 256 == 0, "the observation tile is read in whole rounds of the block");

// forward + backward of samples s0 .. s0 + SB - 1 of the minibatch; the tile's partial gradient goes to `out` (NPAD floats, theta order)
__global__ __launch_bounds__(256) void k_vf_grad(const float* __restrict__ ob, const float* __restrict__ ret, int bs, const float* __restrict__ theta,
                                                 const float* __restrict__ mean, const float* __restrict__ stdv, float* __restrict__ partial) {
  __shared__ VfShared S;                                      // 126 KB: one block per CU
  const int tid = threadIdx.x, s0 = blockIdx.x * SB;
  // One round trip for everything the block reads: the tile's observations (with the filter's mean / std) are requested here, theta right
  // after them by mlp_stage, and the pads are zeroed while they are in flight.
  constexpr int NZ = SB * OB / 256;
  float x[NZ], mu[NZ], sd[NZ];
#pragma unroll
  for (int j = 0; j < NZ; j++) {
    const int i = tid + 256 * j, sm = i / OB, k = i % OB, r = s0 + sm;
    x[j] = r < bs ? ob[(size_t)r * OB + k] : 0.0f; mu[j] = mean[k]; sd[j] = stdv[k];
  }
  mlp_stage(S, theta, [&] {
#pragma unroll
    for (int j = 0; j < NZ; j++) {                            // coalesced read of [sample][input], transposed store
      const int i = tid + 256 * j, sm = i / OB, k = i % OB;
      S.z[k][sm] = (s0 + sm < bs) ? fminf(fmaxf((x[j] - mu[j]) / sd[j], -5.0f), 5.0f) : 0.0f;
    }
  });
  // error, d loss / d vpred  (loss = mean over the minibatch of (vpred - ret)^2)
  mlp_forward(S, [&](int sm, float v) { S.dy[sm] = (s0 + sm < bs) ? 2.0f * (v - ret[s0 + sm]) / (float)bs : 0.0f; });
  mlp_backward(S, partial + (size_t)blockIdx.x * NPAD);
}

// ---- PPO's value half: k_vf_grad on rows gathered by idx, with the loss -------------------------------------------------------------
// loss = mean over the n rows of (vpred - ret)^2 (ppo1's vf_loss); rows idx[0 .. n) of ob_all / ret_all (null idx: rows 0 .. n - 1).
// lpart[blockIdx.x] = the block's sum of squared errors, in float64 (a butterfly over each tile's 32 samples).  GRAD: one tile per block
// (grid = the tiles), its partial gradient to partial + blockIdx.x * NPAD as k_vf_grad writes it; !GRAD: any grid, a block walks the tiles
// blockIdx.x, + gridDim.x, ... and writes the loss alone.
template <bool GRAD>
__global__ __launch_bounds__(256) void k_vf_grad_rows(const float* __restrict__ ob_all, const float* __restrict__ ret_all, const int* __restrict__ idx,
                                                      int n, const float* __restrict__ theta, const float* __restrict__ mean, const float* __restrict__ stdv,
                                                      float* __restrict__ partial, double* __restrict__ lpart) {
  __shared__ VfShared S;
  const int tid = threadIdx.x, ntiles = (n + SB - 1) / SB;
  constexpr int NZ = SB * OB / 256;
  double lsum = 0.0;
  auto run_tile = [&](int tile) {
    const int s0 = tile * SB;
    float x[NZ], mu[NZ], sd[NZ];
#pragma unroll
    for (int j = 0; j < NZ; j++) {
      const int i = tid + 256 * j, sm = i / OB, k = i % OB, r = s0 + sm;
      x[j] = r < n ? ob_all[(size_t)(idx ? idx[r] : r) * OB + k] : 0.0f; mu[j] = mean[k]; sd[j] = stdv[k];
    }
    mlp_stage(S, theta, [&] {
#pragma unroll
      for (int j = 0; j < NZ; j++) {
        const int i = tid + 256 * j, sm = i / OB, k = i % OB;
        S.z[k][sm] = (s0 + sm < n) ? fminf(fmaxf((x[j] - mu[j]) / sd[j], -5.0f), 5.0f) : 0.0f;
      }
    });
    mlp_forward(S, [&](int sm, float v) {                     // threads 0 .. 31: one sample each
      const int r = s0 + sm;
      const float e = r < n ? v - ret_all[idx ? idx[r] : r] : 0.0f;
      S.dy[sm] = 2.0f * e / (float)n;
      double q = (double)e * (double)e;
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) q += __shfl_xor(q, o, 32);
      lsum += q;
    });
  };
  if constexpr (GRAD) {
    run_tile(blockIdx.x);
    mlp_backward(S, partial + (size_t)blockIdx.x * NPAD);
  } else {
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      run_tile(tile);
      __syncthreads();                                        // this tile's readers are done before the next one zeroes the pads
    }
  }
  if (tid == 0) lpart[blockIdx.x] = lsum;
}

// ---- gradient reduction + MpiAdam step (src/mpi_adam.py:21-35): the summation tree of quarter_sum (mlp_tile.h) ---------------------
constexpr int ADAM_PARAMS = QCOLS;
__global__ __launch_bounds__(256) void k_vf_adam(const float* __restrict__ partial, int nblk, float* __restrict__ theta, float* __restrict__ m,
                                                 float* __restrict__ v, float a, float beta1, float beta2, float eps) {
  const int p = blockIdx.x * ADAM_PARAMS + threadIdx.x % ADAM_PARAMS;
  const float g = quarter_sum<NP, NPAD>(partial, nblk);
  if (threadIdx.x >= ADAM_PARAMS || p >= NP) return;
  const float mm = beta1 * m[p] + (1.0f - beta1) * g;
  const float vv = beta2 * v[p] + (1.0f - beta2) * g * g;
  m[p] = mm; v[p] = vv;
  theta[p] += (-a) * mm / (sqrtf(vv) + eps);
}

// ---- the obs filter's statistics for a whole epoch up front -------------------------------------------------------------------
// k_vf_rms is a third of a minibatch's time (rocprofv3: 12.9 of 57 us at 4 096 samples) and does not depend on the parameters:
//   k_vf_rms_part   the column sums / sums of squares of EVERY minibatch of the epoch at once (grid RMS_BLOCKS x nb; the same partial sums,
//                   in the same order, as k_vf_rms computes for one),
//   k_vf_rms_scan   one block: minibatch after minibatch it adds the partials (block order) to the filter's state and records the
//                   float32 mean / std the filter holds AFTER that minibatch — what that minibatch's gradient step normalises with.
// Same arithmetic in the same order as a k_vf_rms per minibatch: bit-identical filter state and parameters (tests/test_trpo.py).
// (Measured dead end, round 3: the whole epoch as ONE launch — resident blocks walking the minibatches with a grid barrier between the
//  gradient and the Adam step, exchanged data through device-scope accesses — 67 us per minibatch against 44 us for the two launches: a
//  barrier across 128 CUs on eight XCDs costs more than a kernel boundary here.)
__global__ __launch_bounds__(256) void k_vf_rms_part(const float* __restrict__ ob_all, int bs, double* __restrict__ part_all /*[nb][RMS_BLOCKS][2*OB]*/) {
  __shared__ double red[4][2 * OB];
  const float* ob = ob_all + (size_t)blockIdx.y * bs * OB;
  double* part = part_all + (size_t)blockIdx.y * RMS_BLOCKS * 2 * OB;
  const int tid = threadIdx.x, col = tid % OB, rg = tid / OB;
  const int rows = (bs + RMS_BLOCKS - 1) / RMS_BLOCKS, r0 = blockIdx.x * rows, r1 = min(bs, r0 + rows);
  if (rg < 4) {
    double s = 0.0, q = 0.0;
    int r = r0 + rg;
    for (; r + 12 < r1; r += 16) {
      const float x0 = ob[(size_t)r * OB + col], x1 = ob[(size_t)(r + 4) * OB + col], x2 = ob[(size_t)(r + 8) * OB + col], x3 = ob[(size_t)(r + 12) * OB + col];
      s += (double)x0; q += (double)x0 * (double)x0; s += (double)x1; q += (double)x1 * (double)x1;
      s += (double)x2; q += (double)x2 * (double)x2; s += (double)x3; q += (double)x3 * (double)x3;
    }
    for (; r < r1; r += 4) { const double x = (double)ob[(size_t)r * OB + col]; s += x; q += x * x; }
    red[rg][col] = s; red[rg][OB + col] = q;
  }
  __syncthreads();
  if (tid < 2 * OB) part[blockIdx.x * 2 * OB + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}
// Two launches: k_vf_rms_fold adds every (minibatch, column) pair's 64 partials up in block order, one block per minibatch (the sums replace the
// first partial in place); k_vf_rms_scan is one wave of 56 threads that walks the minibatches, each carrying its column's sum AND sum of squares:
// no exchange between threads, eight minibatches' sums in flight.  (Round 3's form added each minibatch's partials inside the walk, two block
// barriers per minibatch: 193 us per epoch of 128 minibatches on the fit's critical path; folding inside the scan's own block — one CU pulling
// 7 MB through its L2 port — still 123 us.)
__global__ __launch_bounds__(128) void k_vf_rms_fold(double* __restrict__ part_all) {
  const int c = threadIdx.x;
  if (c >= 2 * OB) return;
  double* part = part_all + (size_t)blockIdx.x * RMS_BLOCKS * 2 * OB;
  double a = 0.0;
  for (int b = 0; b < RMS_BLOCKS; b += 8) {
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; u++) x[u] = part[(b + u) * 2 * OB + c];
#pragma unroll
    for (int u = 0; u < 8; u++) a += x[u];
  }
  part[c] = a;                                                                  // (this thread is the only reader of column c of this minibatch)
}
__global__ __launch_bounds__(64) void k_vf_rms_scan(const double* __restrict__ part_all, int nb, int bs, double* __restrict__ sum, double* __restrict__ sumsq,
                                                    double* __restrict__ count, float* __restrict__ mean, float* __restrict__ stdv,
                                                    float* __restrict__ means /*[nb][OB]*/, float* __restrict__ stds /*[nb][OB]*/) {
  const int tid = threadIdx.x;
  if (tid >= OB) return;
  double s = sum[tid], q = sumsq[tid], c = *count;
  float m = 0.0f, sd = 1.0f;
  for (int i0 = 0; i0 < nb; i0 += 8) {
    double as[8], aq[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = i0 + u < nb ? i0 + u : nb - 1;
      as[u] = part_all[(size_t)i * RMS_BLOCKS * 2 * OB + tid]; aq[u] = part_all[(size_t)i * RMS_BLOCKS * 2 * OB + OB + tid];
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = i0 + u;
      if (i >= nb) break;
      s += as[u]; q += aq[u]; c += (double)bs;
      m = (float)(s / c);                                                       // RunningMeanStd._refresh (policy.py)
      const float var = (float)(q / c) - m * m;
      sd = sqrtf(fmaxf(var, 1e-2f));
      means[(size_t)i * OB + tid] = m; stds[(size_t)i * OB + tid] = sd;
    }
  }
  sum[tid] = s; sumsq[tid] = q; mean[tid] = m; stdv[tid] = sd;
  if (tid == 0) *count = c;
}
}  // namespace dmv
