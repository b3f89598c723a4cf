// disc_kernel.h — the GAIL discriminator (src/adversary.py TransitionClassifier) on the matrix cores.  D(ob, ac) is
//     logit = fc(100 -> 1)( tanh fc(100 -> 100)( tanh fc(84 -> 100)( concat((ob - rms.mean) / rms.std, ac) ) ) )
// in fp32 like the reference's TF graph (no clip of the normalised observation, unlike the policy's +-5).  Three kernels:
//   k_disc_reward  forward pass of a block of 32 rows of a segment's float64 (ob, ac) and the policy's reward
//                  -log(1 - sigmoid(logit) + 1e-8), written literally in fp32 (adversary.py `reward_op`: it saturates at
//                  -log(1e-8) once sigmoid rounds to 1), stored as float64 for dm_episode_scan,
//   k_disc_grad    forward + backward of 32 generator OR expert rows (block b < nbg: generator rows 32 b .., else expert rows): the
//                  block's partial gradient of the total loss (adversary.py `total_loss`) and its partial loss sums,
//   k_disc_reduce  the partials summed in a fixed order (four quarters of the blocks, each in block order) into the flat gradient, and
//                  the six reported values (adversary.py `loss_name`) from the loss sums (fixed strides, then thread order): bitwise reproducible.
// Flat parameter order = adversary/fully_connected{,_1,_2}/{weights,biases}: W1 [84][100], b1, W2 [100][100], b2, w3 [100], b3.  The tile
// layout and the forward / backward passes are mlp_tile.h's, shared with the value fit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mlp_tile.h"

namespace dmd {
using namespace dml;

constexpr int OBD = 56, ACD = 28, IN = OBD + ACD;
using DiscShared = MlpShared<IN>;
constexpr int NP = DiscShared::NP, NPAD = DiscShared::NPAD;
constexpr int L_CE = NP, L_ENT = NP + 1, L_ACC = NP + 2;            // per-block loss sums, in the pad of a partial gradient row
static_assert(L_ACC < NPAD, "the loss sums live in the pad of a partial row");
__device__ inline float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// Stage theta and the block's rows s0 .. s0 + SB - 1 of (ob, ac) (row count n; rows past it are zero) into LDS, then the forward pass: h1, h2
// and each sample's logit in S.dy.
template <typename T>
__device__ inline void disc_forward(DiscShared& S, const T* __restrict__ ob, const T* __restrict__ ac, int s0, int n, const float* __restrict__ theta,
                                    const float* __restrict__ mean, const float* __restrict__ stdv) {
  const int tid = threadIdx.x;
  mlp_stage(S, theta, [&] {
    for (int i = tid; i < SB * OBD; i += 256) {               // coalesced reads of [sample][input], transposed stores
      const int sm = i / OBD, k = i % OBD, r = s0 + sm;
      if (r < n) S.z[k][sm] = ((float)ob[(size_t)r * OBD + k] - mean[k]) / stdv[k];
    }
    for (int i = tid; i < SB * ACD; i += 256) {
      const int sm = i / ACD, k = i % ACD, r = s0 + sm;
      if (r < n) S.z[OBD + k][sm] = (float)ac[(size_t)r * ACD + k];
    }
  });
  mlp_forward(S, [&](int sm, float x) { S.dy[sm] = x; });
}

// reward of rows 32 b .. 32 b + 31 of n: ob [n, 56], ac [n, 28] float64 (the rollout's buffers), reward [n] float64
__global__ __launch_bounds__(256) void k_disc_reward(const double* __restrict__ ob, const double* __restrict__ ac, int n, const float* __restrict__ theta,
                                                     const float* __restrict__ mean, const float* __restrict__ stdv, double* __restrict__ reward) {
  __shared__ DiscShared S;
  const int s0 = blockIdx.x * SB;
  disc_forward<double>(S, ob, ac, s0, n, theta, mean, stdv);
  const int tid = threadIdx.x;
  if (tid < SB && s0 + tid < n) {
    const float s = sigmoidf(S.dy[tid]);
    reward[s0 + tid] = (double)(-logf((1.0f - s) + 1e-8f));
  }
}

// forward + backward of one block of generator rows (blockIdx.x < nbg) or expert rows; partial gradient + loss sums -> partial[b] (NPAD floats)
__global__ __launch_bounds__(256) void k_disc_grad(const float* __restrict__ g_ob, const float* __restrict__ g_ac, int ng, const float* __restrict__ e_ob,
                                                   const float* __restrict__ e_ac, int ne, int nbg, const float* __restrict__ theta,
                                                   const float* __restrict__ mean, const float* __restrict__ stdv, float entcoeff, float* __restrict__ partial) {
  __shared__ DiscShared S;
  __shared__ float lce[SB], lent[SB], lacc[SB];
  const int tid = threadIdx.x;
  const bool expert = (int)blockIdx.x >= nbg;
  const int s0 = (expert ? (int)blockIdx.x - nbg : (int)blockIdx.x) * SB, n = expert ? ne : ng;
  float* out = partial + (size_t)blockIdx.x * NPAD;
  disc_forward<float>(S, expert ? e_ob : g_ob, expert ? e_ac : g_ac, s0, n, theta, mean, stdv);
  if (tid < SB) {                                             // d total / d logit, and the sample's loss terms
    const float x = S.dy[tid], s = sigmoidf(x);
    const bool valid = s0 + tid < n;
    const float sp = log1pf(expf(-fabsf(x)));                 // TF sigmoid_cross_entropy_with_logits: max(x, 0) - x z + log1p(exp(-|x|))
    const float ce = fmaxf(x, 0.0f) - (expert ? x : 0.0f) + sp;
    const float ent = (1.0f - s) * x + (sp + fmaxf(-x, 0.0f)); // logit_bernoulli_entropy: (1 - sigmoid) x + softplus(-x)
    const float d = (expert ? (s - 1.0f) / (float)ne : s / (float)ng) + entcoeff * s * (1.0f - s) * x / (float)(ng + ne);
    S.dy[tid] = valid ? d : 0.0f;
    lce[tid] = valid ? ce : 0.0f; lent[tid] = valid ? ent : 0.0f;
    lacc[tid] = valid && (expert ? s > 0.5f : s < 0.5f) ? 1.0f : 0.0f;
  }
  __syncthreads();
  mlp_backward(S, out);
  // the block's loss sums (sample order)
  if (tid == H + 1) { float a = 0.0f, b = 0.0f, c = 0.0f; for (int sm = 0; sm < SB; sm++) { a += lce[sm]; b += lent[sm]; c += lacc[sm]; } out[L_CE] = a; out[L_ENT] = b; out[L_ACC] = c; }
}

// The gradient: the summation tree of quarter_sum (mlp_tile.h).  One more block (the last) adds the loss sums up: thread t takes blocks t,
// t + 256, ... in order (float64), the 256 sums are added in thread order, and thread 0 writes the six reported values: generator_loss,
// expert_loss, entropy, entropy_loss, generator_acc, expert_acc.  (A lone thread walking 32 768 blocks' sums took 6 ms at 4 096 x 128 rows.)
constexpr int RED_BLOCKS = (NP + QCOLS - 1) / QCOLS;                      // launch RED_BLOCKS + 1 blocks
__global__ __launch_bounds__(256) void k_disc_reduce(const float* __restrict__ partial, int nblk, int nbg, int ng, int ne, float entcoeff,
                                                     float* __restrict__ grad, double* __restrict__ losses) {
  if ((int)blockIdx.x == RED_BLOCKS) {
    __shared__ double ls[5][256];
    const int t = threadIdx.x;
    double ce_g = 0.0, ce_e = 0.0, ent = 0.0, acc_g = 0.0, acc_e = 0.0;
    for (int b = t; b < nblk; b += 256) {
      const float* q = partial + (size_t)b * NPAD;
      if (b < nbg) { ce_g += (double)q[L_CE]; acc_g += (double)q[L_ACC]; } else { ce_e += (double)q[L_CE]; acc_e += (double)q[L_ACC]; }
      ent += (double)q[L_ENT];
    }
    ls[0][t] = ce_g; ls[1][t] = ce_e; ls[2][t] = ent; ls[3][t] = acc_g; ls[4][t] = acc_e;
    __syncthreads();
    if (t < 5) { double a = 0.0; for (int i = 0; i < 256; i++) a += ls[t][i]; ls[t][0] = a; }
    __syncthreads();
    if (t == 0) {
      const double e = ls[2][0] / (double)(ng + ne);
      losses[0] = ls[0][0] / ng; losses[1] = ls[1][0] / ne; losses[2] = e; losses[3] = -(double)entcoeff * e; losses[4] = ls[3][0] / ng; losses[5] = ls[4][0] / ne;
    }
    return;
  }
  const int p = blockIdx.x * QCOLS + threadIdx.x % QCOLS;
  const float g = quarter_sum<NP, NPAD>(partial, nblk);
  if (threadIdx.x < QCOLS && p < NP) grad[p] = g;
}
}  // namespace dmd
