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
// Flat parameter order = adversary/fully_connected{,_1,_2}/{weights,biases}: W1 [84][100], b1, W2 [100][100], b2, w3 [100], b3.
// The tile layout is the value fit's (vf_kernel.h): activations transposed in LDS ([unit][sample], row stride 33), ONE copy of theta in
// LDS in which each bias is the row after its matrix, so a constant row of ones under the input / h1 folds the biases into the products.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dmd {

constexpr int OBD = 56, ACD = 28, IN = OBD + ACD, H = 100, SB = 32;
constexpr int O_W1 = 0, O_B1 = O_W1 + IN * H, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + H, NP = O_B3 + 1;
constexpr int NPAD = (NP + 63) / 64 * 64;
constexpr int L_CE = NP, L_ENT = NP + 1, L_ACC = NP + 2;            // per-block loss sums, in the pad of a partial gradient row
static_assert(L_ACC < NPAD, "the loss sums live in the pad of a partial row");
constexpr int SBP = SB + 1, ZR = IN + 2, HR = H + 4;
constexpr int NWT = (NP + 3) / 4 * 4;
typedef float v16f __attribute__((ext_vector_type(16)));
struct alignas(16) DiscShared {
  float Wt[NWT];                                      // theta
  float z[ZR][SBP];                                   // input rows 0..83, row 84 = 1, row 85 = 0
  float h1[HR][SBP], h2[HR][SBP];                     // h1: row 100 = 1, row 101 = 0
  float d2[HR][SBP], d1[HR][SBP];                     // (as operands of the weight-gradient products their 128-row tiles read on into what follows)
  float xpart[8][SB], dx[SB];
  float tail[24 * SBP];                               // ... zeros
};
static_assert(sizeof(DiscShared) <= 160 * 1024, "DiscShared must fit a CU's LDS");
static_assert(O_W2 + 127 * H + H <= NWT + ZR * SBP, "padded W2 rows (A operand of the backward product) read into z");
static_assert(O_W2 + 101 * H + 128 <= NWT + ZR * SBP, "padded W2 columns of the forward product read into z");
static_assert(3 * 32 <= ZR + HR, "the third input tile of dW1 reads into h1");
static_assert(sizeof(DiscShared::xpart) + sizeof(DiscShared::dx) + sizeof(DiscShared::tail) >= 24 * SBP * sizeof(float), "d1's 128-row tile reads past it");
__device__ inline v16f mfma32(float a, float b, v16f c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
__device__ inline int row32(int r, int hf) { return 8 * (r / 4) + 4 * hf + (r % 4); }
__device__ inline float fast_tanh(float x) {                      // (vf_kernel.h: absolute error ~1e-7)
  const float t = __expf(-2.0f * fabsf(x));
  return copysignf((1.0f - t) * __frcp_rn(1.0f + t), x);
}
__device__ inline float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// Stage theta and the block's rows s0 .. s0 + SB - 1 of (ob, ac) (row count n; rows past it are zero) into LDS, zero every pad,
// then the forward pass: h1, h2 and each sample's logit in S.dx.  Caller: 256 threads.
template <typename T>
__device__ inline void disc_forward(DiscShared& S, const T* __restrict__ ob, const T* __restrict__ ac, int s0, int n, const float* __restrict__ theta,
                                    const float* __restrict__ mean, const float* __restrict__ stdv) {
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, li = l & 31, hf = l >> 5, u0 = 32 * w;
  {
    constexpr int NT = (NP / 4 + 255) / 256;
    const float4* g = reinterpret_cast<const float4*>(theta);
    float4 th[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) { const int i = tid + 256 * j; th[j] = i < NP / 4 ? g[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    const float last = tid < NWT - NP / 4 * 4 && NP / 4 * 4 + tid < NP ? theta[NP / 4 * 4 + tid] : 0.0f;
    float4* act = reinterpret_cast<float4*>(&S.z[0][0]);
    for (int i = tid; i < (int)((sizeof(DiscShared) - sizeof(S.Wt)) / 16); i += 256) act[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    __syncthreads();
    float4* d = reinterpret_cast<float4*>(S.Wt);
#pragma unroll
    for (int j = 0; j < NT; j++) { const int i = tid + 256 * j; if (i < NP / 4) d[i] = th[j]; }
    if (tid < NWT - NP / 4 * 4) S.Wt[NP / 4 * 4 + tid] = last;
    if (tid < SB) { S.z[IN][tid] = 1.0f; S.h1[H][tid] = 1.0f; }
    for (int i = tid; i < SB * OBD; i += 256) {               // coalesced reads of [sample][input], transposed stores
      const int sm = i / OBD, k = i % OBD, r = s0 + sm;
      if (r < n) S.z[k][sm] = ((float)ob[(size_t)r * OBD + k] - mean[k]) / stdv[k];
    }
    for (int i = tid; i < SB * ACD; i += 256) {
      const int sm = i / ACD, k = i % ACD, r = s0 + sm;
      if (r < n) S.z[OBD + k][sm] = (float)ac[(size_t)r * ACD + k];
    }
  }
  __syncthreads();
  {   // layer 1: h1 = tanh(W1ext^T zext)
    v16f acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
    for (int t = 0; t < ZR / 2; t++) { const int k = 2 * t + hf; acc = mfma32(S.Wt[O_W1 + k * H + u0 + li], S.z[k][li], acc); }
#pragma unroll
    for (int r = 0; r < 16; r++) { const int u = u0 + row32(r, hf); if (u < H) S.h1[u][li] = fast_tanh(acc[r]); }
  }
  __syncthreads();
  {   // layer 2
    v16f acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
    for (int t = 0; t < (H + 2) / 2; t++) { const int k = 2 * t + hf; acc = mfma32(S.Wt[O_W2 + k * H + u0 + li], S.h1[k][li], acc); }
#pragma unroll
    for (int r = 0; r < 16; r++) { const int u = u0 + row32(r, hf); if (u < H) S.h2[u][li] = fast_tanh(acc[r]); }
  }
  __syncthreads();
  {   // logit = w3 . h2 + b3, eight partial sums per sample added in a fixed order
    const int sm = tid % SB, part = tid / SB;
    float v = 0.0f;
    for (int j = part; j < H; j += 8) v += S.h2[j][sm] * S.Wt[O_W3 + j];
    S.xpart[part][sm] = v;
  }
  __syncthreads();
  if (tid < SB) {
    float v = S.Wt[O_B3];
#pragma unroll
    for (int p = 0; p < 8; p++) v += S.xpart[p][tid];
    S.dx[tid] = v;
  }
  __syncthreads();
}

// reward of rows 32 b .. 32 b + 31 of n: ob [n, 56], ac [n, 28] float64 (the rollout's buffers), reward [n] float64
__global__ __launch_bounds__(256) void k_disc_reward(const double* __restrict__ ob, const double* __restrict__ ac, int n, const float* __restrict__ theta,
                                                     const float* __restrict__ mean, const float* __restrict__ stdv, double* __restrict__ reward) {
  __shared__ DiscShared S;
  const int s0 = blockIdx.x * SB;
  disc_forward<double>(S, ob, ac, s0, n, theta, mean, stdv);
  const int tid = threadIdx.x;
  if (tid < SB && s0 + tid < n) {
    const float s = sigmoidf(S.dx[tid]);
    reward[s0 + tid] = (double)(-logf((1.0f - s) + 1e-8f));
  }
}

// forward + backward of one block of generator rows (blockIdx.x < nbg) or expert rows; partial gradient + loss sums -> partial[b] (NPAD floats)
__global__ __launch_bounds__(256) void k_disc_grad(const float* __restrict__ g_ob, const float* __restrict__ g_ac, int ng, const float* __restrict__ e_ob,
                                                   const float* __restrict__ e_ac, int ne, int nbg, const float* __restrict__ theta,
                                                   const float* __restrict__ mean, const float* __restrict__ stdv, float entcoeff, float* __restrict__ partial) {
  __shared__ DiscShared S;
  __shared__ float lce[SB], lent[SB], lacc[SB];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, li = l & 31, hf = l >> 5, u0 = 32 * w;
  const bool expert = (int)blockIdx.x >= nbg;
  const int s0 = (expert ? (int)blockIdx.x - nbg : (int)blockIdx.x) * SB, n = expert ? ne : ng;
  float* out = partial + (size_t)blockIdx.x * NPAD;
  disc_forward<float>(S, expert ? e_ob : g_ob, expert ? e_ac : g_ac, s0, n, theta, mean, stdv);
  if (tid < SB) {                                             // d total / d logit, and the sample's loss terms
    const float x = S.dx[tid], s = sigmoidf(x);
    const bool valid = s0 + tid < n;
    const float sp = log1pf(expf(-fabsf(x)));                 // TF sigmoid_cross_entropy_with_logits: max(x, 0) - x z + log1p(exp(-|x|))
    const float ce = fmaxf(x, 0.0f) - (expert ? x : 0.0f) + sp;
    const float ent = (1.0f - s) * x + (sp + fmaxf(-x, 0.0f)); // logit_bernoulli_entropy: (1 - sigmoid) x + softplus(-x)
    const float d = (expert ? (s - 1.0f) / (float)ne : s / (float)ng) + entcoeff * s * (1.0f - s) * x / (float)(ng + ne);
    S.dx[tid] = valid ? d : 0.0f;
    lce[tid] = valid ? ce : 0.0f; lent[tid] = valid ? ent : 0.0f;
    lacc[tid] = valid && (expert ? s > 0.5f : s < 0.5f) ? 1.0f : 0.0f;
  }
  __syncthreads();
  // delta2 = dx w3 (1 - h2^2);  dw3, db3; the block's loss sums (sample order)
  for (int i = tid; i < SB * H; i += 256) { const int j = i / SB, sm = i % SB; const float h = S.h2[j][sm]; S.d2[j][sm] = S.dx[sm] * S.Wt[O_W3 + j] * (1.0f - h * h); }
  if (tid < H) { float a = 0.0f; for (int sm = 0; sm < SB; sm++) a += S.h2[tid][sm] * S.dx[sm]; out[O_W3 + tid] = a; }
  if (tid == H) { float a = 0.0f; for (int sm = 0; sm < SB; sm++) a += S.dx[sm]; out[O_B3] = a; }
  if (tid == H + 1) { float a = 0.0f, b = 0.0f, c = 0.0f; for (int sm = 0; sm < SB; sm++) { a += lce[sm]; b += lent[sm]; c += lacc[sm]; } out[L_CE] = a; out[L_ENT] = b; out[L_ACC] = c; }
  __syncthreads();
  const int col = u0 + li;
  {
    v16f g2[4], acc;
#pragma unroll
    for (int r = 0; r < 16; r++) { g2[0][r] = 0.0f; g2[1][r] = 0.0f; g2[2][r] = 0.0f; g2[3][r] = 0.0f; acc[r] = 0.0f; }
#pragma unroll
    for (int t = 0; t < SB / 2; t++) {                        // dW2ext = h1ext delta2^T  (row 100: db2)
      const float b = S.d2[u0 + li][2 * t + hf];
#pragma unroll
      for (int mt = 0; mt < 4; mt++) g2[mt] = mfma32(S.h1[32 * mt + li][2 * t + hf], b, g2[mt]);
    }
#pragma unroll
    for (int t = 0; t < H / 2; t++) acc = mfma32(S.Wt[O_W2 + (u0 + li) * H + 2 * t + hf], S.d2[2 * t + hf][li], acc);    // W2 delta2
#pragma unroll
    for (int r = 0; r < 16; r++) {                            // delta1 = (W2 delta2) (1 - h1^2)
      const int u = u0 + row32(r, hf);
      if (u < H) { const float h = S.h1[u][li]; S.d1[u][li] = acc[r] * (1.0f - h * h); }
    }
    if (col < H) {
#pragma unroll
      for (int r = 0; r < 16; r++)
#pragma unroll
        for (int mt = 0; mt < 4; mt++) { const int i = 32 * mt + row32(r, hf); if (i <= H) out[O_W2 + i * H + col] = g2[mt][r]; }
    }
  }
  __syncthreads();
  {
    v16f g1[3];
#pragma unroll
    for (int r = 0; r < 16; r++) { g1[0][r] = 0.0f; g1[1][r] = 0.0f; g1[2][r] = 0.0f; }
#pragma unroll
    for (int t = 0; t < SB / 2; t++) {                        // dW1ext = zext delta1^T  (row 84: db1)
      const float b = S.d1[u0 + li][2 * t + hf];
#pragma unroll
      for (int mt = 0; mt < 3; mt++) g1[mt] = mfma32(S.z[32 * mt + li][2 * t + hf], b, g1[mt]);
    }
    if (col < H) {
#pragma unroll
      for (int r = 0; r < 16; r++)
#pragma unroll
        for (int mt = 0; mt < 3; mt++) { const int i = 32 * mt + row32(r, hf); if (i <= IN) out[O_W1 + i * H + col] = g1[mt][r]; }
    }
  }
}

// A block takes 64 parameters; its four waves each sum a quarter of the blocks' partials in block order and the quarters are added in
// order.  One more block (the last) adds the loss sums up: thread t takes blocks t, t + 256, ... in order (float64), the 256 sums are
// added in thread order, and thread 0 writes the six reported values: generator_loss, expert_loss, entropy, entropy_loss, generator_acc,
// expert_acc.  (A lone thread walking 32 768 blocks' sums took 6 ms at 4 096 x 128 rows.)
constexpr int RED_PARAMS = 64, RED_BLOCKS = (NP + RED_PARAMS - 1) / RED_PARAMS;      // launch RED_BLOCKS + 1 blocks
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
  __shared__ float quarter[4][RED_PARAMS];
  const int w = threadIdx.x / RED_PARAMS, p = blockIdx.x * RED_PARAMS + threadIdx.x % RED_PARAMS;
  const int per = (nblk + 3) / 4, b0 = w * per, b1 = min(nblk, b0 + per);
  float g = 0.0f;
  if (p < NP) {
    int b = b0;
    for (; b + 16 <= b1; b += 16) {
      float x[16];
#pragma unroll
      for (int u = 0; u < 16; u++) x[u] = partial[(size_t)(b + u) * NPAD + p];
#pragma unroll
      for (int u = 0; u < 16; u++) g += x[u];
    }
    for (; b < b1; b++) g += partial[(size_t)b * NPAD + p];
  }
  quarter[w][threadIdx.x % RED_PARAMS] = g;
  __syncthreads();
  if (w != 0) return;
  if (p < NP) grad[p] = ((quarter[0][threadIdx.x] + quarter[1][threadIdx.x]) + quarter[2][threadIdx.x]) + quarter[3][threadIdx.x];
}
}  // namespace dmd
