// mlp_tile.h — the fp32 MFMA tile code the learner's kernels share: the value fit (vf_kernel.h), the policy losses, gradient and Fisher
// product (pg_kernel.h) and the GAIL discriminator (disc_kernel.h).  All three are tanh MLPs with two hidden layers of 100 units, run by a block
// of 256 threads (4 waves) on 32-sample tiles, every product on the matrix cores (v_mfma_f32_32x32x2_f32), operands straight from LDS with no
// re-layout between layers:
//   * activations sit transposed, [unit][sample] with a row stride of SBP = 33 floats: a row pair [k, k+1][32 samples] is a B operand (forward,
//     "units x samples" results), a column pair [32 units][s, s+1] is an A or B operand of the weight-gradient products (sum over samples);
//     both reads are bank-conflict free;
//   * the parameters are ONE copy of theta in LDS.  theta's order (W1, b1, W2, b2, W3, b3) makes each bias the row after its matrix, so with a
//     constant row of ones under the input / h1 (/ h2) the biases are part of the products, forward AND backward: the bias gradients are the
//     last rows of the weight-gradient tiles, which land in theta order by themselves;
//   * wave w owns hidden units 32 w .. 32 w + 31 (100 padded to 128: rows past 99 read finite junk and are never stored).  Operand reads past
//     a buffer's rows must stay inside the shared struct, on values that are finite: every pad starts as zero.
// The tile routines are called by all 256 threads of the block.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dml {

constexpr int H = 100, HR = H + 4;                    // hidden units; rows of a hidden activation: + {ones, 3 x zeros}
constexpr int SB = 32, SBP = SB + 1;                  // samples per tile; row stride of the transposed activations

typedef float v16f __attribute__((ext_vector_type(16)));
__device__ inline v16f mfma32(float a, float b, v16f c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
// row of a 32x32 result tile held in register r by the lanes of half `hf`
__device__ inline int row32(int r, int hf) { return 8 * (r / 4) + 4 * hf + (r % 4); }
// tanh(x) = sign(x) (1 - t) / (1 + t), t = exp(-2 |x|): the hardware exponential and reciprocal, absolute error ~1e-7 — an ulp of the
// activation's range, like the float32 graph of the reference.  (The library tanhf is ~60 instructions with two divergent branches: with the
// products on the matrix cores it was a quarter of a tile's time.)
__device__ inline float tanh_fast(float x) {
  const float t = __expf(-2.0f * fabsf(x));
  return copysignf((1.0f - t) * __frcp_rn(1.0f + t), x);
}

// ---- the IN-100-100-1 tanh net: value fit (IN = 56) and discriminator (IN = 84) ---------------------------------------------------
// g[mt] += in_ext delta^T: row tiles mt of the inputs (with their ones row) x this wave's 32 output units, summed over the tile's samples.
template <int MT>
__device__ inline void wgrad_tiles(v16f (&g)[MT], const float (*in)[SBP], const float (*delta)[SBP]) {
  const int l = threadIdx.x & 63, li = l & 31, hf = l >> 5, u0 = 32 * (threadIdx.x >> 6);
#pragma unroll
  for (int t = 0; t < SB / 2; t++) {
    const float b = delta[u0 + li][2 * t + hf];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) g[mt] = mfma32(in[32 * mt + li][2 * t + hf], b, g[mt]);
  }
}
// delta_in = (W2 delta) (1 - h^2) for this wave's 32 hidden units; W2 [H][H] in LDS (row u0 + li of it is the A operand)
__device__ inline void backprop_tanh(const float* W, const float (*delta)[SBP], const float (*h)[SBP], float (*delta_in)[SBP]) {
  const int l = threadIdx.x & 63, li = l & 31, hf = l >> 5, u0 = 32 * (threadIdx.x >> 6);
  v16f acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
  for (int t = 0; t < H / 2; t++) acc = mfma32(W[(u0 + li) * H + 2 * t + hf], delta[2 * t + hf][li], acc);
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int u = u0 + row32(r, hf);
    if (u < H) { const float y = h[u][li]; delta_in[u][li] = acc[r] * (1.0f - y * y); }
  }
}
// rows 0 .. ROWS - 1 (the weights and the bias row) of a weight gradient's tiles, this wave's 32 columns, to out [ROWS][H] in theta order
template <int ROWS, int MT>
__device__ inline void store_tiles(float* __restrict__ out, const v16f (&g)[MT]) {
  const int l = threadIdx.x & 63, li = l & 31, hf = l >> 5, col = 32 * (threadIdx.x >> 6) + li;
  if (col >= H) return;
#pragma unroll
  for (int r = 0; r < 16; r++)
#pragma unroll
    for (int mt = 0; mt < MT; mt++) { const int i = 32 * mt + row32(r, hf); if (i < ROWS) out[i * H + col] = g[mt][r]; }
}

template <int IN>
struct alignas(16) MlpShared {
  static constexpr int O_W1 = 0, O_B1 = O_W1 + IN * H, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + H, NP = O_B3 + 1;
  static constexpr int NPAD = (NP + 63) / 64 * 64;    // a block's row of partial gradients
  static constexpr int NWT = (NP + 3) / 4 * 4, ZR = IN + 2, MT1 = (IN + 32) / 32;   // z: inputs + {ones, zeros}; MT1: row tiles of dW1ext
  float Wt[NWT];                                      // theta: W1 [IN][100], b1, W2 [100][100], b2, w3 [100], b3
  float z[ZR][SBP];                                   // row IN = 1, row IN + 1 = 0
  float h1[HR][SBP], h2[HR][SBP];                     // h1: row 100 = 1, row 101 = 0
  float d2[HR][SBP], d1[HR][SBP];                     // (as operands of the weight-gradient products their 128-row tiles read on into what follows)
  float ypart[8][SB], dy[SB];                         // the head's partial sums; per sample its output, then d loss / d output
  float tail[24 * SBP];                               // ... zeros
};

// Stage theta into LDS and zero every pad; `store_inputs()` then writes the tile's inputs to rows 0 .. IN - 1 of S.z (rows of samples past
// the end: zero).  theta is requested before the pads are zeroed, so the zeroing runs while it is in flight.
template <int IN, class StoreInputs>
__device__ inline void mlp_stage(MlpShared<IN>& S, const float* __restrict__ theta, StoreInputs store_inputs) {
  using L = MlpShared<IN>;
  static_assert(sizeof(L) <= 160 * 1024, "the shared struct must fit a CU's LDS");
  static_assert(L::O_W2 + 101 * H + 128 <= L::NWT + L::ZR * SBP, "padded W2 columns of the forward product read into z");
  static_assert(L::O_W2 + 127 * H + H <= L::NWT + (L::ZR + HR) * SBP, "padded W2 rows (A operand of the backward product) read into z / h1");
  static_assert(32 * L::MT1 <= L::ZR + HR, "the last input tile of dW1 reads into h1");
  static_assert(sizeof(L::ypart) + sizeof(L::dy) + sizeof(L::tail) >= 24 * SBP * sizeof(float), "d1's 128-row tile reads past it");
  constexpr int NP = L::NP, NWT = L::NWT, NT = (NP / 4 + 255) / 256;
  const int tid = threadIdx.x;
  const float4* g = reinterpret_cast<const float4*>(theta);
  float4 th[NT];
#pragma unroll
  for (int j = 0; j < NT; j++) { const int i = tid + 256 * j; th[j] = i < NP / 4 ? g[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
  const float last = tid < NWT - NP / 4 * 4 && NP / 4 * 4 + tid < NP ? theta[NP / 4 * 4 + tid] : 0.0f;
  float4* act = reinterpret_cast<float4*>(&S.z[0][0]);
  for (int i = tid; i < (int)((sizeof(L) - sizeof(S.Wt)) / 16); i += 256) act[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  __syncthreads();
  float4* d = reinterpret_cast<float4*>(S.Wt);
#pragma unroll
  for (int j = 0; j < NT; j++) { const int i = tid + 256 * j; if (i < NP / 4) d[i] = th[j]; }
  if (tid < NWT - NP / 4 * 4) S.Wt[NP / 4 * 4 + tid] = last;
  if (tid < SB) { S.z[IN][tid] = 1.0f; S.h1[H][tid] = 1.0f; }
  store_inputs();
  __syncthreads();
}

// out = tanh(W^T in) for this wave's 32 units; in: ROWS rows (the inputs, the ones row, a zero row), W [ROWS][H]
template <int ROWS>
__device__ inline void tanh_layer(const float* W, const float (*in)[SBP], float (*out)[SBP]) {
  const int l = threadIdx.x & 63, li = l & 31, hf = l >> 5, u0 = 32 * (threadIdx.x >> 6);
  v16f acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
  for (int t = 0; t < ROWS / 2; t++) { const int k = 2 * t + hf; acc = mfma32(W[k * H + u0 + li], in[k][li], acc); }
#pragma unroll
  for (int r = 0; r < 16; r++) { const int u = u0 + row32(r, hf); if (u < H) out[u][li] = tanh_fast(acc[r]); }
}

// Forward pass of the staged tile: h1, h2, then y = w3 . h2 + b3 as eight partial sums per sample added in a fixed order.  Thread sm < SB
// calls out(sm, y) for sample sm (it may write S.dy[sm]); a block barrier follows.
template <int IN, class Out>
__device__ inline void mlp_forward(MlpShared<IN>& S, Out out) {
  using L = MlpShared<IN>;
  const int tid = threadIdx.x;
  tanh_layer<L::ZR>(S.Wt + L::O_W1, S.z, S.h1);
  __syncthreads();
  tanh_layer<H + 2>(S.Wt + L::O_W2, S.h1, S.h2);
  __syncthreads();
  {
    const int sm = tid % SB, part = tid / SB;
    float v = 0.0f;
    for (int j = part; j < H; j += 8) v += S.h2[j][sm] * S.Wt[L::O_W3 + j];
    S.ypart[part][sm] = v;
  }
  __syncthreads();
  if (tid < SB) {
    float v = S.Wt[L::O_B3];
#pragma unroll
    for (int p = 0; p < 8; p++) v += S.ypart[p][tid];
    out(tid, v);
  }
  __syncthreads();
}

// Backward pass from S.dy = d loss / d output per sample (zero for samples past the end): the tile's partial gradient to out (NP floats, theta order).
template <int IN>
__device__ __forceinline__ void mlp_backward(MlpShared<IN>& S, float* __restrict__ out) {
  using L = MlpShared<IN>;
  const int tid = threadIdx.x;
  // delta2 = dy w3 (1 - h2^2);  dw3, db3
  for (int i = tid; i < SB * H; i += 256) { const int j = i / SB, sm = i % SB; const float h = S.h2[j][sm]; S.d2[j][sm] = S.dy[sm] * S.Wt[L::O_W3 + j] * (1.0f - h * h); }
  if (tid < H) { float a = 0.0f; for (int sm = 0; sm < SB; sm++) a += S.h2[tid][sm] * S.dy[sm]; out[L::O_W3 + tid] = a; }
  if (tid == H) { float a = 0.0f; for (int sm = 0; sm < SB; sm++) a += S.dy[sm]; out[L::O_B3] = a; }
  __syncthreads();
  {
    v16f g2[4];
#pragma unroll
    for (int r = 0; r < 16; r++) { g2[0][r] = 0.0f; g2[1][r] = 0.0f; g2[2][r] = 0.0f; g2[3][r] = 0.0f; }
    wgrad_tiles(g2, S.h1, S.d2);                              // dW2ext = h1ext delta2^T  (row 100: db2)
    backprop_tanh(S.Wt + L::O_W2, S.d2, S.h1, S.d1);          // delta1 = (W2 delta2) (1 - h1^2)
    store_tiles<H + 1>(out + L::O_W2, g2);
  }
  __syncthreads();
  v16f g1[L::MT1];
#pragma unroll
  for (int r = 0; r < 16; r++)
#pragma unroll
    for (int mt = 0; mt < L::MT1; mt++) g1[mt][r] = 0.0f;
  wgrad_tiles(g1, S.z, S.d1);                                 // dW1ext = zext delta1^T  (row IN: db1)
  store_tiles<IN + 1>(out + L::O_W1, g1);
}

// ---- fixed-order sums of per-block partial gradients ------------------------------------------------------------------------------
// column p of partial [b][stride] summed over blocks b0 .. b1 - 1 in block order, NF loads in flight (the additions stay in order)
template <int NF>
__device__ inline float column_sum(const float* __restrict__ partial, int stride, int p, int b0, int b1) {
  float g = 0.0f;
  int b = b0;
  for (; b + NF <= b1; b += NF) {
    float x[NF];
#pragma unroll
    for (int u = 0; u < NF; u++) x[u] = partial[(size_t)(b + u) * stride + p];
#pragma unroll
    for (int u = 0; u < NF; u++) g += x[u];
  }
  for (; b < b1; b++) g += partial[(size_t)b * stride + p];
  return g;
}
// A block takes QCOLS parameters, p = blockIdx.x * QCOLS + threadIdx.x % QCOLS; its four waves each sum a quarter of the nblk blocks' partials
// (in block order, sixteen loads in flight) and the quarters are added in order: a fixed summation tree — results do not depend on timing.
// The sum is returned to wave 0 (threads 0 .. QCOLS - 1); columns p >= NP are zero.
constexpr int QCOLS = 64;
template <int NP, int NPAD>
__device__ inline float quarter_sum(const float* __restrict__ partial, int nblk) {
  __shared__ float quarter[4][QCOLS];
  const int w = threadIdx.x / QCOLS, c = threadIdx.x % QCOLS, p = blockIdx.x * QCOLS + c;
  const int per = (nblk + 3) / 4, b0 = w * per, b1 = min(nblk, b0 + per);
  quarter[w][c] = p < NP ? column_sum<16>(partial, NPAD, p, b0, b1) : 0.0f;
  __syncthreads();
  return ((quarter[0][c] + quarter[1][c]) + quarter[2][c]) + quarter[3][c];
}

}  // namespace dml
