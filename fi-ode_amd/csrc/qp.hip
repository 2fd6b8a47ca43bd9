// Standalone FastBarrierProjectionNoUpper (barrier_projection.py:217-313) and eval-mode
// eval_dot (dynamics/classification.py:104-132) with its vector-Jacobian product, for gfx950.
//
// The reference's bisection stops every row at the first iteration where max|eps| < tol over the
// whole batch, reading that max on the host each iteration (barrier_projection.py:247-249).  Each
// row's bisection path is independent of the others, so the same exit is found without host
// syncs in two passes: pass 1 runs all max_iter iterations per row and AND-reduces the per-row
// 32-bit "converged at iteration i" masks into one word; pass 2 reads the word's lowest set bit K
// and re-runs each row to exactly iteration K.
#include "common.h"
#include "tile.h"
#include "../../include/fiode.h"
#include "wgrad.h"

namespace {
using namespace fiode_tile;

__global__ __launch_bounds__(256) void k_qp_mask(int n, const float* lower, const float* nominal, int max_iter,
                                                 float tol, uint32_t* word) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t conv = 0xFFFFFFFFu;
  if (r < n) {
    float lo[C], nm[C], v[C], mu;
    load_row10(lower + (size_t)r * C, lo);
    load_row10(nominal + (size_t)r * C, nm);
    conv = qp_bisect(lo, nm, max_iter - 1, tol, v, mu);
  }
  conv = wave_and(conv);
  if ((threadIdx.x & 63) == 0) atomicAnd(word, conv);
}

__global__ __launch_bounds__(256) void k_qp_final(int n, const float* lower, const float* nominal, int max_iter,
                                                  float tol, const uint32_t* word, float* v_out, float* mu_out,
                                                  int32_t* exit_iter) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = qp_exit_iter(*word, max_iter);
  if (r == 0 && exit_iter) *exit_iter = K;
  if (r >= n) return;
  float lo[C], nm[C], v[C], mu;
  load_row10(lower + (size_t)r * C, lo);
  load_row10(nominal + (size_t)r * C, nm);
  qp_bisect(lo, nm, K, tol, v, mu);
  store_row10(v_out + (size_t)r * C, v);
  if (mu_out) mu_out[r] = mu;
}

__global__ __launch_bounds__(256) void k_qp_bwd(int n, const float* g, const float* v, const float* mu,
                                                const float* nominal, float* g_lower, float* g_nominal) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  float gg[C], vv[C], nm[C], gn[C], gl[C];
  load_row10(g + (size_t)r * C, gg);
  load_row10(v + (size_t)r * C, vv);
  load_row10(nominal + (size_t)r * C, nm);
  qp_backward_row(gg, vv, mu[r], nm, gn, gl);
  if (g_lower) store_row10(g_lower + (size_t)r * C, gl);
  if (g_nominal) store_row10(g_nominal + (size_t)r * C, gn);
}

// ---- eval_dot (eval mode) ------------------------------------------------------------------------
struct DynEvalArgs {
  int N, S, B;
  DynScalars d;
  const float* x_feat;
  const float* h;
  const float *Q1, *b1, *Qx, *bx, *Q2, *b2, *Q3, *b3;
  uint32_t* word;
  float* u;      // [B][M]
  float* ft;     // [N][C]
  float* f;      // [N][C]
  int32_t* exit_iter;
};

__global__ __launch_bounds__(128) void k_dyn_static(DynEvalArgs a) {
  const int b = blockIdx.x, i = threadIdx.x;
  if (b == 0 && i == 0) *a.word = 0xFFFFFFFFu;
  float s = 0.f;
  const float* xb = a.x_feat + (size_t)b * FIODE_X;
#pragma unroll
  for (int c = 0; c < FIODE_X; ++c) s = __fmaf_rn(a.Qx[i * FIODE_X + c], xb[c], s);
  a.u[(size_t)b * M + i] = (s + a.bx[i]) + a.b1[i];
}

template <Act A>
__global__ __launch_bounds__(256) void k_dyn_fwd(DynEvalArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Q2s = smem;
  float* Q3s = smem + M * LDQ;
  load_weight_images(a.Q2, a.Q3, Q2s, Q3s);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
  float q1[4][5];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int s = 0; s < 5; ++s) q1[mb][s] = a.Q1[(32 * mb + col) * C + 2 * s + half];
  const uint32_t kw[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  const int ntiles = (a.N + 31) / 32;
  for (int tile = blockIdx.x * FIODE_WAVES + wave; tile < ntiles; tile += gridDim.x * FIODE_WAVES) {
    const int row = tile * 32 + col;
    const bool valid = row < a.N;
    const int rr = valid ? row : a.N - 1;
    const int b = rr / a.S;
    float h[C];
    load_row10(a.h + (size_t)rr * C, h);
    f32x16 z1[4], z2[4];
    const f32x16 z3 = mlp_tile<false, A>(Q2s, Q3s, q1, a.u + (size_t)b * M, a.b2, a.b3, h, kw, kw, 1.0f, col, half, z1, z2);
    float ft[C], lower[C], nominal[C], sig[C], span[C], v[C], mu;
    gather_ft(z3, half, ft);
    barrier_nominal(a.d, h, ft, lower, nominal, sig, span);
    uint32_t conv = qp_bisect(lower, nominal, a.d.max_iter - 1, a.d.tol, v, mu);
    if (!valid) conv = 0xFFFFFFFFu;
    conv = wave_and(conv);
    if (lane == 0) atomicAnd(a.word, conv);
    if (valid && half == 0) store_row10(a.ft + (size_t)row * C, ft);
  }
}

__global__ __launch_bounds__(256) void k_dyn_final(DynEvalArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = qp_exit_iter(*a.word, a.d.max_iter);
  if (r == 0 && a.exit_iter) *a.exit_iter = K;
  if (r >= a.N) return;
  float h[C], ft[C], lower[C], nominal[C], sig[C], span[C], v[C], mu;
  load_row10(a.h + (size_t)r * C, h);
  load_row10(a.ft + (size_t)r * C, ft);
  barrier_nominal(a.d, h, ft, lower, nominal, sig, span);
  qp_bisect(lower, nominal, K, a.d.tol, v, mu);
  store_row10(a.f + (size_t)r * C, v);
}

// ---- eval_dot backward (eval mode) -----------------------------------------------------------------
// The vector-Jacobian product of fiode_dyn_eval_act on the forward's 32-row wave tiles.  Nothing is
// saved by the forward: a wave recomputes its tile's MLP with the forward's own tile code (the same
// bits), runs the QP to the forward's batch-global exit iteration K (read from device memory) and
// then goes back through QP, barrier and MLP.  All four 32-unit blocks of both hidden layers are in
// the wave's accumulators, so each backward layer's output is directly the next one's B operand and
// a GroupSort pair (u, u + 64) is two registers of one lane: no LDS exchange, no barrier in the loop.
// a1, a2, gz2, gz1 and gft go to the workspace for fiode_internal::launch_wgrad.
struct DynBwdArgs {
  DynEvalArgs e;               // the forward's arguments (word: a scratch word, ft / f / exit_iter unused)
  const float* g_f;            // [N][C]
  const int32_t* exit_iter;    // device int32[1]: the forward's K
  float* g_h;                  // [N][C]
  float *a1, *a2, *gz2, *gz1;  // [N][M]
  float* gft;                  // [N][C]
  fiode_dyn_eval_debug dbg;
};

template <Act A>
__global__ __launch_bounds__(256, 1) void k_dyn_bwd(DynBwdArgs b) {
  const DynEvalArgs& a = b.e;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Q2s = smem;
  float* Q3s = smem + M * LDQ;
  float* Q1s = Q3s + 32 * LDQ;                 // [M][C]
  load_weight_images(a.Q2, a.Q3, Q2s, Q3s);
  for (int e = threadIdx.x; e < M * C; e += blockDim.x) Q1s[e] = a.Q1[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
  float q1[4][5];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int s = 0; s < 5; ++s) q1[mb][s] = a.Q1[(32 * mb + col) * C + 2 * s + half];
  int K = *b.exit_iter;
  K = K < 0 ? 0 : (K > a.d.max_iter - 1 ? a.d.max_iter - 1 : K);
  const int ntiles = (a.N + 31) / 32;
  for (int tile = blockIdx.x * FIODE_WAVES + wave; tile < ntiles; tile += gridDim.x * FIODE_WAVES) {
    const int row = tile * 32 + col;
    const bool valid = row < a.N;
    const int rr = valid ? row : a.N - 1;
    const int img = rr / a.S;
    float h[C];
    load_row10(a.h + (size_t)rr * C, h);
    f32x16 z1[4], z2[4], z3;
    uint32_t codes[4] = {0u, 0u, 0u, 0u};
    if constexpr (A == GROUPSORT) {
      z3 = mlp_tile_groupsort_codes(Q2s, Q3s, q1, a.u + (size_t)img * M, a.b2, a.b3, h, col, half, z1, z2, codes);
    } else {
      const uint32_t kw[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
      z3 = mlp_tile<false, A>(Q2s, Q3s, q1, a.u + (size_t)img * M, a.b2, a.b3, h, kw, kw, 1.0f, col, half, z1, z2);
    }
    float ft[C], lower[C], nominal[C], sig[C], span[C], v[C], mu;
    gather_ft(z3, half, ft);
    barrier_nominal(a.d, h, ft, lower, nominal, sig, span);
    qp_bisect(lower, nominal, K, a.d.tol, v, mu);
    // QP and barrier backward of the row (rows past N: zero upstream gradient, so zero everywhere)
    float g[C], g_nom[C], g_low[C], gft[C], gh[C];
    load_row10(b.g_f + (size_t)rr * C, g);
#pragma unroll
    for (int j = 0; j < C; ++j) g[j] = valid ? g[j] : 0.f;
    qp_backward_row(g, v, mu, nominal, g_nom, g_low);
    // gh: the barrier's part of g_h (through lower and upper); the MLP's part is added below
    // (gsel: this lane's B operand of the Q3^T product, chosen here from values, not by an index)
    const bool scaled = a.d.scale_nominal != 0;
    float gsel[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      float t[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int j = 2 * s + q;
        const float dlow = (-a.d.alpha_1 * a.d.sigma_1) * expf(a.d.sigma_1 * h[j]);
        const float gs = ((g_nom[j] * span[j]) * (1.0f - sig[j])) * sig[j];
        const float ghs = (g_low[j] + g_nom[j] * (1.0f - sig[j])) * dlow + (g_nom[j] * sig[j]) * (-a.d.alpha_2);
        t[q] = scaled ? gs : g_nom[j];
        gh[j] = scaled ? ghs : g_low[j] * dlow;
        gft[j] = t[q];
      }
      gsel[s] = half ? t[1] : t[0];
    }
    if (valid && half == 0) {
      store_row10(b.gft + (size_t)row * C, gft);
      if (b.dbg.f) store_row10(b.dbg.f + (size_t)row * C, v);
      if (b.dbg.qp_lower) store_row10(b.dbg.qp_lower + (size_t)row * C, lower);
      if (b.dbg.qp_nominal) store_row10(b.dbg.qp_nominal + (size_t)row * C, nominal);
      if (b.dbg.mu) b.dbg.mu[row] = mu;
      if (b.dbg.g_ftilde) store_row10(b.dbg.g_ftilde + (size_t)row * C, gft);
    }
    // g_a2^T = Q3^T g_ft^T: A = Q3[2s + half][32 mb + col], B = g_ft[n = col][2s + half]; then layer 2's activation
    f32x16 ga[4] = {f16_zero(), f16_zero(), f16_zero(), f16_zero()};
#pragma unroll
    for (int s = 0; s < 5; ++s) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) ga[mb] = mfma32(Q3s[(2 * s + half) * LDQ + 32 * mb + col], gsel[s], ga[mb]);
    }
    act_backward_tile<A>(z2, ga, codes[2], codes[3]);
    if (valid) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        store_acc_rows(b.a2 + (size_t)row * M, mb, half, z2[mb]);
        store_acc_rows(b.gz2 + (size_t)row * M, mb, half, ga[mb]);
      }
    }
    // g_a1^T = Q2^T g_z2^T: A = Q2[k][32 mb + col] read transposed from the Q2 image, B = g_z2[n = col][k],
    // k = 32 kb + 8 g + 4 half + e: register 4 g + e of this lane's block kb
    f32x16 gb[4] = {f16_zero(), f16_zero(), f16_zero(), f16_zero()};
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const float* q2col = Q2s + (32 * kb + 8 * gq + 4 * half) * LDQ + col;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int mb = 0; mb < 4; ++mb) gb[mb] = mfma32(q2col[e * LDQ + 32 * mb], ga[kb][4 * gq + e], gb[mb]);
      }
      __builtin_amdgcn_sched_barrier(0);   // as mlp12_tile: bound the LDS-read hoisting window to one k-block
    }
    act_backward_tile<A>(z1, gb, codes[0], codes[1]);
    if (valid) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        store_acc_rows(b.a1 + (size_t)row * M, mb, half, z1[mb]);
        store_acc_rows(b.gz1 + (size_t)row * M, mb, half, gb[mb]);
      }
    }
    // Q1^T g_z1 as a padded 32 x 32 block: A = Q1[k][i = col] (zero for i >= C), gathered like the MLP output
    f32x16 dh = f16_zero();
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = 32 * kb + 8 * gq + 4 * half + e;
          dh = mfma32(col < C ? Q1s[k * C + col] : 0.f, gb[kb][4 * gq + e], dh);
        }
    float gq1[C];
    gather_ft(dh, half, gq1);
#pragma unroll
    for (int j = 0; j < C; ++j) gh[j] = gh[j] + gq1[j];
    if (valid && half == 0) store_row10(b.g_h + (size_t)row * C, gh);
  }
}

// Per-image parts of the weight-gradient chain for calls with few rows per image (see
// fiode_dyn_eval_backward): g_u[b] = the image's g_z1 rows summed in row order, then dQx = g_u^T x and
// dx = g_u Qx (fixed-order sums).
__global__ __launch_bounds__(256) void k_dyn_bwd_gu(int B, int S, const float* gz1, float* g_u) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (size_t)B * M) return;
  const size_t b = q / M, i = q - b * M;
  const float* p = gz1 + b * S * M + i;
  float s = 0.f;
  for (int r = 0; r < S; ++r) s += p[(size_t)r * M];
  g_u[q] = s;
}

__global__ __launch_bounds__(256) void k_dyn_bwd_static(int B, const float* g_u, const float* x_feat, const float* Qx,
                                                        float* dQx, float* dx) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < (size_t)M * FIODE_X) {
    const int i = (int)e / FIODE_X, c = (int)e - i * FIODE_X;
    float s = 0.f;
#pragma unroll 16
    for (int b = 0; b < B; ++b) s = __fmaf_rn(g_u[(size_t)b * M + i], x_feat[(size_t)b * FIODE_X + c], s);
    dQx[e] = s;
  } else if (e < (size_t)M * FIODE_X + (size_t)B * FIODE_X) {
    const size_t q = e - (size_t)M * FIODE_X, b = q / FIODE_X;
    const int c = (int)(q - b * FIODE_X);
    float s = 0.f;
#pragma unroll 16
    for (int i = 0; i < M; ++i) s = __fmaf_rn(g_u[b * M + i], Qx[i * FIODE_X + c], s);
    dx[q] = s;
  }
}

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// The weight-gradient chain (fiode_internal::launch_wgrad) stages one image's rows per 40-row chunk,
// so with few rows per image (the ODE function's S = 1) its chunks are nearly empty and a row group
// walks its images one barrier pair at a time (B = 128, S = 1: 309 us measured for the whole backward,
// the chain one group of 128 one-row chunks).  The gradients of Q1, Q2, Q3, b2, b3 and the sum b1 = bx
// do not depend on how rows are grouped into images: below FLAT_ROWS rows per image the chain runs
// with k images merged into one (k: the largest divisor of the batch with k S <= 64 rows), and the
// per-image parts (dQx, dx) come from k_dyn_bwd_gu / k_dyn_bwd_static.  k = 1: the chain as it is.
constexpr int FLAT_ROWS = 32;
inline int merge_factor(int batch, int rows) {
  if (rows >= FLAT_ROWS) return 1;
  int k = 64 / rows < batch ? 64 / rows : batch;
  while (k > 1 && batch % k) --k;
  return k;
}
inline size_t bwd_wgrad_bytes(int batch, int rows) {
  const int k = merge_factor(batch, rows);
  size_t nb = fiode_internal::wgrad_bytes(batch / k, rows * k, true);
  if (k > 1) nb += al((size_t)M * FIODE_X * 4) + al((size_t)batch * M * 4);
  return nb;
}
}  // namespace

extern "C" int fiode_qp_forward(void* stream, int32_t n, int32_t c, const float* lower, const float* nominal,
                                int32_t max_iter, float tol, float* v, float* mu, int32_t* exit_iter,
                                void* workspace, size_t workspace_bytes) {
  if (c != C) return FIODE_ESHAPE;
  if (n < 0 || max_iter < 1 || max_iter > 32 || !workspace || workspace_bytes < 16) return FIODE_EINVAL;
  if (n == 0) return FIODE_OK;
  if (!lower || !nominal || !v) return FIODE_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint32_t* word = static_cast<uint32_t*>(workspace);
  FIODE_HIP_CHECK(hipMemsetAsync(word, 0xFF, 4, st));
  const int blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_qp_mask, dim3(blocks), dim3(256), 0, st, n, lower, nominal, max_iter, tol, word);
  FIODE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_qp_final, dim3(blocks), dim3(256), 0, st, n, lower, nominal, max_iter, tol, word, v, mu,
                     exit_iter);
  FIODE_HIP_CHECK(hipGetLastError());
  return FIODE_OK;
}

extern "C" int fiode_qp_backward(void* stream, int32_t n, int32_t c, const float* g, const float* v,
                                 const float* mu, const float* lower, const float* nominal, float* g_lower,
                                 float* g_nominal) {
  (void)lower;   // the reference's Jacobian depends on lower only through v (barrier_projection.py:288)
  if (c != C) return FIODE_ESHAPE;
  if (n < 0) return FIODE_EINVAL;
  if (n == 0) return FIODE_OK;
  if (!g || !v || !mu || !nominal) return FIODE_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_qp_bwd, dim3((n + 255) / 256), dim3(256), 0, st, n, g, v, mu, nominal, g_lower, g_nominal);
  FIODE_HIP_CHECK(hipGetLastError());
  return FIODE_OK;
}

extern "C" size_t fiode_dyn_eval_workspace_bytes(int32_t n) {
  if (n <= 0) return 256;
  return al(16) + al((size_t)n * M * 4) + al((size_t)n * C * 4);
}

extern "C" int fiode_dyn_eval_act(void* stream, const fiode_dyn_config* dyn, const fiode_dyn_weights* w,
                                  int32_t batch, int32_t rows_per_image, const float* x_feat, const float* h,
                                  float* f, int32_t* exit_iter, void* workspace, size_t workspace_bytes,
                                  int32_t activation) {
  if (!dyn || !w) return FIODE_EINVAL;
  if (activation != FIODE_ACT_RELU && activation != FIODE_ACT_GROUPSORT) return FIODE_EINVAL;
  if (dyn->n_hidden != C || dyn->mlp_size != M || dyn->x_dim != FIODE_X) return FIODE_ESHAPE;
  if (dyn->qp_max_iter < 1 || dyn->qp_max_iter > 32) return FIODE_EINVAL;
  if (batch < 0 || rows_per_image <= 0) return FIODE_EINVAL;
  const long long nl = (long long)batch * rows_per_image;
  if (nl > (1LL << 30)) return FIODE_EINVAL;
  const int n = (int)nl;
  if (n == 0) return FIODE_OK;
  if (!x_feat || !h || !f || !workspace) return FIODE_EINVAL;
  if (workspace_bytes < fiode_dyn_eval_workspace_bytes(n)) return FIODE_EWORKSPACE;
  char* ws = static_cast<char*>(workspace);
  DynEvalArgs a{};
  a.N = n; a.S = rows_per_image; a.B = batch;
  a.d.alpha_1 = dyn->alpha_1; a.d.alpha_2 = dyn->alpha_2; a.d.sigma_1 = dyn->sigma_1;
  a.d.tol = dyn->qp_tol; a.d.scale_nominal = dyn->scale_nominal; a.d.max_iter = dyn->qp_max_iter;
  a.x_feat = x_feat; a.h = h;
  a.Q1 = w->Q1; a.b1 = w->b1; a.Qx = w->Qx; a.bx = w->bx; a.Q2 = w->Q2; a.b2 = w->b2; a.Q3 = w->Q3; a.b3 = w->b3;
  a.word = reinterpret_cast<uint32_t*>(ws);
  a.u = reinterpret_cast<float*>(ws + al(16));
  a.ft = reinterpret_cast<float*>(ws + al(16) + al((size_t)n * M * 4));
  a.f = f;
  a.exit_iter = exit_iter;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_dyn_static, dim3(batch), dim3(128), 0, st, a);
  FIODE_HIP_CHECK(hipGetLastError());
  const int ntiles = (n + 31) / 32;
  const dim3 fgrid((ntiles + FIODE_WAVES - 1) / FIODE_WAVES);
  const size_t flds = (size_t)(M + 32) * LDQ * sizeof(float);
  if (activation == FIODE_ACT_GROUPSORT) hipLaunchKernelGGL(k_dyn_fwd<GROUPSORT>, fgrid, dim3(256), flds, st, a);
  else hipLaunchKernelGGL(k_dyn_fwd<RELU>, fgrid, dim3(256), flds, st, a);
  FIODE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_dyn_final, dim3((n + 255) / 256), dim3(256), 0, st, a);
  FIODE_HIP_CHECK(hipGetLastError());
  return FIODE_OK;
}

extern "C" size_t fiode_dyn_eval_backward_workspace_bytes(int32_t batch, int32_t rows_per_image) {
  if (batch <= 0 || rows_per_image <= 0 || (long long)batch * rows_per_image > (1LL << 30)) return 256;
  const size_t n = (size_t)batch * rows_per_image;
  return al(16) + al((size_t)batch * M * 4) + 4 * al(n * M * 4) + al(n * C * 4) +
         bwd_wgrad_bytes(batch, rows_per_image);
}

extern "C" int fiode_dyn_eval_backward(void* stream, const fiode_dyn_config* dyn, const fiode_dyn_weights* w,
                                       int32_t batch, int32_t rows_per_image, const float* x_feat, const float* h,
                                       const float* g_f, const int32_t* exit_iter, float* g_h,
                                       fiode_lyap_grads* grads, const fiode_dyn_eval_debug* dbg, void* workspace,
                                       size_t workspace_bytes, int32_t activation) {
  if (!dyn || !w) return FIODE_EINVAL;
  if (activation != FIODE_ACT_RELU && activation != FIODE_ACT_GROUPSORT) return FIODE_EINVAL;
  if (dyn->n_hidden != C || dyn->mlp_size != M || dyn->x_dim != FIODE_X) return FIODE_ESHAPE;
  if (dyn->qp_max_iter < 1 || dyn->qp_max_iter > 32) return FIODE_EINVAL;
  if (batch < 0 || rows_per_image <= 0) return FIODE_EINVAL;
  const long long nl = (long long)batch * rows_per_image;
  if (nl > (1LL << 30)) return FIODE_EINVAL;
  const int n = (int)nl;
  if (n == 0) return FIODE_OK;
  if (!x_feat || !h || !g_f || !exit_iter || !g_h || !grads || !workspace) return FIODE_EINVAL;
  if (!w->Q1 || !w->b1 || !w->Qx || !w->bx || !w->Q2 || !w->b2 || !w->Q3 || !w->b3) return FIODE_EINVAL;
  if (!grads->Q1 || !grads->b1 || !grads->Qx || !grads->bx || !grads->Q2 || !grads->b2 || !grads->Q3 ||
      !grads->b3 || !grads->x_feat)
    return FIODE_EINVAL;
  if (workspace_bytes < fiode_dyn_eval_backward_workspace_bytes(batch, rows_per_image)) return FIODE_EWORKSPACE;
  char* ws = static_cast<char*>(workspace);
  DynBwdArgs b{};
  DynEvalArgs& a = b.e;
  a.N = n; a.S = rows_per_image; a.B = batch;
  a.d.alpha_1 = dyn->alpha_1; a.d.alpha_2 = dyn->alpha_2; a.d.sigma_1 = dyn->sigma_1;
  a.d.tol = dyn->qp_tol; a.d.scale_nominal = dyn->scale_nominal; a.d.max_iter = dyn->qp_max_iter;
  a.x_feat = x_feat; a.h = h;
  a.Q1 = w->Q1; a.b1 = w->b1; a.Qx = w->Qx; a.bx = w->bx; a.Q2 = w->Q2; a.b2 = w->b2; a.Q3 = w->Q3; a.b3 = w->b3;
  size_t o = 0;
  a.word = reinterpret_cast<uint32_t*>(ws + o); o += al(16);
  a.u = reinterpret_cast<float*>(ws + o); o += al((size_t)batch * M * 4);
  const size_t nm = al((size_t)n * M * 4);
  b.a1 = reinterpret_cast<float*>(ws + o); o += nm;
  b.a2 = reinterpret_cast<float*>(ws + o); o += nm;
  b.gz2 = reinterpret_cast<float*>(ws + o); o += nm;
  b.gz1 = reinterpret_cast<float*>(ws + o); o += nm;
  b.gft = reinterpret_cast<float*>(ws + o); o += al((size_t)n * C * 4);
  b.g_f = g_f; b.exit_iter = exit_iter; b.g_h = g_h;
  if (dbg) b.dbg = *dbg;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_dyn_static, dim3(batch), dim3(128), 0, st, a);
  FIODE_HIP_CHECK(hipGetLastError());
  const int ntiles = (n + 31) / 32;
  const dim3 grid((ntiles + FIODE_WAVES - 1) / FIODE_WAVES);
  const size_t lds = ((size_t)(M + 32) * LDQ + (size_t)M * C) * sizeof(float);
  if (activation == FIODE_ACT_GROUPSORT) hipLaunchKernelGGL(k_dyn_bwd<GROUPSORT>, grid, dim3(256), lds, st, b);
  else hipLaunchKernelGGL(k_dyn_bwd<RELU>, grid, dim3(256), lds, st, b);
  FIODE_HIP_CHECK(hipGetLastError());
  // weight and x_feat gradients from the per-row activations and activation gradients (rows r = b S + s)
  fiode_internal::WgradIO io{};
  io.x_feat = x_feat; io.Qx = w->Qx; io.h = h;
  io.a1 = b.a1; io.a2 = b.a2; io.gz2 = b.gz2; io.gz1 = b.gz1; io.gft = b.gft;
  io.s_used = nullptr;
  io.grads = *grads;
  const int k = merge_factor(batch, rows_per_image);
  io.B = batch / k; io.S = rows_per_image * k;
  io.workspace = ws + o;
  if (k == 1) return fiode_internal::launch_wgrad(st, io);
  // k images as one: the chain's dQx / dx are not the call's and go to scratch / nowhere
  o += fiode_internal::wgrad_bytes(io.B, io.S, true);
  io.grads.Qx = reinterpret_cast<float*>(ws + o); o += al((size_t)M * FIODE_X * 4);
  io.grads.x_feat = nullptr;
  float* g_u = reinterpret_cast<float*>(ws + o);
  const int rc = fiode_internal::launch_wgrad(st, io);
  if (rc) return rc;
  hipLaunchKernelGGL(k_dyn_bwd_gu, dim3((unsigned)(((size_t)batch * M + 255) / 256)), dim3(256), 0, st, batch,
                     rows_per_image, b.gz1, g_u);
  FIODE_HIP_CHECK(hipGetLastError());
  const size_t items = (size_t)M * FIODE_X + (size_t)batch * FIODE_X;
  hipLaunchKernelGGL(k_dyn_bwd_static, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, batch, g_u, x_feat,
                     w->Qx, grads->Qx, grads->x_feat);
  FIODE_HIP_CHECK(hipGetLastError());
  return FIODE_OK;
}

extern "C" int fiode_dyn_eval(void* stream, const fiode_dyn_config* dyn, const fiode_dyn_weights* w, int32_t batch,
                              int32_t rows_per_image, const float* x_feat, const float* h, float* f,
                              int32_t* exit_iter, void* workspace, size_t workspace_bytes) {
  return fiode_dyn_eval_act(stream, dyn, w, batch, rows_per_image, x_feat, h, f, exit_iter, workspace, workspace_bytes,
                            FIODE_ACT_RELU);
}

extern "C" const char* fiode_error_string(int code) {
  switch (code) {
    case FIODE_OK: return "ok";
    case FIODE_EINVAL: return "invalid argument";
    case FIODE_ESHAPE: return "unsupported shape (dynamics: n_hidden=10, mlp_size=128, x_dim=10; spectral: 3x3 taps, min(cout, cin) <= 64, n <= 64; transforms: n in {8, 16, 32})";
    case FIODE_EWORKSPACE: return "workspace too small";
    default: return code >= FIODE_EHIP ? hipGetErrorString((hipError_t)(code - FIODE_EHIP)) : "unknown error";
  }
}

extern "C" int fiode_abi_version(void) { return FIODE_ABI_VERSION; }
