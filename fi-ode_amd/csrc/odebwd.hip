// Input gradients of the eval-mode fixed-grid RK4 solve (fiode_odeint_act, method rk4, 3/8 rule):
// given g_y = dL/dy(t1) and the forward's step states y_n (the solve asked for its own grid as
// output times), dL/dh0 and dL/dx_feat.  No weight gradients: an attack on the image discards them.
//
// Replay: four passes, one per RK4 stage.  Pass s evaluates stage s of ALL steps at once (rows
// n_steps x B; given y_n the stages of different steps are independent), with the forward's 32-row
// wave tiles of k_dyn_fwd and the QP's batch-global exit taken per group of B rows (one step's eval),
// each group with its own exit word.  It leaves k[n][s][B][C] and the exit iterations K[n][s].
//
// Reverse sweep: one wave per 32-row tile of the batch, no dependence between tiles (no exchange, no
// polling, no grid sizing).  For n from last to first and s from 4 to 1 the wave rebuilds the stage
// input from y_n and the saved k, runs the tile vector-Jacobian product of one dynamics evaluation
// (the code of k_dyn_bwd in qp.hip without its stores: MLP recompute, QP to K[n][s], QP / barrier /
// MLP backward) and applies the RK4 adjoint combinations in registers.  g_z1 of every evaluation is
// the gradient of u[b] = U_x x_b + bx + b1: it accumulates in the wave's accumulators over the whole
// sweep and g_u [B][M] is written once; g_x = g_u Qx follows.
//
// The dopri5 solve has the same two phases over its logged accepted steps (seven stages, the dense
// output at t1 in the last step): the second half of this file, fiode_odeint_dopri5_backward_x.
#include "common.h"
#include "tile.h"
#include "dopri5.h"
#include "../../include/fiode.h"

namespace {
using namespace fiode_tile;

constexpr int OBX_MAX_STEPS = 1024;

struct ObxArgs {
  int B, n_steps, N;             // N = n_steps * B rows of a replay pass
  float t0, t1, hs;
  DynScalars d;
  const float* x_feat;
  const float* ys;               // [n_steps + 1][B][C] step states (ys[0] = h0)
  const float *Q1, *b1, *Qx, *bx, *Q2, *b2, *Q3, *b3;
  const float* g_y;              // [B][C]
  float* g_h0;                   // [B][C]
  float* g_x;                    // [B][X]
  uint32_t* words;               // [4][n_steps] exit words of the replay
  int32_t* Kx;                   // [n_steps][4] exit iterations
  float* u;                      // [B][M]
  float* k;                      // [n_steps][4][B][C] stage derivatives
  float* ft;                     // [N][C] MLP output of the current pass
  float* g_u;                    // [B][M]
};

// step n of the FixedGridODESolver grid in float32, as os_rk4 (odesolve.hip) forms it
__device__ __forceinline__ float obx_dt(const ObxArgs& a, int n) {
  const float ta = (float)n * a.hs + a.t0;
  const float tb = (n + 1 == a.n_steps) ? a.t1 : (float)(n + 1) * a.hs + a.t0;
  return tb - ta;
}

// input of stage s (0..3) of step n for batch row b: the float32 expressions of stage_input
// (odesolve.hip; rk4_alt_step_func), from y_n and the replay's k of the earlier stages
__device__ __forceinline__ void obx_stage_input(const ObxArgs& a, int n, int s, int b, float dt, float (&h)[C]) {
  const size_t BC = (size_t)a.B * C;
  const float* kr = a.k + (size_t)n * 4 * BC + (size_t)b * C;
  float y[C];
  load_row10(a.ys + (size_t)n * BC + (size_t)b * C, y);
  const float third = 1.0f / 3.0f;
  if (s == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) h[c] = y[c];
    return;
  }
  float f1[C], f2[C], f3[C];
  load_row10(kr, f1);
  if (s == 1) {
#pragma unroll
    for (int c = 0; c < C; ++c) h[c] = y[c] + (dt * f1[c]) * third;
    return;
  }
  load_row10(kr + BC, f2);
  if (s == 2) {
#pragma unroll
    for (int c = 0; c < C; ++c) h[c] = y[c] + dt * (f2[c] - f1[c] * third);
    return;
  }
  load_row10(kr + 2 * BC, f3);
#pragma unroll
  for (int c = 0; c < C; ++c) h[c] = y[c] + dt * ((f1[c] - f2[c]) + f3[c]);
}

__global__ __launch_bounds__(128) void k_obx_static(ObxArgs a) {
  const int b = blockIdx.x, i = threadIdx.x;
  if (b == 0)
    for (int e = i; e < 4 * a.n_steps; e += blockDim.x) a.words[e] = 0xFFFFFFFFu;
  float s = 0.f;
  const float* xb = a.x_feat + (size_t)b * FIODE_X;
#pragma unroll
  for (int c = 0; c < FIODE_X; ++c) s = __fmaf_rn(a.Qx[i * FIODE_X + c], xb[c], s);
  a.u[(size_t)b * M + i] = (s + a.bx[i]) + a.b1[i];
}

// pass s, part 1: MLP and the full bisection of every row; the convergence masks are AND-reduced per
// step (group of B rows).  A tile inside one step reduces over the wave first (one atomic); a tile
// that straddles steps (B < 32 or a step boundary) sends one atomic per row.
template <Act A>
__global__ __launch_bounds__(256) void k_obx_stage(ObxArgs a, int s) {
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
    for (int t = 0; t < 5; ++t) q1[mb][t] = a.Q1[(32 * mb + col) * C + 2 * t + half];
  const uint32_t kw[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  const int ntiles = (a.N + 31) / 32;
  for (int tile = blockIdx.x * FIODE_WAVES + wave; tile < ntiles; tile += gridDim.x * FIODE_WAVES) {
    const int row = tile * 32 + col;
    const bool valid = row < a.N;
    const int rr = valid ? row : a.N - 1;
    const int n = rr / a.B, b = rr - n * a.B;
    float h[C];
    obx_stage_input(a, n, s, b, obx_dt(a, n), h);
    f32x16 z1[4], z2[4];
    const f32x16 z3 = mlp_tile<false, A>(Q2s, Q3s, q1, a.u + (size_t)b * M, a.b2, a.b3, h, kw, kw, 1.0f, col, half, z1, z2);
    float ft[C], lower[C], nominal[C], sig[C], span[C], v[C], mu;
    gather_ft(z3, half, ft);
    barrier_nominal(a.d, h, ft, lower, nominal, sig, span);
    uint32_t conv = qp_bisect(lower, nominal, a.d.max_iter - 1, a.d.tol, v, mu);
    if (!valid) conv = 0xFFFFFFFFu;
    const int n0 = __shfl(n, 0, 64);
    uint32_t* wrow = a.words + (size_t)s * a.n_steps;
    if (__all(n == n0)) {
      conv = wave_and(conv);
      if (lane == 0) atomicAnd(wrow + n0, conv);
    } else if (valid && half == 0) {
      atomicAnd(wrow + n, conv);
    }
    if (valid && half == 0) store_row10(a.ft + (size_t)row * C, ft);
  }
}

// pass s, part 2: every row to its step's exit iteration; k[n][s] and K[n][s]
__global__ __launch_bounds__(256) void k_obx_final(ObxArgs a, int s) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.N) return;
  const int n = r / a.B, b = r - n * a.B;
  const int K = qp_exit_iter(a.words[(size_t)s * a.n_steps + n], a.d.max_iter);
  if (b == 0) a.Kx[n * 4 + s] = K;
  float h[C], ft[C], lower[C], nominal[C], sig[C], span[C], v[C], mu;
  obx_stage_input(a, n, s, b, obx_dt(a, n), h);
  load_row10(a.ft + (size_t)r * C, ft);
  barrier_nominal(a.d, h, ft, lower, nominal, sig, span);
  qp_bisect(lower, nominal, K, a.d.tol, v, mu);
  store_row10(a.k + (((size_t)n * 4 + s) * a.B + b) * C, v);
}

// The vector-Jacobian product of one dynamics evaluation on a 32-row wave tile, given its exit
// iteration K: gh = J_h^T g, and g_z1 (the gradient of u) is ADDED to gu.  k_dyn_bwd's tile code
// (qp.hip) without the weight-gradient stores; rows past the batch carry g = 0 and give zeros.
template <Act A>
__device__ __forceinline__ void obx_vjp_tile(const DynScalars& d, const float* Q2s, const float* Q3s, const float* Q1s,
                                             const float (&q1)[4][5], const float* u_row, const float* b2,
                                             const float* b3, const float (&h)[C], const float (&g)[C], int K, int col,
                                             int half, float (&gh)[C], f32x16 (&gu)[4]) {
  f32x16 z1[4], z2[4], z3;
  uint32_t codes[4] = {0u, 0u, 0u, 0u};
  if constexpr (A == GROUPSORT) {
    z3 = mlp_tile_groupsort_codes(Q2s, Q3s, q1, u_row, b2, b3, h, col, half, z1, z2, codes);
  } else {
    const uint32_t kw[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    z3 = mlp_tile<false, A>(Q2s, Q3s, q1, u_row, b2, b3, h, kw, kw, 1.0f, col, half, z1, z2);
  }
  float ft[C], lower[C], nominal[C], sig[C], span[C], v[C], mu;
  gather_ft(z3, half, ft);
  barrier_nominal(d, h, ft, lower, nominal, sig, span);
  qp_bisect(lower, nominal, K, d.tol, v, mu);
  float g_nom[C], g_low[C];
  qp_backward_row(g, v, mu, nominal, g_nom, g_low);
  // gh: the barrier's part (through lower and upper); gsel: this lane's B operand of the Q3^T product
  const bool scaled = d.scale_nominal != 0;
  float gsel[5];
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    float t[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = 2 * s + q;
      const float dlow = (-d.alpha_1 * d.sigma_1) * expf(d.sigma_1 * h[j]);
      const float gs = ((g_nom[j] * span[j]) * (1.0f - sig[j])) * sig[j];
      const float ghs = (g_low[j] + g_nom[j] * (1.0f - sig[j])) * dlow + (g_nom[j] * sig[j]) * (-d.alpha_2);
      t[q] = scaled ? gs : g_nom[j];
      gh[j] = scaled ? ghs : g_low[j] * dlow;
    }
    gsel[s] = half ? t[1] : t[0];
  }
  // g_a2^T = Q3^T g_ft^T, then layer 2's activation
  f32x16 ga[4] = {f16_zero(), f16_zero(), f16_zero(), f16_zero()};
#pragma unroll
  for (int s = 0; s < 5; ++s) {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) ga[mb] = mfma32(Q3s[(2 * s + half) * LDQ + 32 * mb + col], gsel[s], ga[mb]);
  }
  act_backward_tile<A>(z2, ga, codes[2], codes[3]);
  // g_a1^T = Q2^T g_z2^T (A read transposed from the Q2 image), then layer 1's activation
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
    __builtin_amdgcn_sched_barrier(0);
  }
  act_backward_tile<A>(z1, gb, codes[0], codes[1]);
  // Q1^T g_z1 as a padded 32 x 32 block, gathered like the MLP output
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
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) gu[mb][r] = gu[mb][r] + gb[mb][r];
}

// The reverse sweep.  Forward step (dt, 3/8 rule):  h2 = y + (dt k1)/3,  h3 = y + dt (k2 - k1/3),
// h4 = y + dt (k1 - k2 + k3),  y' = y + (k1 + 3 (k2 + k3) + k4) dt / 8.  With a = dL/dy':
// gk1 = gk4 = a dt / 8, gk2 = gk3 = 3 a dt / 8, and stage s = 4 .. 1 with gh = J(h_s)^T gk_s adds gh to
// dL/dy and (c1, c2, c3) gh to (gk1, gk2, gk3): s = 4: (dt, -dt, dt); 3: (-dt/3, dt, 0); 2: (dt/3, 0, 0).
template <Act A>
__global__ __launch_bounds__(256, 1) void k_ode_bwd_x(ObxArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Q2s = smem;
  float* Q3s = smem + M * LDQ;
  float* Q1s = Q3s + 32 * LDQ;                 // [M][C]
  load_weight_images(a.Q2, a.Q3, Q2s, Q3s);
  for (int e = threadIdx.x; e < M * C; e += blockDim.x) Q1s[e] = a.Q1[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
  const int tile = blockIdx.x * (blockDim.x >> 6) + wave;
  if (tile * 32 >= a.B) return;                // no barrier below
  float q1[4][5];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int t = 0; t < 5; ++t) q1[mb][t] = a.Q1[(32 * mb + col) * C + 2 * t + half];
  const int row = tile * 32 + col;
  const bool valid = row < a.B;
  const int b = valid ? row : a.B - 1;
  const float* u_row = a.u + (size_t)b * M;
  float gy[C];
  load_row10(a.g_y + (size_t)b * C, gy);
#pragma unroll
  for (int j = 0; j < C; ++j) gy[j] = valid ? gy[j] : 0.f;
  f32x16 gu[4] = {f16_zero(), f16_zero(), f16_zero(), f16_zero()};
  const float third = 1.0f / 3.0f;
  for (int n = a.n_steps - 1; n >= 0; --n) {
    const float dt = obx_dt(a, n);
    float gk1[C], gk2[C], gk3[C], gk4[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const float w = (gy[j] * dt) * 0.125f;
      gk1[j] = w;
      gk4[j] = w;
      gk2[j] = 3.0f * w;
      gk3[j] = 3.0f * w;
    }
#pragma unroll 1
    for (int s = 3; s >= 0; --s) {
      int K = a.Kx[n * 4 + s];
      K = K < 0 ? 0 : (K > a.d.max_iter - 1 ? a.d.max_iter - 1 : K);
      float h[C], g[C], gh[C];
      obx_stage_input(a, n, s, b, dt, h);
#pragma unroll
      for (int j = 0; j < C; ++j) g[j] = s == 3 ? gk4[j] : (s == 2 ? gk3[j] : (s == 1 ? gk2[j] : gk1[j]));
      obx_vjp_tile<A>(a.d, Q2s, Q3s, Q1s, q1, u_row, a.b2, a.b3, h, g, K, col, half, gh, gu);
      const float c1 = s == 3 ? dt : (s == 2 ? -(dt * third) : (s == 1 ? dt * third : 0.f));
      const float c2 = s == 3 ? -dt : (s == 2 ? dt : 0.f);
      const float c3 = s == 3 ? dt : 0.f;
#pragma unroll
      for (int j = 0; j < C; ++j) {
        gy[j] = gy[j] + gh[j];
        gk1[j] = gk1[j] + c1 * gh[j];
        gk2[j] = gk2[j] + c2 * gh[j];
        gk3[j] = gk3[j] + c3 * gh[j];
      }
    }
  }
  if (valid) {
    if (half == 0) store_row10(a.g_h0 + (size_t)row * C, gy);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) store_acc_rows(a.g_u + (size_t)row * M, mb, half, gu[mb]);
  }
}

// g_x = g_u Qx (fixed-order sums), one thread per element
__global__ __launch_bounds__(256) void k_obx_gx(ObxArgs a) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= (size_t)a.B * FIODE_X) return;
  const size_t b = q / FIODE_X;
  const int c = (int)(q - b * FIODE_X);
  float s = 0.f;
#pragma unroll 16
  for (int i = 0; i < M; ++i) s = __fmaf_rn(a.g_u[b * M + i], a.Qx[i * FIODE_X + c], s);
  a.g_x[q] = s;
}

// ---- dopri5: the gradient on the accepted steps (fiode_odeint_dopri5_backward_x) -----------------
// The log of fiode_odeint_act_log gives (t_n, dt_n) and y_n of every accepted step; the step sizes
// are constants of the gradient (the controller carries none).  Stage numbering: s = 0 is k1 = f(y),
// s = 1..6 is k_{s+1} = f(y + dt sum_{j<s} DP_BETA[s-1][j] k_{j+1}); s = 6 is k7 = f(y1), which only the
// last step needs (elsewhere it is the next step's k1).  Per step, with a = dL/dy_{n+1}:
//   gy = a, gk_j = dt DP_BETA[5][j] a;  s = 5 .. 0: gh = J(h_s)^T gk_s, gy += gh, gk_j += dt DP_BETA[s-1][j] gh.
// The last step ends past t1 and the solve interpolates (os_dopri5): with g = dL/dy(t1), x formed as
// there and the quartic's weights p0 (y), p1 (y1), pm (ymid), pa (dt k1), pb (dt k7):
//   a = p1 g, gy = a + (p0 + pm) g, gk_j += dt DP_CMID[j] pm g, gk_1 += dt pa g, gk_7 += dt pb g,
// and the stage loop starts at s = 6, whose input y1 obeys the same rule with DP_BETA[5].
using namespace fiode_dp;

struct DpxArgs {
  int B, n_steps;
  double t1;
  DynScalars d;
  const double* times;           // [n_steps][2] (t_n, dt_n)
  const float* x_feat;
  const float* ys;               // [n_steps][B][C] y_n at the start of step n
  const float *Q1, *b1, *Qx, *bx, *Q2, *b2, *Q3, *b3;
  const float* g_y;              // [B][C]
  float* g_h0;                   // [B][C]
  uint32_t* words;               // [7][n_steps] exit words of the replay
  int32_t* Kx;                   // [n_steps][7] exit iterations
  float* u;                      // [B][M]
  float* k;                      // [n_steps][7][B][C] stage derivatives
  float* ft;                     // [n_steps B][C] MLP output of the current pass
  float* g_u;                    // [B][M]
};

// input of stage s (0..6) of step n for batch row b: the float32 expressions of stage_input(IN_DP)
// (odesolve.hip), from y_n and the replay's k of the earlier stages
__device__ __forceinline__ void dpx_stage_input(const DpxArgs& a, int n, int s, int b, float dt, float (&h)[C]) {
  const size_t BC = (size_t)a.B * C;
  const float* kr = a.k + (size_t)n * 7 * BC + (size_t)b * C;
  float y[C];
  load_row10(a.ys + (size_t)n * BC + (size_t)b * C, y);
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  for (int jj = 0; jj < s; ++jj) {
    float f[C];
    load_row10(kr + (size_t)jj * BC, f);
    const float co = DP_BETA[s - 1][jj] * dt;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = acc[c] + f[c] * co;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) h[c] = s == 0 ? y[c] : y[c] + acc[c];
}

__global__ __launch_bounds__(128) void k_dpx_static(DpxArgs a) {
  const int b = blockIdx.x, i = threadIdx.x;
  if (b == 0)
    for (int e = i; e < 7 * a.n_steps; e += blockDim.x) {
      a.words[e] = 0xFFFFFFFFu;
      if (e % 7 == 6) a.Kx[e] = -1;          // k7: evaluated for the last step only
    }
  float s = 0.f;
  const float* xb = a.x_feat + (size_t)b * FIODE_X;
#pragma unroll
  for (int c = 0; c < FIODE_X; ++c) s = __fmaf_rn(a.Qx[i * FIODE_X + c], xb[c], s);
  a.u[(size_t)b * M + i] = (s + a.bx[i]) + a.b1[i];
}

// pass s over the steps n0 .. n0 + N / B - 1 (N rows), part 1: k_obx_stage with the dopri5 stage input
template <Act A>
__global__ __launch_bounds__(256) void k_dpx_stage(DpxArgs a, int s, int n0, int N) {
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
    for (int t = 0; t < 5; ++t) q1[mb][t] = a.Q1[(32 * mb + col) * C + 2 * t + half];
  const uint32_t kw[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  const int ntiles = (N + 31) / 32;
  for (int tile = blockIdx.x * FIODE_WAVES + wave; tile < ntiles; tile += gridDim.x * FIODE_WAVES) {
    const int row = tile * 32 + col;
    const bool valid = row < N;
    const int rr = valid ? row : N - 1;
    const int n = n0 + rr / a.B, b = rr % a.B;
    float h[C];
    dpx_stage_input(a, n, s, b, (float)a.times[2 * n + 1], h);
    f32x16 z1[4], z2[4];
    const f32x16 z3 = mlp_tile<false, A>(Q2s, Q3s, q1, a.u + (size_t)b * M, a.b2, a.b3, h, kw, kw, 1.0f, col, half, z1, z2);
    float ft[C], lower[C], nominal[C], sig[C], span[C], v[C], mu;
    gather_ft(z3, half, ft);
    barrier_nominal(a.d, h, ft, lower, nominal, sig, span);
    uint32_t conv = qp_bisect(lower, nominal, a.d.max_iter - 1, a.d.tol, v, mu);
    if (!valid) conv = 0xFFFFFFFFu;
    const int nf = __shfl(n, 0, 64);
    uint32_t* wrow = a.words + (size_t)s * a.n_steps;
    if (__all(n == nf)) {
      conv = wave_and(conv);
      if (lane == 0) atomicAnd(wrow + nf, conv);
    } else if (valid && half == 0) {
      atomicAnd(wrow + n, conv);
    }
    if (valid && half == 0) store_row10(a.ft + (size_t)row * C, ft);
  }
}

// pass s, part 2: every row to its step's exit iteration; k[n][s] and K[n][s]
__global__ __launch_bounds__(256) void k_dpx_final(DpxArgs a, int s, int n0, int N) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= N) return;
  const int n = n0 + r / a.B, b = r % a.B;
  const int K = qp_exit_iter(a.words[(size_t)s * a.n_steps + n], a.d.max_iter);
  if (b == 0) a.Kx[n * 7 + s] = K;
  float h[C], ft[C], lower[C], nominal[C], sig[C], span[C], v[C], mu;
  dpx_stage_input(a, n, s, b, (float)a.times[2 * n + 1], h);
  load_row10(a.ft + (size_t)r * C, ft);
  barrier_nominal(a.d, h, ft, lower, nominal, sig, span);
  qp_bisect(lower, nominal, K, a.d.tol, v, mu);
  store_row10(a.k + (((size_t)n * 7 + s) * a.B + b) * C, v);
}

// The reverse sweep over the accepted steps (the comment at the head of this section).
template <Act A>
__global__ __launch_bounds__(256, 1) void k_ode_bwd_x_dp(DpxArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Q2s = smem;
  float* Q3s = smem + M * LDQ;
  float* Q1s = Q3s + 32 * LDQ;                 // [M][C]
  load_weight_images(a.Q2, a.Q3, Q2s, Q3s);
  for (int e = threadIdx.x; e < M * C; e += blockDim.x) Q1s[e] = a.Q1[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
  const int tile = blockIdx.x * (blockDim.x >> 6) + wave;
  if (tile * 32 >= a.B) return;                // no barrier below
  float q1[4][5];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int t = 0; t < 5; ++t) q1[mb][t] = a.Q1[(32 * mb + col) * C + 2 * t + half];
  const int row = tile * 32 + col;
  const bool valid = row < a.B;
  const int b = valid ? row : a.B - 1;
  const float* u_row = a.u + (size_t)b * M;
  float gy[C];
  load_row10(a.g_y + (size_t)b * C, gy);
#pragma unroll
  for (int j = 0; j < C; ++j) gy[j] = valid ? gy[j] : 0.f;
  f32x16 gu[4] = {f16_zero(), f16_zero(), f16_zero(), f16_zero()};
  const int last = a.n_steps - 1;
  for (int n = last; n >= 0; --n) {
    const double tn = a.times[2 * n], dtn = a.times[2 * n + 1];
    const float dt = (float)dtn;
    // weights of the dense output at t1 (last step), or y_{n+1} = y1 itself
    float p0 = 0.f, p1 = 1.f, pm = 0.f, pa = 0.f, pb = 0.f;
    if (n == last) {
      const float x = (float)((a.t1 - tn) / ((tn + dtn) - tn));
      const float x2 = x * x, x3 = x2 * x, x4 = x3 * x;
      p0 = ((1.0f - 11.0f * x2) + 18.0f * x3) - 8.0f * x4;
      p1 = (14.0f * x3 - 5.0f * x2) - 8.0f * x4;
      pm = (16.0f * x2 - 32.0f * x3) + 16.0f * x4;
      pa = ((x - 4.0f * x2) + 5.0f * x3) - 2.0f * x4;
      pb = (x2 - 3.0f * x3) + 2.0f * x4;
    }
    float gk[7][C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float g = gy[c], av = p1 * g, gm = (dt * pm) * g;
#pragma unroll
      for (int j = 0; j < 6; ++j) gk[j][c] = (dt * DP_BETA[5][j]) * av + DP_CMID[j] * gm;
      gk[0][c] = gk[0][c] + (dt * pa) * g;
      gk[6][c] = (dt * pb) * g + DP_CMID[6] * gm;
      gy[c] = av + (p0 + pm) * g;
    }
#pragma unroll 1
    for (int s = (n == last ? 6 : 5); s >= 0; --s) {
      int K = a.Kx[n * 7 + s];
      K = K < 0 ? 0 : (K > a.d.max_iter - 1 ? a.d.max_iter - 1 : K);
      float h[C], g[C], gh[C];
      dpx_stage_input(a, n, s, b, dt, h);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float t = gk[0][c];
#pragma unroll
        for (int j = 1; j < 7; ++j) t = s == j ? gk[j][c] : t;
        g[c] = t;
      }
      obx_vjp_tile<A>(a.d, Q2s, Q3s, Q1s, q1, u_row, a.b2, a.b3, h, g, K, col, half, gh, gu);
      const int i = s > 0 ? s - 1 : 0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const float cj = j < s ? DP_BETA[i][j] * dt : 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) gk[j][c] = gk[j][c] + cj * gh[c];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) gy[c] = gy[c] + gh[c];
    }
  }
  if (valid) {
    if (half == 0) store_row10(a.g_h0 + (size_t)row * C, gy);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) store_acc_rows(a.g_u + (size_t)row * M, mb, half, gu[mb]);
  }
}

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct DpxLayout {
  size_t words, Kx, u, k, ft, g_u, total;
};
DpxLayout dpx_layout(int B, int n_steps) {
  const size_t N = (size_t)n_steps * B;
  DpxLayout L;
  size_t o = 0;
  L.words = o; o += al((size_t)7 * n_steps * 4);
  L.Kx = o; o += al((size_t)7 * n_steps * 4);
  L.u = o; o += al((size_t)B * M * 4);
  L.k = o; o += al(7 * N * C * 4);
  L.ft = o; o += al(N * C * 4);
  L.g_u = o; o += al((size_t)B * M * 4);
  L.total = o;
  return L;
}

// steps of the float32 grid (os_rk4: niters = ceil((t1 - t0) / h + 1)), or -1
int obx_steps(double t0, double t1, double step_size) {
  if (!(step_size > 0) || !(t1 > t0)) return -1;
  const float f0 = (float)t0, f1 = (float)t1, hs = (float)step_size;
  if (!(hs > 0.f) || !(f1 > f0)) return -1;
  const float q = (f1 - f0) / hs + 1.0f;
  if (!(q <= (float)(OBX_MAX_STEPS + 1))) return -1;
  const int niters = (int)ceilf(q);
  return niters - 1 >= 1 ? niters - 1 : -1;
}

struct ObxLayout {
  size_t words, Kx, u, k, ft, g_u, total;
};
ObxLayout obx_layout(int B, int n_steps) {
  const size_t N = (size_t)n_steps * B;
  ObxLayout L;
  size_t o = 0;
  L.words = o; o += al((size_t)4 * n_steps * 4);
  L.Kx = o; o += al((size_t)4 * n_steps * 4);
  L.u = o; o += al((size_t)B * M * 4);
  L.k = o; o += al(4 * N * C * 4);
  L.ft = o; o += al(N * C * 4);
  L.g_u = o; o += al((size_t)B * M * 4);
  L.total = o;
  return L;
}
}  // namespace

extern "C" int32_t fiode_odeint_backward_x_steps(double t0, double t1, double step_size) {
  return obx_steps(t0, t1, step_size);
}

extern "C" size_t fiode_odeint_backward_x_workspace_bytes(int32_t batch, double t0, double t1, double step_size) {
  const int n_steps = obx_steps(t0, t1, step_size);
  if (batch <= 0 || batch > FIODE_ODEINT_MAX_BATCH || n_steps < 0) return 256;
  return obx_layout(batch, n_steps).total;
}

extern "C" int fiode_odeint_backward_x(void* stream, const fiode_dyn_config* dyn, const fiode_dyn_weights* w,
                                       int32_t batch, double t0, double t1, double step_size, const float* x_feat,
                                       const float* states, const float* g_y, float* g_h0, float* g_x_feat,
                                       int32_t* exit_iters, float* stage_k, void* workspace, size_t workspace_bytes,
                                       int32_t activation) {
  if (!dyn || !w) return FIODE_EINVAL;
  if (activation != FIODE_ACT_RELU && activation != FIODE_ACT_GROUPSORT) return FIODE_EINVAL;
  if (dyn->n_hidden != C || dyn->mlp_size != M || dyn->x_dim != FIODE_X) return FIODE_ESHAPE;
  if (dyn->qp_max_iter < 1 || dyn->qp_max_iter > 32) return FIODE_EINVAL;
  if (batch <= 0 || batch > FIODE_ODEINT_MAX_BATCH) return FIODE_EINVAL;
  const int n_steps = obx_steps(t0, t1, step_size);
  if (n_steps < 0) return FIODE_EINVAL;
  if ((long long)batch * n_steps > (1LL << 30)) return FIODE_EINVAL;
  if (!x_feat || !states || !g_y || !g_h0 || !g_x_feat || !workspace) return FIODE_EINVAL;
  if (!w->Q1 || !w->b1 || !w->Qx || !w->bx || !w->Q2 || !w->b2 || !w->Q3 || !w->b3) return FIODE_EINVAL;
  if (workspace_bytes < fiode_odeint_backward_x_workspace_bytes(batch, t0, t1, step_size)) return FIODE_EWORKSPACE;
  const ObxLayout L = obx_layout(batch, n_steps);
  char* ws = static_cast<char*>(workspace);
  ObxArgs a{};
  a.B = batch; a.n_steps = n_steps; a.N = batch * n_steps;
  a.t0 = (float)t0; a.t1 = (float)t1; a.hs = (float)step_size;
  a.d.alpha_1 = dyn->alpha_1; a.d.alpha_2 = dyn->alpha_2; a.d.sigma_1 = dyn->sigma_1;
  a.d.tol = dyn->qp_tol; a.d.scale_nominal = dyn->scale_nominal; a.d.max_iter = dyn->qp_max_iter;
  a.x_feat = x_feat; a.ys = states;
  a.Q1 = w->Q1; a.b1 = w->b1; a.Qx = w->Qx; a.bx = w->bx; a.Q2 = w->Q2; a.b2 = w->b2; a.Q3 = w->Q3; a.b3 = w->b3;
  a.g_y = g_y; a.g_h0 = g_h0; a.g_x = g_x_feat;
  a.words = reinterpret_cast<uint32_t*>(ws + L.words);
  a.Kx = exit_iters ? exit_iters : reinterpret_cast<int32_t*>(ws + L.Kx);
  a.u = reinterpret_cast<float*>(ws + L.u);
  a.k = stage_k ? stage_k : reinterpret_cast<float*>(ws + L.k);
  a.ft = reinterpret_cast<float*>(ws + L.ft);
  a.g_u = reinterpret_cast<float*>(ws + L.g_u);
  const bool gs = activation == FIODE_ACT_GROUPSORT;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_obx_static, dim3(batch), dim3(128), 0, st, a);
  FIODE_HIP_CHECK(hipGetLastError());
  // replay: stage s of every step needs stages < s of its own step only
  const int rtiles = (a.N + 31) / 32;
  const dim3 fgrid((rtiles + FIODE_WAVES - 1) / FIODE_WAVES);
  const size_t flds = (size_t)(M + 32) * LDQ * sizeof(float);
  for (int s = 0; s < 4; ++s) {
    if (gs) hipLaunchKernelGGL(k_obx_stage<GROUPSORT>, fgrid, dim3(256), flds, st, a, s);
    else hipLaunchKernelGGL(k_obx_stage<RELU>, fgrid, dim3(256), flds, st, a, s);
    FIODE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_obx_final, dim3((a.N + 255) / 256), dim3(256), 0, st, a, s);
    FIODE_HIP_CHECK(hipGetLastError());
  }
  // sweep: one wave per tile; the tiles are independent latency chains, so they spread over the
  // compute units first (one wave per workgroup up to 256 tiles) and share a workgroup's weight
  // images only past that
  const int btiles = (batch + 31) / 32;
  const int wpb = btiles <= 256 ? 1 : (btiles <= 512 ? 2 : 4);
  const dim3 bgrid((btiles + wpb - 1) / wpb);
  const size_t blds = ((size_t)(M + 32) * LDQ + (size_t)M * C) * sizeof(float);
  if (gs) hipLaunchKernelGGL(k_ode_bwd_x<GROUPSORT>, bgrid, dim3(64 * wpb), blds, st, a);
  else hipLaunchKernelGGL(k_ode_bwd_x<RELU>, bgrid, dim3(64 * wpb), blds, st, a);
  FIODE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_obx_gx, dim3((unsigned)(((size_t)batch * FIODE_X + 255) / 256)), dim3(256), 0, st, a);
  FIODE_HIP_CHECK(hipGetLastError());
  return FIODE_OK;
}

extern "C" size_t fiode_odeint_dopri5_backward_x_workspace_bytes(int32_t batch, int32_t n_steps) {
  if (batch <= 0 || batch > FIODE_ODEINT_MAX_BATCH || n_steps < 1 || n_steps > FIODE_ODEINT_LOG_MAX_STEPS) return 256;
  return dpx_layout(batch, n_steps).total;
}

extern "C" int fiode_odeint_dopri5_backward_x(void* stream, const fiode_dyn_config* dyn, const fiode_dyn_weights* w,
                                              int32_t batch, int32_t n_steps, double t1, const double* step_times,
                                              const float* step_states, const float* x_feat, const float* g_y,
                                              float* g_h0, float* g_x_feat, int32_t* exit_iters, float* stage_k,
                                              void* workspace, size_t workspace_bytes, int32_t activation) {
  if (!dyn || !w) return FIODE_EINVAL;
  if (activation != FIODE_ACT_RELU && activation != FIODE_ACT_GROUPSORT) return FIODE_EINVAL;
  if (dyn->n_hidden != C || dyn->mlp_size != M || dyn->x_dim != FIODE_X) return FIODE_ESHAPE;
  if (dyn->qp_max_iter < 1 || dyn->qp_max_iter > 32) return FIODE_EINVAL;
  if (batch <= 0 || batch > FIODE_ODEINT_MAX_BATCH) return FIODE_EINVAL;
  if (n_steps < 1 || n_steps > FIODE_ODEINT_LOG_MAX_STEPS) return FIODE_EINVAL;
  if (!(t1 == t1)) return FIODE_EINVAL;
  if (!step_times || !step_states || !x_feat || !g_y || !g_h0 || !g_x_feat || !workspace) return FIODE_EINVAL;
  if (!w->Q1 || !w->b1 || !w->Qx || !w->bx || !w->Q2 || !w->b2 || !w->Q3 || !w->b3) return FIODE_EINVAL;
  if (workspace_bytes < fiode_odeint_dopri5_backward_x_workspace_bytes(batch, n_steps)) return FIODE_EWORKSPACE;
  const DpxLayout L = dpx_layout(batch, n_steps);
  char* ws = static_cast<char*>(workspace);
  DpxArgs a{};
  a.B = batch; a.n_steps = n_steps; a.t1 = t1;
  a.d.alpha_1 = dyn->alpha_1; a.d.alpha_2 = dyn->alpha_2; a.d.sigma_1 = dyn->sigma_1;
  a.d.tol = dyn->qp_tol; a.d.scale_nominal = dyn->scale_nominal; a.d.max_iter = dyn->qp_max_iter;
  a.times = step_times; a.x_feat = x_feat; a.ys = step_states;
  a.Q1 = w->Q1; a.b1 = w->b1; a.Qx = w->Qx; a.bx = w->bx; a.Q2 = w->Q2; a.b2 = w->b2; a.Q3 = w->Q3; a.b3 = w->b3;
  a.g_y = g_y; a.g_h0 = g_h0;
  a.words = reinterpret_cast<uint32_t*>(ws + L.words);
  a.Kx = exit_iters ? exit_iters : reinterpret_cast<int32_t*>(ws + L.Kx);
  a.u = reinterpret_cast<float*>(ws + L.u);
  a.k = stage_k ? stage_k : reinterpret_cast<float*>(ws + L.k);
  a.ft = reinterpret_cast<float*>(ws + L.ft);
  a.g_u = reinterpret_cast<float*>(ws + L.g_u);
  ObxArgs gx{};                                  // k_obx_gx reads B, g_u, Qx and writes g_x
  gx.B = batch; gx.g_u = a.g_u; gx.Qx = w->Qx; gx.g_x = g_x_feat;
  const bool gs = activation == FIODE_ACT_GROUPSORT;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_dpx_static, dim3(batch), dim3(128), 0, st, a);
  FIODE_HIP_CHECK(hipGetLastError());
  // replay: stage s of every step needs stages < s of its own step only; k7 for the last step alone
  const size_t flds = (size_t)(M + 32) * LDQ * sizeof(float);
  for (int s = 0; s < 7; ++s) {
    const int n0 = s < 6 ? 0 : n_steps - 1;
    const int N = s < 6 ? n_steps * batch : batch;
    const int rtiles = (N + 31) / 32;
    const dim3 fgrid((rtiles + FIODE_WAVES - 1) / FIODE_WAVES);
    if (gs) hipLaunchKernelGGL(k_dpx_stage<GROUPSORT>, fgrid, dim3(256), flds, st, a, s, n0, N);
    else hipLaunchKernelGGL(k_dpx_stage<RELU>, fgrid, dim3(256), flds, st, a, s, n0, N);
    FIODE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_dpx_final, dim3((N + 255) / 256), dim3(256), 0, st, a, s, n0, N);
    FIODE_HIP_CHECK(hipGetLastError());
  }
  // sweep: one wave per tile, spread over the compute units first (as fiode_odeint_backward_x)
  const int btiles = (batch + 31) / 32;
  const int wpb = btiles <= 256 ? 1 : (btiles <= 512 ? 2 : 4);
  const dim3 bgrid((btiles + wpb - 1) / wpb);
  const size_t blds = ((size_t)(M + 32) * LDQ + (size_t)M * C) * sizeof(float);
  if (gs) hipLaunchKernelGGL(k_ode_bwd_x_dp<GROUPSORT>, bgrid, dim3(64 * wpb), blds, st, a);
  else hipLaunchKernelGGL(k_ode_bwd_x_dp<RELU>, bgrid, dim3(64 * wpb), blds, st, a);
  FIODE_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_obx_gx, dim3((unsigned)(((size_t)batch * FIODE_X + 255) / 256)), dim3(256), 0, st, gx);
  FIODE_HIP_CHECK(hipGetLastError());
  return FIODE_OK;
}
