// CROWN certification on the decision-boundary grid (robustness/certify_crown.py:113-158), gfx950.
//
// Per image and per batch of grid rows (the partition of cert.hip's batch_of):
//   (lb, ub)     = backward CROWN bounds of the 10 -> 128 -> 128 -> 10 ReLU MLP over the L-inf box of
//                  half-width 1/T around each grid row (Zhang et al. 2018, adaptive lower slope; the
//                  algebra is written out in DESIGN.md section 7e), with scale_nominal followed by
//                  ibp_sigmoid (classification.py:175-181);
//   (f_lb, f_ub) = ibp_cbf_qp (classification.py:208-242, upper=False): 10 sub-problems per row for each
//                  of two FastBarrierProjectionNoUpper calls, each with its own batch-global exit;
//   violation    = -f_lb[label] + max_{wrong} f_ub + kappa      (certify_crown.py:29-34, 143-150)
//   out[b]       = max over the batch's rows.
// Four kernels per batch, enqueued back to back with no host synchronisation:
//   k_crown_bounds  the bounds, f32 MFMA against the W2 image resident in LDS -> [rows][20] workspace
//   k_crown_qp1     every sub-problem's convergence mask, ANDed into two words per batch
//   k_crown_qp2     both solves to their exits, the diagonal, the violation, the batch maximum
//   k_crown_fin     decode; the device-side stop flag.
// k_crown_bounds (8 waves, two per SIMD; each MFMA phase in two passes of 64 output units so that the live
// accumulators fit), one wave = two grid rows (rho = 0, 1) per trip:
//   layer 1   z1 = W1 eta + u, r1 = eps |W1| 1 (exact interval), relaxation (s1, t1, alpha1) -> LDS
//   layer 2   D[(rho, c)][j] = sum_k d_k(rho) B[k][c] W2[j][k] twice, against W2 with d = (s1 + alpha1) / 2
//             and against |W2| with d = (s1 - alpha1) / 2, B = [W1 | z1] (and a twelfth column t1 / 2 with
//             d = 1 in both; 12 of 16 columns per row): their sum and difference are the upper and lower
//             coefficient rows through W1 and z1, and W2+ t1 and W2- t1.  The
//             (rho, c) operand is formed per lane (one multiply per MFMA operand value); column j of the
//             accumulator is on the lane, so |.|_1 over c is a sum over registers and one half swap.
//   outputs   Q^T[k][(rho, i)] = sum_j W2[j][k] Lambda[(rho, i)][j], W2 read transposed (A operand), the
//             Lambda operand formed per lane from W3 and (s2, alpha2); then R = Q+ s1 + Q- alpha1 (or
//             swapped) in registers, which is already the B operand of (R W1)^T = W1^T R (the accumulator
//             of one product as the next one's operand, as mlp12_tile); once for the lower rows, once for
//             the upper ones.
// Nothing of size [rows][128][128] exists; what leaves the chip is [batch rows][20] floats.
// GroupSort dynamics (fiode_certify_crown_act): k_crown_fold_gs once per call and k_crown_bounds_gs in
// k_crown_bounds' place -- the same relaxation on the 64 pair differences of each hidden layer; see there.
#include "common.h"
#include "tile.h"
#include "../../include/fiode.h"

namespace {
using namespace fiode_tile;

constexpr int MAXT = 64;
constexpr int NW = 8;                 // waves per workgroup of k_crown_bounds: two per SIMD
constexpr int W1ROWS = 16;            // rows of the W1^T and W3 images (rows >= C zero)
constexpr int TABF = 68;              // eta table, padded to a multiple of 4 floats
constexpr int WAVEF = 9 * 2 * M;      // per-wave arrays [2][M]: dP dM z1 th s1 a1 s2 a2 t2

struct CrownArgs {
  uint32_t G, lo, hi;       // grid rows; this batch's rows [lo, hi)
  int b, nb, label, T, stop_on_violation, own_flag;
  float eps, two_eps, kappa;
  float etab[MAXT + 1];     // float32(v / T), v = 0..T (double quotient, host-rounded)
  DynScalars d;
  const float* x_feat;
  const uint8_t* grid;
  const float *Q1, *b1, *Qx, *bx, *Q2, *b2, *Q3, *b3;
  float* u;                 // [M] Qx x + bx + b1
  float* r1;                // [M] eps sum_c |W1[k][c]|
  float* lbub;              // [max batch rows][2][C]
  uint32_t* words;          // [nb][2] QP exit AND words (lower-bound call, upper-bound call)
  uint32_t* keys;           // [nb] order-preserving max key
  int32_t* stop;            // the caller's flag, or a word of the workspace
  float* out;
  int32_t* exit_iters;
  fiode_crown_debug dbg;
  float* gs;                // GroupSort only: the folded images (GS_* offsets below), else NULL
};

// ---- GroupSort (pairs (k, k + H)): d = z[:H] - z[H:], r = relu(d), a = S z + [I; -I] r.
// The slope-carrying units are the H pair differences of each layer; the skip path S z is affine in
// eta and is folded once per call by k_crown_fold_gs into these images (floats from CrownArgs::gs):
//   d1 = A1 eta + c1                         A1 = Delta W1, c1 = Delta u, r1 = eps |A1| 1
//   d2 = F2 eta + f2 + M2 r1                 M2 = Delta N(W2), [F2 | f2] = Delta (P(W2) [W1 | u] + [0 | b2])
//   o  = G3 eta + g3 + H3 r1 + N3 r2         H3 = P(W3) N(W2), N3 = N(W3), [G3 | g3] = P(W3) E2 + [0 | b3]
// with E2 = P(W2) [W1 | u] + [0 | b2].  A1, F2 are stored transposed ([c][k]) as the kernel reads them.
constexpr int H = M / 2;
constexpr int LDH = H + 4;            // padded LDS row stride (floats) of the 64-wide images
constexpr int GS_A1 = 0;              // [C][H]
constexpr int GS_C1 = GS_A1 + C * H;  // [H]
constexpr int GS_R1 = GS_C1 + H;      // [H]
constexpr int GS_M2 = GS_R1 + H;      // [H][H]
constexpr int GS_F2 = GS_M2 + H * H;  // [C][H]
constexpr int GS_F2C = GS_F2 + C * H; // [H]
constexpr int GS_H3 = GS_F2C + H;     // [C][H]
constexpr int GS_N3 = GS_H3 + C * H;  // [C][H]
constexpr int GS_G3 = GS_N3 + C * H;  // [C][C]
constexpr int GS_G3C = GS_G3 + 112;   // [C]
constexpr int GS_FLOATS = GS_G3C + 16;
constexpr int WAVEF_GS = 10 * 2 * H + 2 * W1ROWS;   // per-wave arrays [2][H]: dP dM d1 th s1 a1 s2 a2 t2 zc; oc [2][16]

__device__ __forceinline__ uint32_t fkey(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// eta row as fiode_certify reads it: float32(v / T) with the label's column swapped with column 0
__device__ __forceinline__ void eta_row(const CrownArgs& a, const float* tab, uint32_t r, float (&h)[C]) {
  const uint8_t* g = a.grid + (size_t)r * C;
  float v[C];
#pragma unroll
  for (int j = 0; j < C; ++j) v[j] = tab[g[j]];
  float v0 = v[0], vl = v[0];
#pragma unroll
  for (int j = 0; j < C; ++j) vl = (j == a.label) ? v[j] : vl;
#pragma unroll
  for (int j = 0; j < C; ++j) h[j] = (j == 0) ? vl : ((j == a.label) ? v0 : v[j]);
}

// ReLU relaxation on [l, u]: upper line s z + t, lower line alpha z (alpha = 1 iff u > -l; a tie gives 0)
__device__ __forceinline__ void relax(float l, float u, float& s, float& t, float& al) {
  if (l >= 0.f) {
    s = 1.f; al = 1.f; t = 0.f;
  } else if (u <= 0.f) {
    s = 0.f; al = 0.f; t = 0.f;
  } else {
    s = u / (u - l);
    t = -s * l;
    al = (u > -l) ? 1.f : 0.f;
  }
}

// LDS writes of one phase are read by other lanes of the same wave in the next
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void k_crown_prep(CrownArgs a) {
  if (a.own_flag) {
    if (threadIdx.x == 0) *a.stop = 0;
  } else if (*a.stop != 0) {
    return;
  }
  const int i = threadIdx.x;
  if (i < M) {
    float s = 0.f, r = 0.f;
#pragma unroll
    for (int c = 0; c < FIODE_X; ++c) s = __fmaf_rn(a.Qx[i * FIODE_X + c], a.x_feat[c], s);
#pragma unroll
    for (int c = 0; c < C; ++c) r = r + fabsf(a.Q1[i * C + c]);
    a.u[i] = (s + a.bx[i]) + a.b1[i];
    a.r1[i] = a.eps * r;
  }
  for (int b = i; b < a.nb; b += blockDim.x) {
    a.words[2 * b] = 0xFFFFFFFFu;
    a.words[2 * b + 1] = 0xFFFFFFFFu;
    a.keys[b] = 0u;
  }
}

__global__ __launch_bounds__(64 * NW) void k_crown_bounds(CrownArgs a) {
  if (*a.stop != 0) return;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Q2s = smem;
  float* W1T = Q2s + M * LDQ;
  float* Q3s = W1T + W1ROWS * LDQ;
  float* tab = Q3s + W1ROWS * LDQ;
  float* ones = tab + TABF;                         // [M]: the t1 column takes no slope factor
  float* wbase = ones + M;
  load_weight_images(a.Q2, a.Q3, Q2s, Q3s, W1ROWS);
  for (int e = threadIdx.x; e < W1ROWS * M; e += blockDim.x) {
    const int c = e >> 7, k = e & (M - 1);
    W1T[c * LDQ + k] = c < C ? a.Q1[k * C + c] : 0.f;
  }
  for (int v = threadIdx.x; v < TABF; v += blockDim.x) tab[v] = v <= a.T ? a.etab[v] : 0.f;
  for (int v = threadIdx.x; v < M; v += blockDim.x) ones[v] = 1.f;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
  float* wl = wbase + wave * WAVEF;
  float *dP = wl, *dM = wl + 2 * M, *z1 = wl + 4 * M, *th = wl + 6 * M, *s1 = wl + 8 * M, *a1 = wl + 10 * M,
        *s2 = wl + 12 * M, *a2 = wl + 14 * M, *t2 = wl + 16 * M;
  const uint32_t rows = a.hi - a.lo;
  const uint32_t ntiles = (rows + 1) / 2;
  const int rho = col >> 4, ci = col & 15;          // (row of the pair, column c / output i) of this lane
  for (uint32_t tile = blockIdx.x * NW + wave; tile < ntiles; tile += gridDim.x * NW) {
    // ---- layer 1 (exact): lane = (row `half`, units col + 32 m) ---------------------------------
    {
      const uint32_t row = a.lo + 2 * tile + half;
      const uint32_t rr = row < a.hi ? row : a.hi - 1;
      float h[C];
      eta_row(a, tab, rr, h);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int k = 32 * m + col;
        float z = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) z = __fmaf_rn(W1T[c * LDQ + k], h[c], z);
        z = z + a.u[k];
        const float r = a.r1[k];
        float s, t, al;
        relax(z - r, z + r, s, t, al);
        const int o = half * M + k;
        dP[o] = (s + al) * 0.5f;
        dM[o] = (s - al) * 0.5f;
        z1[o] = z;
        th[o] = t * 0.5f;
        s1[o] = s;
        a1[o] = al;
      }
    }
    wave_lds_sync();
    // ---- layer 2 pre-activation bounds -----------------------------------------------------------
    {
      // its slope factors: (s1 +- alpha1) / 2 for the W1 and z1 columns; the t1 column is W2+- t1 itself
      const float* pd = ci == C + 1 ? ones : dP + rho * M;
      const float* md = ci == C + 1 ? ones : dM + rho * M;
      // the B column of this lane: W1[:, c] (c < 10), z1 (10), t1 / 2 (11), zero rows of the image (12..15)
      const float* bm = ci == C ? z1 + rho * M : (ci == C + 1 ? th + rho * M : W1T + ci * LDQ);
      // two passes of 64 units j each: 4 accumulator tiles live (64 registers), so that two waves per
      // SIMD fit the register file; the lane's operand is formed once per pass
#pragma unroll 1
      for (int np = 0; np < 2; ++np) {
        f32x16 P[2], N[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          P[nt] = f16_zero();
          N[nt] = f16_zero();
        }
        const float* q2 = Q2s + (64 * np + col) * LDQ;
#pragma unroll 1
        for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int k0 = 32 * kb + 8 * g + 4 * half;
            const f32x4 dp = *reinterpret_cast<const f32x4*>(pd + k0);
            const f32x4 dm = *reinterpret_cast<const f32x4*>(md + k0);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bm + k0);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
              const f32x4 q = *reinterpret_cast<const f32x4*>(q2 + 32 * nt * LDQ + k0);
#pragma unroll
              for (int t = 0; t < 4; ++t) {
                P[nt] = mfma32(dp[t] * bv[t], q[t], P[nt]);
                N[nt] = mfma32(dm[t] * bv[t], fabsf(q[t]), N[nt]);
              }
            }
            __builtin_amdgcn_sched_barrier(0);   // as mlp12_tile: bound the LDS-read hoisting window
          }
        }
        // registers 8 r .. 8 r + 7 of a lane are row r's columns c = {0..3, 8..11} (half 0) / {4..7, 12..15}
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          const int j = 64 * np + 32 * nt + col;
          const float bj = a.b2[j];
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            float sU = 0.f, sL = 0.f;
#pragma unroll
            for (int e = 0; e < 6; ++e) {
              const float p = P[nt][8 * r + e], n = N[nt][8 * r + e];      // c = 12, 13 (half 1): exact zeros
              sU = sU + fabsf(p + n);
              sL = sL + fabsf(p - n);
            }
            const float p6 = P[nt][8 * r + 6], n6 = N[nt][8 * r + 6], p7 = P[nt][8 * r + 7], n7 = N[nt][8 * r + 7];
            float zU = half == 0 ? (p6 + n6) + (p7 + n7) : 0.f;
            float zL = half == 0 ? (p6 - n6) + (p7 - n7) : 0.f;
            sU = sU + shfl_xor32(sU);
            sL = sL + shfl_xor32(sL);
            zU = zU + shfl_xor32(zU);
            zL = zL + shfl_xor32(zL);
            const float u2 = (zU + a.eps * sU) + bj;
            const float l2 = (zL - a.eps * sL) + bj;
            float s, t, al;
            relax(l2, u2, s, t, al);
            if (half == r) {
              s2[r * M + j] = s;
              a2[r * M + j] = al;
              t2[r * M + j] = t;
              const uint32_t row = a.lo + 2 * tile + r;
              if (row < a.hi) {
                if (a.dbg.l2) a.dbg.l2[(size_t)row * M + j] = l2;
                if (a.dbg.u2) a.dbg.u2[(size_t)row * M + j] = u2;
              }
            }
          }
        }
      }
    }
    wave_lds_sync();
    // ---- the ten outputs: lower rows (lu = 0), then upper rows (lu = 1); lane = (rho, i = ci) -----
    const uint32_t orow = a.lo + 2 * tile + rho;
#pragma unroll 1
    for (int lu = 0; lu < 2; ++lu) {
      f32x16 D2 = f16_zero();
      float acc = 0.f;
      // two passes of 64 units k each (Qt: 2 accumulator tiles live; the Lambda operand is formed again in
      // the second pass, its bias terms counted in the first only)
#pragma unroll 1
      for (int kp = 0; kp < 2; ++kp) {
        f32x16 Qt[2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) Qt[mb] = f16_zero();
        const float w0 = kp == 0 ? 1.f : 0.f;
        const float* q2t = Q2s + 64 * kp + col;
#pragma unroll 1
        for (int jb = 0; jb < 4; ++jb) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int j0 = 32 * jb + 8 * g + 4 * half;
            const f32x4 w3 = *reinterpret_cast<const f32x4*>(Q3s + ci * LDQ + j0);
            const f32x4 sv = *reinterpret_cast<const f32x4*>(s2 + rho * M + j0);
            const f32x4 av = *reinterpret_cast<const f32x4*>(a2 + rho * M + j0);
            const f32x4 tv = *reinterpret_cast<const f32x4*>(t2 + rho * M + j0);
            const float bv[4] = {a.b2[j0], a.b2[j0 + 1], a.b2[j0 + 2], a.b2[j0 + 3]};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const float wp = fmaxf(w3[t], 0.f), wm = fminf(w3[t], 0.f);
              const float lam = lu ? wp * sv[t] + wm * av[t] : wp * av[t] + wm * sv[t];
              acc = acc + w0 * (lam * bv[t]);
              acc = acc + w0 * ((lu ? wp : wm) * tv[t]);
#pragma unroll
              for (int mb = 0; mb < 2; ++mb) Qt[mb] = mfma32(q2t[(j0 + t) * LDQ + 32 * mb], lam, Qt[mb]);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        // Qt[mb][r] = Q[(rho, i)][k = 64 kp + 32 mb + acc_row(r, half)]
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int k0 = 64 * kp + 32 * mb + 8 * g + 4 * half;
            const f32x4 sv = *reinterpret_cast<const f32x4*>(s1 + rho * M + k0);
            const f32x4 av = *reinterpret_cast<const f32x4*>(a1 + rho * M + k0);
            const f32x4 zv = *reinterpret_cast<const f32x4*>(z1 + rho * M + k0);
            const f32x4 tv = *reinterpret_cast<const f32x4*>(th + rho * M + k0);
            const f32x4 w1 = col < W1ROWS ? *reinterpret_cast<const f32x4*>(W1T + col * LDQ + k0)
                                          : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const float q = Qt[mb][4 * g + t];
              const float qp = fmaxf(q, 0.f), qm = fminf(q, 0.f);
              const float R = lu ? qp * sv[t] + qm * av[t] : qp * av[t] + qm * sv[t];
              acc = acc + R * zv[t];
              acc = acc + (lu ? qp : qm) * (2.0f * tv[t]);
              D2 = mfma32(w1[t], R, D2);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      // D2[r] = (R W1)[(rho, i)][c = acc_row(r, half)]: c = 0..3, 8, 9 on half 0, 4..7 on half 1
      float l1 = ((fabsf(D2[0]) + fabsf(D2[1])) + fabsf(D2[2])) + fabsf(D2[3]);
      if (half == 0) l1 = (l1 + fabsf(D2[4])) + fabsf(D2[5]);
      l1 = l1 + shfl_xor32(l1);
      acc = acc + shfl_xor32(acc);
      if (half == 0 && ci < C && orow < a.hi) {
        const float bound = (lu ? acc + a.eps * l1 : acc - a.eps * l1) + a.b3[ci];
        a.lbub[(size_t)(orow - a.lo) * (2 * C) + lu * C + ci] = bound;
        float* dst = lu ? a.dbg.ub : a.dbg.lb;
        if (dst) dst[(size_t)orow * C + ci] = bound;
      }
    }
    wave_lds_sync();    // the next trip overwrites the arrays this one read
  }
}

// The folded GroupSort images, once per call (one workgroup; W2, W1 | u and W3 staged in LDS, E2 kept there).
__global__ __launch_bounds__(256) void k_crown_fold_gs(CrownArgs a) {
  if (*a.stop != 0) return;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Q2s = smem;
  float* W1T = Q2s + M * LDQ;                       // rows c < C: W1[:, c]; row C: u
  float* Q3s = W1T + W1ROWS * LDQ;
  float* E2s = Q3s + W1ROWS * LDQ;                  // [C + 1][LDQ]: rows c < C: E2[:, c]; row C: P(W2) u + b2
  load_weight_images(a.Q2, a.Q3, Q2s, Q3s, W1ROWS);
  for (int e = threadIdx.x; e < W1ROWS * M; e += blockDim.x) {
    const int c = e >> 7, k = e & (M - 1);
    W1T[c * LDQ + k] = c < C ? a.Q1[k * C + c] : (c == C ? a.u[k] : 0.f);
  }
  __syncthreads();
  float* g = a.gs;
  for (int e = threadIdx.x; e < (C + 1) * M; e += blockDim.x) {
    const int c = e >> 7, j = e & (M - 1);
    float s = 0.f;
    for (int k = 0; k < M; ++k) s = __fmaf_rn(Q2s[j * LDQ + (k ^ H)], W1T[c * LDQ + k], s);
    E2s[c * LDQ + j] = c == C ? s + a.b2[j] : s;
  }
  for (int e = threadIdx.x; e < C * H; e += blockDim.x) {
    const int i = e >> 6, k = e & (H - 1);
    float s = 0.f;
    for (int j = 0; j < M; ++j) s = __fmaf_rn(Q3s[i * LDQ + (j ^ H)], Q2s[j * LDQ + k] - Q2s[j * LDQ + k + H], s);
    g[GS_H3 + e] = s;
    g[GS_N3 + e] = Q3s[i * LDQ + k] - Q3s[i * LDQ + k + H];
    g[GS_A1 + e] = W1T[i * LDQ + k] - W1T[i * LDQ + k + H];
  }
  for (int e = threadIdx.x; e < H * H; e += blockDim.x) {
    const int j = e >> 6, k = e & (H - 1);
    g[GS_M2 + e] = (Q2s[j * LDQ + k] - Q2s[j * LDQ + k + H]) - (Q2s[(j + H) * LDQ + k] - Q2s[(j + H) * LDQ + k + H]);
  }
  if (threadIdx.x < H) {
    const int k = threadIdx.x;
    float r = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) r = r + fabsf(W1T[c * LDQ + k] - W1T[c * LDQ + k + H]);
    g[GS_C1 + k] = W1T[C * LDQ + k] - W1T[C * LDQ + k + H];
    g[GS_R1 + k] = a.eps * r;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < (C + 1) * H; e += blockDim.x) {
    const int c = e >> 6, j = e & (H - 1);
    g[c < C ? GS_F2 + e : GS_F2C + j] = E2s[c * LDQ + j] - E2s[c * LDQ + j + H];
  }
  for (int e = threadIdx.x; e < (C + 1) * C; e += blockDim.x) {
    const int c = e / C, i = e % C;
    float s = 0.f;
    for (int j = 0; j < M; ++j) s = __fmaf_rn(Q3s[i * LDQ + (j ^ H)], E2s[c * LDQ + j], s);
    if (c < C) g[GS_G3 + i * C + c] = s;
    else g[GS_G3C + i] = s + a.b3[i];
  }
}

// k_crown_bounds for GroupSort: the same three phases on the H pair differences of each layer (one pass
// of 64 units where ReLU takes two of 64), against the folded images.  The skip terms enter as the
// initial values of the accumulators: F2 and its centre F2 eta + f2 under the layer-2 products, H3 under
// K^T = H3^T + M2^T Lambda^T, G3 under the coefficient rows (which also take Lambda F2, one more MFMA per
// Lambda operand); the constants take Lambda (F2 eta + f2) where ReLU has Lambda b2, and G3 eta + g3 for b3.
__global__ __launch_bounds__(64 * NW) void k_crown_bounds_gs(CrownArgs a) {
  if (*a.stop != 0) return;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* M2s = smem;                                // [H][LDH]
  float* A1T = M2s + H * LDH;                       // [16][LDH] each, rows >= C zero
  float* F2T = A1T + W1ROWS * LDH;
  float* H3s = F2T + W1ROWS * LDH;
  float* N3s = H3s + W1ROWS * LDH;
  float* G3s = N3s + W1ROWS * LDH;                  // [16][16], zero outside [C][C]
  float* tab = G3s + W1ROWS * W1ROWS;
  float* ones = tab + TABF;                         // [H]
  float* wbase = ones + H;
  const float* g = a.gs;
  for (int e = threadIdx.x; e < H * H; e += blockDim.x) M2s[(e >> 6) * LDH + (e & (H - 1))] = g[GS_M2 + e];
  for (int e = threadIdx.x; e < W1ROWS * H; e += blockDim.x) {
    const int c = e >> 6, o = c * LDH + (e & (H - 1));
    const bool in = c < C;
    A1T[o] = in ? g[GS_A1 + e] : 0.f;
    F2T[o] = in ? g[GS_F2 + e] : 0.f;
    H3s[o] = in ? g[GS_H3 + e] : 0.f;
    N3s[o] = in ? g[GS_N3 + e] : 0.f;
  }
  for (int e = threadIdx.x; e < W1ROWS * W1ROWS; e += blockDim.x) {
    const int i = e >> 4, c = e & 15;
    G3s[e] = (i < C && c < C) ? g[GS_G3 + i * C + c] : 0.f;
  }
  for (int v = threadIdx.x; v < TABF; v += blockDim.x) tab[v] = v <= a.T ? a.etab[v] : 0.f;
  for (int v = threadIdx.x; v < H; v += blockDim.x) ones[v] = 1.f;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
  float* wl = wbase + wave * WAVEF_GS;
  float *dP = wl, *dM = wl + 2 * H, *d1 = wl + 4 * H, *th = wl + 6 * H, *s1 = wl + 8 * H, *a1 = wl + 10 * H,
        *s2 = wl + 12 * H, *a2 = wl + 14 * H, *t2 = wl + 16 * H, *zc = wl + 18 * H, *oc = wl + 20 * H;
  const uint32_t rows = a.hi - a.lo;
  const uint32_t ntiles = (rows + 1) / 2;
  const int rho = col >> 4, ci = col & 15;
  for (uint32_t tile = blockIdx.x * NW + wave; tile < ntiles; tile += gridDim.x * NW) {
    // ---- layer 1 (exact): lane = (row `half`, pairs col + 32 m); the skip centres of d2 and of the outputs
    {
      const uint32_t row = a.lo + 2 * tile + half;
      const uint32_t rr = row < a.hi ? row : a.hi - 1;
      float h[C];
      eta_row(a, tab, rr, h);
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int k = 32 * m + col;
        float d = 0.f, z = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          d = __fmaf_rn(A1T[c * LDH + k], h[c], d);
          z = __fmaf_rn(F2T[c * LDH + k], h[c], z);
        }
        d = d + g[GS_C1 + k];
        const float r = g[GS_R1 + k];
        float s, t, al;
        relax(d - r, d + r, s, t, al);
        const int o = half * H + k;
        dP[o] = (s + al) * 0.5f;
        dM[o] = (s - al) * 0.5f;
        d1[o] = d;
        th[o] = t * 0.5f;
        s1[o] = s;
        a1[o] = al;
        zc[o] = z + g[GS_F2C + k];
      }
      if (col < W1ROWS) {
        float z = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) z = __fmaf_rn(G3s[col * W1ROWS + c], h[c], z);
        oc[half * W1ROWS + col] = col < C ? z + g[GS_G3C + col] : 0.f;
      }
    }
    wave_lds_sync();
    // ---- bounds of the layer-2 pair differences d2 ---------------------------------------------------
    {
      const float* pd = ci == C + 1 ? ones : dP + rho * H;
      const float* md = ci == C + 1 ? ones : dM + rho * H;
      const float* bm = ci == C ? d1 + rho * H : (ci == C + 1 ? th + rho * H : A1T + ci * LDH);
      f32x16 P[2], N[2];
      // registers 8 r .. 8 r + 7 of a lane are row r's columns c = {0..3, 8..11} (half 0) / {4..7, 12..15}:
      // the skip coefficients F2[j][c] (c < 10) and the skip centre (c = 10) start the sums
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        N[nt] = f16_zero();
        const int j = 32 * nt + col;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
          for (int e = 0; e < 6; ++e) P[nt][8 * r + e] = F2T[((e & 3) + 8 * (e >> 2) + 4 * half) * LDH + j];
          P[nt][8 * r + 6] = half == 0 ? zc[r * H + j] : 0.f;
          P[nt][8 * r + 7] = 0.f;
        }
      }
      const float* q2 = M2s + col * LDH;
#pragma unroll 1
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int k0 = 32 * kb + 8 * gq + 4 * half;
          const f32x4 dp = *reinterpret_cast<const f32x4*>(pd + k0);
          const f32x4 dm = *reinterpret_cast<const f32x4*>(md + k0);
          const f32x4 bv = *reinterpret_cast<const f32x4*>(bm + k0);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(q2 + 32 * nt * LDH + k0);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              P[nt] = mfma32(dp[t] * bv[t], q[t], P[nt]);
              N[nt] = mfma32(dm[t] * bv[t], fabsf(q[t]), N[nt]);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int j = 32 * nt + col;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          float sU = 0.f, sL = 0.f;
#pragma unroll
          for (int e = 0; e < 6; ++e) {
            const float p = P[nt][8 * r + e], n = N[nt][8 * r + e];
            sU = sU + fabsf(p + n);
            sL = sL + fabsf(p - n);
          }
          const float p6 = P[nt][8 * r + 6], n6 = N[nt][8 * r + 6], p7 = P[nt][8 * r + 7], n7 = N[nt][8 * r + 7];
          float zU = half == 0 ? (p6 + n6) + (p7 + n7) : 0.f;
          float zL = half == 0 ? (p6 - n6) + (p7 - n7) : 0.f;
          sU = sU + shfl_xor32(sU);
          sL = sL + shfl_xor32(sL);
          zU = zU + shfl_xor32(zU);
          zL = zL + shfl_xor32(zL);
          const float u2 = zU + a.eps * sU;
          const float l2 = zL - a.eps * sL;
          float s, t, al;
          relax(l2, u2, s, t, al);
          if (half == r) {
            s2[r * H + j] = s;
            a2[r * H + j] = al;
            t2[r * H + j] = t;
            const uint32_t row = a.lo + 2 * tile + r;
            if (row < a.hi) {
              if (a.dbg.l2) a.dbg.l2[(size_t)row * M + j] = l2;      // columns 0..H-1 of the [G][M] arrays
              if (a.dbg.u2) a.dbg.u2[(size_t)row * M + j] = u2;
            }
          }
        }
      }
    }
    wave_lds_sync();
    // ---- the ten outputs: lower rows (lu = 0), then upper rows (lu = 1); lane = (rho, i = ci) -----
    const uint32_t orow = a.lo + 2 * tile + rho;
#pragma unroll 1
    for (int lu = 0; lu < 2; ++lu) {
      f32x16 D2 = f16_zero(), Kt[2];
      float acc = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) D2[r] = G3s[ci * W1ROWS + acc_row(r, half)];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const f32x4 hv = *reinterpret_cast<const f32x4*>(H3s + ci * LDH + 32 * mb + 8 * gq + 4 * half);
#pragma unroll
          for (int t = 0; t < 4; ++t) Kt[mb][4 * gq + t] = hv[t];
        }
      const float* m2t = M2s + col;
#pragma unroll 1
      for (int jb = 0; jb < 2; ++jb) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int j0 = 32 * jb + 8 * gq + 4 * half;
          const f32x4 w3 = *reinterpret_cast<const f32x4*>(N3s + ci * LDH + j0);
          const f32x4 sv = *reinterpret_cast<const f32x4*>(s2 + rho * H + j0);
          const f32x4 av = *reinterpret_cast<const f32x4*>(a2 + rho * H + j0);
          const f32x4 tv = *reinterpret_cast<const f32x4*>(t2 + rho * H + j0);
          const f32x4 bv = *reinterpret_cast<const f32x4*>(zc + rho * H + j0);
          const f32x4 fv = col < W1ROWS ? *reinterpret_cast<const f32x4*>(F2T + col * LDH + j0)
                                        : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const float wp = fmaxf(w3[t], 0.f), wm = fminf(w3[t], 0.f);
            const float lam = lu ? wp * sv[t] + wm * av[t] : wp * av[t] + wm * sv[t];
            acc = acc + lam * bv[t];
            acc = acc + (lu ? wp : wm) * tv[t];
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) Kt[mb] = mfma32(m2t[(j0 + t) * LDH + 32 * mb], lam, Kt[mb]);
            D2 = mfma32(fv[t], lam, D2);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // Kt[mb][r] = K[(rho, i)][k = 32 mb + acc_row(r, half)]
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int k0 = 32 * mb + 8 * gq + 4 * half;
          const f32x4 sv = *reinterpret_cast<const f32x4*>(s1 + rho * H + k0);
          const f32x4 av = *reinterpret_cast<const f32x4*>(a1 + rho * H + k0);
          const f32x4 zv = *reinterpret_cast<const f32x4*>(d1 + rho * H + k0);
          const f32x4 tv = *reinterpret_cast<const f32x4*>(th + rho * H + k0);
          const f32x4 w1 = col < W1ROWS ? *reinterpret_cast<const f32x4*>(A1T + col * LDH + k0)
                                        : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const float q = Kt[mb][4 * gq + t];
            const float qp = fmaxf(q, 0.f), qm = fminf(q, 0.f);
            const float R = lu ? qp * sv[t] + qm * av[t] : qp * av[t] + qm * sv[t];
            acc = acc + R * zv[t];
            acc = acc + (lu ? qp : qm) * (2.0f * tv[t]);
            D2 = mfma32(w1[t], R, D2);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // D2[r] = (G3 + Lambda F2 + R A1)[(rho, i)][c = acc_row(r, half)]: c = 0..3, 8, 9 on half 0, 4..7 on half 1
      float l1 = ((fabsf(D2[0]) + fabsf(D2[1])) + fabsf(D2[2])) + fabsf(D2[3]);
      if (half == 0) l1 = (l1 + fabsf(D2[4])) + fabsf(D2[5]);
      l1 = l1 + shfl_xor32(l1);
      acc = acc + shfl_xor32(acc);
      if (half == 0 && ci < C && orow < a.hi) {
        const float bound = (lu ? acc + a.eps * l1 : acc - a.eps * l1) + oc[rho * W1ROWS + ci];
        a.lbub[(size_t)(orow - a.lo) * (2 * C) + lu * C + ci] = bound;
        float* dst = lu ? a.dbg.ub : a.dbg.lb;
        if (dst) dst[(size_t)orow * C + ci] = bound;
      }
    }
    wave_lds_sync();    // the next trip overwrites the arrays this one read
  }
}

// barrier lower bound at h (classification.py:224-225)
__device__ __forceinline__ float barrier_lo(const DynScalars& d, float h) {
  return -d.alpha_1 * (expf(d.sigma_1 * h) - 1.0f);
}

// What ibp_cbf_qp's sub-problems of one grid row are built from: the (ibp_sigmoid'ed) bounds and the
// barrier lower bounds at eta - eps and eta + eps.
struct RowQP {
  float h[C], lb[C], ub[C], lo_m[C], lo_p[C];
};
__device__ __forceinline__ void load_row_qp(const CrownArgs& a, const float* tab, uint32_t row, RowQP& q) {
  eta_row(a, tab, row, q.h);
  const float* src = a.lbub + (size_t)(row - a.lo) * (2 * C);
  load_row10(src, q.lb);
  load_row10(src + C, q.ub);
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const float hl = q.h[j] - a.eps, hu = q.h[j] + a.eps;
    q.lo_m[j] = barrier_lo(a.d, hl);
    q.lo_p[j] = barrier_lo(a.d, hu);
    if (a.d.scale_nominal) {             // ibp_sigmoid (classification.py:175-181)
      const float sl = 1.0f / (1.0f + expf(-q.lb[j])), su = 1.0f / (1.0f + expf(-q.ub[j]));
      q.lb[j] = (a.d.alpha_2 * (1.0f - hu) - q.lo_p[j]) * sl + q.lo_p[j];
      q.ub[j] = (a.d.alpha_2 * (1.0f - hl) - q.lo_m[j]) * su + q.lo_m[j];
    }
  }
}
// sub-problem i of the lower-bound call (which = 0) or the upper-bound call (1), classification.py:210-231
__device__ __forceinline__ void sub_problem(const RowQP& q, int i, int which, float (&lower)[C], float (&nom)[C]) {
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const bool diag = j == i;
    if (which == 0) {
      lower[j] = diag ? q.lo_p[j] : q.lo_m[j];
      nom[j] = diag ? q.lb[j] : q.ub[j];
    } else {
      lower[j] = diag ? q.lo_m[j] : q.lo_p[j];
      nom[j] = diag ? q.ub[j] : q.lb[j];
    }
  }
}

__device__ __forceinline__ bool crown_stopped(const CrownArgs& a) {
  return *a.stop != 0;            // k_crown_prep has cleared a flag of the workspace's own
}

// one lane = one grid row, its ten sub-problems of each call in turn
__global__ __launch_bounds__(256) void k_crown_qp1(CrownArgs a) {
  if (crown_stopped(a)) return;
  __shared__ float tab[MAXT + 1];
  for (int v = threadIdx.x; v <= a.T; v += blockDim.x) tab[v] = a.etab[v];
  __syncthreads();
  const uint32_t r = a.lo + blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = r < a.hi;
  RowQP q;
  load_row_qp(a, tab, valid ? r : a.hi - 1, q);
  uint32_t c0 = 0xFFFFFFFFu, c1 = 0xFFFFFFFFu;
#pragma unroll 1
  for (int i = 0; i < C; ++i) {
    float lower[C], nom[C], v[C], mu;
    sub_problem(q, i, 0, lower, nom);
    c0 &= qp_bisect(lower, nom, a.d.max_iter - 1, a.d.tol, v, mu);
    sub_problem(q, i, 1, lower, nom);
    c1 &= qp_bisect(lower, nom, a.d.max_iter - 1, a.d.tol, v, mu);
  }
  c0 = wave_and(valid ? c0 : 0xFFFFFFFFu);
  c1 = wave_and(valid ? c1 : 0xFFFFFFFFu);
  if ((threadIdx.x & 63) == 0) {
    atomicAnd(a.words + 2 * a.b, c0);
    atomicAnd(a.words + 2 * a.b + 1, c1);
  }
}

__global__ __launch_bounds__(256) void k_crown_qp2(CrownArgs a) {
  if (crown_stopped(a)) return;
  __shared__ float tab[MAXT + 1];
  for (int v = threadIdx.x; v <= a.T; v += blockDim.x) tab[v] = a.etab[v];
  __syncthreads();
  const uint32_t r = a.lo + blockIdx.x * blockDim.x + threadIdx.x;
  const bool valid = r < a.hi;
  RowQP q;
  load_row_qp(a, tab, valid ? r : a.hi - 1, q);
  const int e0 = qp_exit_iter(a.words[2 * a.b], a.d.max_iter), e1 = qp_exit_iter(a.words[2 * a.b + 1], a.d.max_iter);
  float flb[C], fub[C];
#pragma unroll
  for (int j = 0; j < C; ++j) flb[j] = fub[j] = 0.f;
#pragma unroll 1
  for (int i = 0; i < C; ++i) {
    float lower[C], nom[C], v[C], mu;
    sub_problem(q, i, 0, lower, nom);
    qp_bisect(lower, nom, e0, a.d.tol, v, mu);
#pragma unroll
    for (int j = 0; j < C; ++j) flb[j] = (j == i) ? v[j] : flb[j];
    sub_problem(q, i, 1, lower, nom);
    qp_bisect(lower, nom, e1, a.d.tol, v, mu);
#pragma unroll
    for (int j = 0; j < C; ++j) fub[j] = (j == i) ? v[j] : fub[j];
  }
  // runner-up set under the perturbation: eta >= max eta - 2 eps, label excluded (certify_crown.py:144-147)
  float mx = q.h[0];
#pragma unroll
  for (int j = 1; j < C; ++j) mx = fmaxf(mx, q.h[j]);
  const float thr = mx - a.two_eps;
  float fw = -INFINITY, fy = 0.f;
#pragma unroll
  for (int j = 0; j < C; ++j) {
    if (j == a.label) fy = flb[j];
    else if (q.h[j] >= thr) fw = fmaxf(fw, fub[j]);
  }
  float viol = (-fy + fw) + a.kappa;
  if (valid) {
    if (a.dbg.f_lb) store_row10(a.dbg.f_lb + (size_t)r * C, flb);
    if (a.dbg.f_ub) store_row10(a.dbg.f_ub + (size_t)r * C, fub);
  }
  viol = valid ? viol : -INFINITY;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) viol = fmaxf(viol, __shfl_xor(viol, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(a.keys + a.b, fkey(viol));
}

__global__ void k_crown_fin(CrownArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (crown_stopped(a)) {
    a.out[a.b] = -INFINITY;
    return;
  }
  const float m = unkey(a.keys[a.b]);
  a.out[a.b] = m;
  if (a.exit_iters) {
    a.exit_iters[2 * a.b] = qp_exit_iter(a.words[2 * a.b], a.d.max_iter);
    a.exit_iters[2 * a.b + 1] = qp_exit_iter(a.words[2 * a.b + 1], a.d.max_iter);
  }
  if (a.stop_on_violation && m > 0.f) *a.stop = 1;
}

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

inline uint32_t max_batch_rows(int64_t G, int32_t batches) {
  const int64_t ebs = G / batches;
  const int64_t nb = batches + ((G % batches) != 0 ? 1 : 0);
  const int64_t tail = G - (nb - 1) * ebs;
  return (uint32_t)(tail > ebs ? tail : ebs);
}

// the part every activation needs; GroupSort appends the folded images
inline size_t crown_base_bytes(int64_t G, int32_t batches) {
  const size_t nb = (size_t)batches + 1;
  return al(256) + 2 * al(FIODE_M * 4) + al((size_t)max_batch_rows(G, batches) * 2 * C * 4) + al(nb * 8) + al(nb * 4);
}

// gs_ok: fiode_certify_crown_act; fiode_certify_crown keeps refusing GroupSort with FIODE_ESHAPE
int crown_run(void* stream, const fiode_crown_config* cfg, const fiode_dyn_config* dyn, const fiode_dyn_weights* w,
              const float* x_feat, const uint8_t* grid, int64_t G, float* out, int32_t* exit_iters, int32_t* stop_flag,
              const fiode_crown_debug* dbg, void* workspace, size_t workspace_bytes, int32_t activation, bool gs_ok) {
  if (!cfg || !dyn || !w || !x_feat || !grid || !out || !workspace) return FIODE_EINVAL;
  if (activation != FIODE_ACT_RELU && activation != FIODE_ACT_GROUPSORT) return FIODE_EINVAL;
  if (activation == FIODE_ACT_GROUPSORT && !gs_ok) return FIODE_ESHAPE;
  const bool gs = activation == FIODE_ACT_GROUPSORT;
  if (dyn->n_hidden != C || dyn->mlp_size != M || dyn->x_dim != FIODE_X) return FIODE_ESHAPE;
  if (cfg->n_classes != C) return FIODE_ESHAPE;
  if (dyn->qp_max_iter < 1 || dyn->qp_max_iter > 32) return FIODE_EINVAL;
  if (cfg->label < 0 || cfg->label >= C || cfg->T <= 0 || cfg->T > MAXT || cfg->batches <= 0 || !(cfg->min_std > 0.f))
    return FIODE_EINVAL;
  if (G == 0) return FIODE_OK;
  if (G < cfg->batches || G >= (1LL << 32)) return FIODE_EINVAL;
  if (workspace_bytes < fiode_certify_crown_workspace_bytes_act(G, cfg->batches, activation)) return FIODE_EWORKSPACE;
  CrownArgs a{};
  a.G = (uint32_t)G;
  const uint32_t ebs = (uint32_t)(G / cfg->batches);
  a.nb = cfg->batches + ((G % cfg->batches) != 0 ? 1 : 0);
  a.label = cfg->label;
  a.T = cfg->T;
  a.stop_on_violation = cfg->stop_on_violation;
  for (int v = 0; v <= cfg->T; ++v) a.etab[v] = (float)((double)v / (double)cfg->T);
  a.eps = (float)(1.0 / cfg->T);                                                   // certify_crown.py:61
  a.two_eps = (float)(2.0 * (1.0 / cfg->T));                                       // :146
  a.kappa = (float)(sqrt(2.0) * (1.0 / (double)cfg->min_std) * (double)cfg->eps);  // :65-67
  a.d.alpha_1 = dyn->alpha_1; a.d.alpha_2 = dyn->alpha_2; a.d.sigma_1 = dyn->sigma_1;
  a.d.tol = dyn->qp_tol; a.d.scale_nominal = dyn->scale_nominal; a.d.max_iter = dyn->qp_max_iter;
  a.x_feat = x_feat; a.grid = grid;
  a.Q1 = w->Q1; a.b1 = w->b1; a.Qx = w->Qx; a.bx = w->bx; a.Q2 = w->Q2; a.b2 = w->b2; a.Q3 = w->Q3; a.b3 = w->b3;
  char* ws = static_cast<char*>(workspace);
  size_t o = 0;
  int32_t* own = reinterpret_cast<int32_t*>(ws + o); o += al(256);
  a.u = reinterpret_cast<float*>(ws + o); o += al(FIODE_M * 4);
  a.r1 = reinterpret_cast<float*>(ws + o); o += al(FIODE_M * 4);
  a.lbub = reinterpret_cast<float*>(ws + o); o += al((size_t)max_batch_rows(G, cfg->batches) * 2 * C * 4);
  a.words = reinterpret_cast<uint32_t*>(ws + o); o += al((size_t)(cfg->batches + 1) * 8);
  a.keys = reinterpret_cast<uint32_t*>(ws + o); o += al((size_t)(cfg->batches + 1) * 4);
  a.gs = gs ? reinterpret_cast<float*>(ws + o) : nullptr;
  a.own_flag = stop_flag ? 0 : 1;
  a.stop = stop_flag ? stop_flag : own;
  a.out = out;
  a.exit_iters = exit_iters;
  if (dbg) a.dbg = *dbg;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int dev = 0, ncu = 256;
  if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    ncu = 256;
  if (ncu <= 0) ncu = 256;
  const size_t lds = gs ? ((size_t)(H + 4 * W1ROWS) * LDH + W1ROWS * W1ROWS + TABF + H + (size_t)NW * WAVEF_GS) * sizeof(float)
                        : ((size_t)(M + 2 * W1ROWS) * LDQ + TABF + M + (size_t)NW * WAVEF) * sizeof(float);
  const auto bounds = gs ? k_crown_bounds_gs : k_crown_bounds;
  FIODE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(bounds),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_crown_prep, dim3(1), dim3(256), 0, st, a);
  FIODE_HIP_CHECK(hipGetLastError());
  if (gs) {
    const size_t lds_fold = (size_t)(M + 2 * W1ROWS + C + 1) * LDQ * sizeof(float);
    FIODE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_crown_fold_gs),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fold));
    hipLaunchKernelGGL(k_crown_fold_gs, dim3(1), dim3(256), lds_fold, st, a);
    FIODE_HIP_CHECK(hipGetLastError());
  }
  for (int b = 0; b < a.nb; ++b) {
    a.b = b;
    a.lo = (uint32_t)b * ebs;
    a.hi = b < a.nb - 1 ? a.lo + ebs : a.G;          // the last batch takes the tail (cert.hip batch_of)
    const uint32_t rows = a.hi - a.lo;
    const uint32_t ntiles = (rows + 1) / 2;
    uint32_t blocks = (ntiles + NW - 1) / NW;
    if (blocks > (uint32_t)ncu) blocks = (uint32_t)ncu;        // persistent: one workgroup per CU (LDS)
    hipLaunchKernelGGL(bounds, dim3(blocks), dim3(64 * NW), lds, st, a);
    FIODE_HIP_CHECK(hipGetLastError());
    const dim3 qgrid((rows + 255) / 256);
    hipLaunchKernelGGL(k_crown_qp1, qgrid, dim3(256), 0, st, a);
    FIODE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_crown_qp2, qgrid, dim3(256), 0, st, a);
    FIODE_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_crown_fin, dim3(1), dim3(64), 0, st, a);
    FIODE_HIP_CHECK(hipGetLastError());
  }
  return FIODE_OK;
}

}  // namespace

extern "C" size_t fiode_certify_crown_workspace_bytes(int64_t G, int32_t batches) {
  if (G <= 0 || batches <= 0) return 256;
  return crown_base_bytes(G, batches);
}

extern "C" size_t fiode_certify_crown_workspace_bytes_act(int64_t G, int32_t batches, int32_t activation) {
  if (G <= 0 || batches <= 0 || (activation != FIODE_ACT_RELU && activation != FIODE_ACT_GROUPSORT)) return 256;
  return crown_base_bytes(G, batches) + (activation == FIODE_ACT_GROUPSORT ? al((size_t)GS_FLOATS * 4) : 0);
}

extern "C" int fiode_certify_crown(void* stream, const fiode_crown_config* cfg, const fiode_dyn_config* dyn,
                                   const fiode_dyn_weights* w, const float* x_feat, const uint8_t* grid, int64_t G,
                                   float* out, int32_t* exit_iters, int32_t* stop_flag, const fiode_crown_debug* dbg,
                                   void* workspace, size_t workspace_bytes, int32_t activation) {
  return crown_run(stream, cfg, dyn, w, x_feat, grid, G, out, exit_iters, stop_flag, dbg, workspace, workspace_bytes,
                   activation, false);
}

extern "C" int fiode_certify_crown_act(void* stream, const fiode_crown_config* cfg, const fiode_dyn_config* dyn,
                                       const fiode_dyn_weights* w, const float* x_feat, const uint8_t* grid, int64_t G,
                                       float* out, int32_t* exit_iters, int32_t* stop_flag,
                                       const fiode_crown_debug* dbg, void* workspace, size_t workspace_bytes,
                                       int32_t activation) {
  return crown_run(stream, cfg, dyn, w, x_feat, grid, G, out, exit_iters, stop_flag, dbg, workspace, workspace_bytes,
                   activation, true);
}
