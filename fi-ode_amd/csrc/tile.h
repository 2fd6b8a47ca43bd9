// Wave-tile building blocks of the Cayley-MLP dynamics (classification.py:96-102) shared by
// the training-step, eval and ODE kernels.  See lyap.hip for the layout.
#pragma once
#include "common.h"

namespace fiode_tile {
constexpr int C = FIODE_C;
constexpr int M = FIODE_M;
constexpr int LDQ = FIODE_LDQ;

__device__ __forceinline__ void load_row10(const float* p, float (&v)[C]) {
  const float2* q = reinterpret_cast<const float2*>(p);
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const float2 t = q[j];
    v[2 * j] = t.x;
    v[2 * j + 1] = t.y;
  }
}
__device__ __forceinline__ void store_row10(float* p, const float (&v)[C]) {
  float2* q = reinterpret_cast<float2*>(p);
#pragma unroll
  for (int j = 0; j < 5; ++j) q[j] = make_float2(v[2 * j], v[2 * j + 1]);
}

// relu(dropout(z)) on one accumulator tile, in place (classification.py:98,100); DROP = false:
// plain relu (dropout off: keep = 1, scale = 1 -- the same values, without the per-element mask work)
template <bool DROP = true>
__device__ __forceinline__ void dropout_relu(f32x16& z, uint32_t kw, int half, float scale) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if (DROP) {
      const bool keep = (kw >> acc_row(r, half)) & 1u;
      z[r] = keep ? fmaxf(z[r] * scale, 0.f) : 0.f;
    } else {
      z[r] = fmaxf(z[r], 0.f);
    }
  }
}

// The activation of the MLP's two hidden layers, a compile-time parameter of the tile code.
// GROUPSORT (group size 2 over the halves, cayley.py GroupSort): with a = z[:M/2], b = z[M/2:] the
// output is cat(max(a, b), min(a, b)) -- unit u pairs with unit u + M/2.  With dropout (the fused
// Lyapunov training step, lyap.hip) the sort takes the dropped values: GroupSort(dropout(z)),
// classification.py:98,100.  The train_ode solves (odetrain.hip) instantiate RELU only.
enum Act { RELU = 0, GROUPSORT = 1 };

// GroupSort on the four accumulator blocks of a 32-row wave tile, in place.  Block mb holds units
// 32 mb .. 32 mb + 31 and register r of a lane is the same (unit offset, sample) in every block, so
// the pair (u, u + 64) is z[mb][r] / z[mb + 2][r] of one lane: 2 x 16 max/min, no exchange.
__device__ __forceinline__ void groupsort_tile(f32x16 (&z)[4]) {
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float a = z[mb][r], b = z[mb + 2][r];
      z[mb][r] = fmaxf(a, b);
      z[mb + 2][r] = fminf(a, b);
    }
}

// groupsort_tile that also returns the order of every pair, for the backward: bit 16 mb + r of gt is
// a > b and of eq is a == b for the pair z[mb][r] / z[mb + 2][r] (the sorted values are the same).
__device__ __forceinline__ void groupsort_tile_codes(f32x16 (&z)[4], uint32_t& gt, uint32_t& eq) {
  gt = 0;
  eq = 0;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float a = z[mb][r], b = z[mb + 2][r];
      gt |= (a > b ? 1u : 0u) << (16 * mb + r);
      eq |= (a == b ? 1u : 0u) << (16 * mb + r);
      z[mb][r] = fmaxf(a, b);
      z[mb + 2][r] = fminf(a, b);
    }
}

// GroupSort(dropout(z)) on the four accumulator blocks of a wave tile, in place: d = keep ? z * scale
// : 0 (dropout_relu's float32 expression), then the sort of groupsort_tile.  The keep bits of the
// pair z[mb][r] / z[mb + 2][r] are bit acc_row(r, half) of kw[mb] and of kw[mb + 2].  A pair with
// both members dropped is a tie of two zeros.
__device__ __forceinline__ void dropout_groupsort_tile(f32x16 (&z)[4], const uint32_t (&kw)[4], int half,
                                                       float scale) {
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool ka = (kw[mb] >> acc_row(r, half)) & 1u, kb = (kw[mb + 2] >> acc_row(r, half)) & 1u;
      const float a = ka ? z[mb][r] * scale : 0.f, b = kb ? z[mb + 2][r] * scale : 0.f;
      z[mb][r] = fmaxf(a, b);
      z[mb + 2][r] = fminf(a, b);
    }
}

// dropout_groupsort_tile that also returns the order of every pair of dropped values (the codes of
// groupsort_tile_codes; the sorted values are the same bits).
__device__ __forceinline__ void dropout_groupsort_tile_codes(f32x16 (&z)[4], const uint32_t (&kw)[4], int half,
                                                             float scale, uint32_t& gt, uint32_t& eq) {
  gt = 0;
  eq = 0;
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool ka = (kw[mb] >> acc_row(r, half)) & 1u, kb = (kw[mb + 2] >> acc_row(r, half)) & 1u;
      const float a = ka ? z[mb][r] * scale : 0.f, b = kb ? z[mb + 2][r] * scale : 0.f;
      gt |= (a > b ? 1u : 0u) << (16 * mb + r);
      eq |= (a == b ? 1u : 0u) << (16 * mb + r);
      z[mb][r] = fmaxf(a, b);
      z[mb + 2][r] = fminf(a, b);
    }
}

// The same on ONE accumulator block whose 32 rows are 16 units u and their 16 partners u + M/2 (tile
// rows i and i + 16, i.e. registers r and r + 8 of one lane: the paired unit map of k_lyap_bwd).
// ka / kb: the keep bits of the 16 units and of their partners, bit acc_row(r, half) for r < 8.
// Bit r of gt / eq: d[u] > d[u + M/2] and d[u] == d[u + M/2].
__device__ __forceinline__ void dropout_groupsort_pairs(f32x16& z, uint32_t ka, uint32_t kb, int half, float scale,
                                                        uint32_t& gt, uint32_t& eq) {
  gt = 0;
  eq = 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const bool ba = (ka >> acc_row(r, half)) & 1u, bb = (kb >> acc_row(r, half)) & 1u;
    const float a = ba ? z[r] * scale : 0.f, b = bb ? z[r + 8] * scale : 0.f;
    gt |= (a > b ? 1u : 0u) << r;
    eq |= (a == b ? 1u : 0u) << r;
    z[r] = fmaxf(a, b);
    z[r + 8] = fminf(a, b);
  }
}

// Backward of dropout_groupsort_pairs, in place: g holds d/d(sorted output) and becomes
// d/d(pre-dropout value): the routing of act_backward_tile<GROUPSORT>, then times keep * scale.
__device__ __forceinline__ void dropout_groupsort_pairs_backward(f32x16& g, uint32_t gt, uint32_t eq, uint32_t ka,
                                                                 uint32_t kb, int half, float scale) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const float gmx = g[r], gmn = g[r + 8];
    const bool first_max = (gt >> r) & 1u, tie = (eq >> r) & 1u;
    const bool ba = (ka >> acc_row(r, half)) & 1u, bb = (kb >> acc_row(r, half)) & 1u;
    const float halfsum = gmx / 2.0f + gmn / 2.0f;
    const float ga = tie ? halfsum : (first_max ? gmx : gmn);
    const float gb = tie ? halfsum : (first_max ? gmn : gmx);
    g[r] = ba ? ga * scale : 0.f;
    g[r + 8] = bb ? gb * scale : 0.f;
  }
}

// Backward of the activation on the four accumulator blocks of a wave tile, in place: g holds
// d/d(activation output) and becomes d/d(pre-activation).  RELU: g [a > 0] with a the activation
// output.  GROUPSORT: the max / min gradients go back to the pair's members by the codes of
// groupsort_tile_codes; a tie splits them in half (torch.maximum / minimum, sconv.hip gs_grad).
template <Act A>
__device__ __forceinline__ void act_backward_tile(const f32x16 (&a)[4], f32x16 (&g)[4], uint32_t gt, uint32_t eq) {
  if constexpr (A == GROUPSORT) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float gmx = g[mb][r], gmn = g[mb + 2][r];
        const bool first_max = (gt >> (16 * mb + r)) & 1u, tie = (eq >> (16 * mb + r)) & 1u;
        const float halfsum = gmx / 2.0f + gmn / 2.0f;
        g[mb][r] = tie ? halfsum : (first_max ? gmx : gmn);
        g[mb + 2][r] = tie ? halfsum : (first_max ? gmn : gmx);
      }
  } else {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) g[mb][r] = a[mb][r] > 0.f ? g[mb][r] : 0.f;
  }
}

// store one [32 hidden x 32 samples] accumulator block as rows of a sample-major [N][M] array
__device__ __forceinline__ void store_acc_rows(float* base_row, int mb, int half, const f32x16& z) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *reinterpret_cast<f32x4*>(base_row + 32 * mb + 8 * g + 4 * half) =
        f32x4{z[4 * g], z[4 * g + 1], z[4 * g + 2], z[4 * g + 3]};
}
__device__ __forceinline__ void load_acc_rows(const float* base_row, int mb, int half, f32x16& z) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(base_row + 32 * mb + 8 * g + 4 * half);
    z[4 * g] = t[0]; z[4 * g + 1] = t[1]; z[4 * g + 2] = t[2]; z[4 * g + 3] = t[3];
  }
}

// gather the 10 outputs of the (M padded to 32) layer-3 accumulator into every lane of the row
__device__ __forceinline__ void gather_ft(const f32x16& z3, int half, float (&ft)[C]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float o = shfl_xor32(z3[t]);
    ft[t] = half ? o : z3[t];
    ft[4 + t] = half ? z3[t] : o;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float o = shfl_xor32(z3[4 + t]);
    ft[8 + t] = half ? o : z3[4 + t];
  }
}

// Layers 1-2 of the MLP of one wave tile: z1/z2 become the post-dropout-ReLU activations a1^T,
// a2^T.  q1: hoisted layer-1 A operands.  A: the activation (GROUPSORT with DROP: the sort of the
// dropped values, dropout_groupsort_tile).
template <bool DROP = true, Act A = RELU>
__device__ __forceinline__ void mlp12_tile(const float* Q2s, const float (&q1)[4][5], const float* u_row,
                                           const float* b2, const float (&h)[C], const uint32_t (&kw1)[4],
                                           const uint32_t (&kw2)[4], float scale, int col, int half, f32x16 (&z1)[4],
                                           f32x16 (&z2)[4]) {
  // layer 1: z1 = u[b] + Q1 h   (hidden_to_mlp(h) + U_x(x), classification.py:97)
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) load_acc_rows(u_row, mb, half, z1[mb]);
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const float bs = half ? h[2 * s + 1] : h[2 * s];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) z1[mb] = mfma32(q1[mb][s], bs, z1[mb]);
  }
  if constexpr (A == GROUPSORT) {
    if constexpr (DROP) dropout_groupsort_tile(z1, kw1, half, scale);
    else groupsort_tile(z1);
  } else {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) dropout_relu<DROP>(z1[mb], kw1[mb], half, scale);
  }
  // layer 2: z2 = b2 + Q2 a1
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) load_acc_rows(b2, mb, half, z2[mb]);
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(Q2s + (32 * mb + col) * LDQ + 32 * kb + 8 * g + 4 * half);
#pragma unroll
        for (int t = 0; t < 4; ++t) z2[mb] = mfma32(q[t], z1[kb][4 * g + t], z2[mb]);
      }
    __builtin_amdgcn_sched_barrier(0);   // bound the LDS-read hoisting window to one k-block
  }
  if constexpr (A == GROUPSORT) {
    if constexpr (DROP) dropout_groupsort_tile(z2, kw2, half, scale);
    else groupsort_tile(z2);
  } else {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) dropout_relu<DROP>(z2[mb], kw2[mb], half, scale);
  }
}

// The MLP of one wave tile: layers 1-3, returns the layer-3 accumulator (mlp12_tile + layer 3).
template <bool DROP = true, Act A = RELU>
__device__ __forceinline__ f32x16 mlp_tile(const float* Q2s, const float* Q3s, const float (&q1)[4][5],
                                           const float* u_row, const float* b2, const float* b3,
                                           const float (&h)[C], const uint32_t (&kw1)[4], const uint32_t (&kw2)[4],
                                           float scale, int col, int half, f32x16 (&z1)[4], f32x16 (&z2)[4]) {
  mlp12_tile<DROP, A>(Q2s, q1, u_row, b2, h, kw1, kw2, scale, col, half, z1, z2);
  // layer 3: z3 = b3 + Q3 a2 (rows >= 10 of the 32-row tile are zero weights)
  f32x16 z3;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = acc_row(r, half);
    z3[r] = i < C ? b3[i] : 0.f;
  }
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      // rows >= C of the layer-3 A operand are zero (the image may hold only C rows)
      const f32x4 q = col < C ? *reinterpret_cast<const f32x4*>(Q3s + col * LDQ + 32 * kb + 8 * g + 4 * half)
                              : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) z3 = mfma32(q[t], z2[kb][4 * g + t], z3);
    }
  return z3;
}

// mlp_tile<false, GROUPSORT> that also returns the sort codes of both hidden layers (codes[0..1]:
// gt / eq of layer 1, codes[2..3]: of layer 2; the eval_dot backward).  The same operations in the
// same order as mlp_tile, so z1 / z2 and the returned accumulator are the same bits.
__device__ __forceinline__ f32x16 mlp_tile_groupsort_codes(const float* Q2s, const float* Q3s,
                                                           const float (&q1)[4][5], const float* u_row,
                                                           const float* b2, const float* b3, const float (&h)[C],
                                                           int col, int half, f32x16 (&z1)[4], f32x16 (&z2)[4],
                                                           uint32_t (&codes)[4]) {
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) load_acc_rows(u_row, mb, half, z1[mb]);
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const float bs = half ? h[2 * s + 1] : h[2 * s];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) z1[mb] = mfma32(q1[mb][s], bs, z1[mb]);
  }
  groupsort_tile_codes(z1, codes[0], codes[1]);
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) load_acc_rows(b2, mb, half, z2[mb]);
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(Q2s + (32 * mb + col) * LDQ + 32 * kb + 8 * g + 4 * half);
#pragma unroll
        for (int t = 0; t < 4; ++t) z2[mb] = mfma32(q[t], z1[kb][4 * g + t], z2[mb]);
      }
    __builtin_amdgcn_sched_barrier(0);
  }
  groupsort_tile_codes(z2, codes[2], codes[3]);
  f32x16 z3;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = acc_row(r, half);
    z3[r] = i < C ? b3[i] : 0.f;
  }
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 q = col < C ? *reinterpret_cast<const f32x4*>(Q3s + col * LDQ + 32 * kb + 8 * g + 4 * half)
                              : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) z3 = mfma32(q[t], z2[kb][4 * g + t], z3);
    }
  return z3;
}

// Stage the 128x128 mlp_to_mlp weight and the 10x128 mlp_to_hidden weight (zero rows up to
// q3_rows) into padded LDS images: 16-byte global loads, all of a thread's loads in flight
// together (a dependent 4-byte load loop took ~15 us of L2 latency at kernel start).
__device__ __forceinline__ void load_weight_images(const float* Q2, const float* Q3, float* Q2s, float* Q3s,
                                                   int q3_rows = 32) {
  const f32x4* Q2v = reinterpret_cast<const f32x4*>(Q2);
  constexpr int N2 = M * M / 4;                        // 4096 float4
  for (int e0 = threadIdx.x; e0 < N2; e0 += 8 * blockDim.x) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + u * blockDim.x;
      if (e < N2) v[u] = Q2v[e];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + u * blockDim.x;
      if (e < N2) *reinterpret_cast<f32x4*>(Q2s + (e >> 5) * LDQ + (e & 31) * 4) = v[u];
    }
  }
  if (Q3s) {
    const f32x4* Q3v = reinterpret_cast<const f32x4*>(Q3);
    for (int e = threadIdx.x; e < q3_rows * M / 4; e += blockDim.x) {
      const int i = e >> 5;
      *reinterpret_cast<f32x4*>(Q3s + i * LDQ + (e & 31) * 4) = i < C ? Q3v[e] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}
}  // namespace fiode_tile
