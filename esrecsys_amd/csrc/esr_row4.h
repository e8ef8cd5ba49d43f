// The float4 row-group layer of esr_bpr.hip, esr_warp.hip, esr_fpmc.hip, esr_sgns.hip, esr_bag.hip and esr_rerank.hip.  One
// item (a triple, a slot, a selected bag) per group of G lanes, G the power of two >= D / 4 (1 .. 32): lane l of the group
// holds elements 4 l .. 4 l + 3 of every row as one float4 (lanes with 4 l >= D hold zeros and store nothing): 16 bytes per
// lane and access, 64 / G items per wave.
// The first part is plain C++ (tests/host reach it through esr_warp_sample.h): the geometry and the one summation chain.
// The device part holds where a thread stands, the row accesses, the float4 arithmetic, the one logistic and the triple
// family's gradient rows; each keeps the expression the kernels used to spell out: kernels agree bit for bit only on the
// same expression (the note above group_sum).
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef ESR_HD
#if defined(__HIPCC__)
#define ESR_HD __host__ __device__
#else
#define ESR_HD
#endif
#endif

namespace esr {

constexpr int kRow4MaxRank = 128, kRow4RankMultiple = 4;  // 32 lanes x one float4; D a multiple of 4

// The power of two >= D / 4: the lanes of one item.
ESR_HD inline int row4_lanes(int D) {
  int G = 1;
  while (G < D / 4) G <<= 1;
  return G;
}

// One lane's chain over its four elements, on from acc: the only text of the summation order of every score of the
// family (warp_lane_dot for the host programs, row4_dot for the kernels).
ESR_HD inline float row4_chain(float x0, float x1, float x2, float x3, float y0, float y1, float y2, float y3, float acc) {
  acc = fmaf(x0, y0, acc);
  acc = fmaf(x1, y1, acc);
  acc = fmaf(x2, y2, acc);
  return fmaf(x3, y3, acc);
}

}  // namespace esr

// Expands BODY with a constexpr int GG = G, G one of row4_lanes' values.
#define ESR_DISPATCH_G(G, ...)                             \
  switch (G) {                                             \
    case 1: { constexpr int GG = 1; __VA_ARGS__; } break;  \
    case 2: { constexpr int GG = 2; __VA_ARGS__; } break;  \
    case 4: { constexpr int GG = 4; __VA_ARGS__; } break;  \
    case 8: { constexpr int GG = 8; __VA_ARGS__; } break;  \
    case 16: { constexpr int GG = 16; __VA_ARGS__; } break; \
    default: { constexpr int GG = 32; __VA_ARGS__; } break; \
  }

#ifdef __HIPCC__
#include "esr_common.h"

namespace esr {

// Where a thread stands: its lane in the group, whether that lane holds a chunk (D = 100: 25 of the 32 lanes do), the
// group's first item and the grid's stride in items (both uniform per group).
template <int G> __device__ __forceinline__ int row4_lig() { return threadIdx.x % G; }
__device__ __forceinline__ bool row4_holds(int lig, int D) { return lig < D >> 2; }
template <int G> __device__ __forceinline__ int64_t row4_first() { return (int64_t)blockIdx.x * (kBlock / G) + threadIdx.x / G; }
template <int G> __device__ __forceinline__ int64_t row4_stride() { return (int64_t)gridDim.x * (kBlock / G); }

__device__ __forceinline__ float4 row4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// where the lane's chunk of row `row` of table [n, D] lies (for a kernel that takes several rows under one test of holds)
__device__ __forceinline__ const float4* row4_ptr(const float* table, int64_t row, int D, int lig) {
  return reinterpret_cast<const float4*>(table + row * D + 4 * lig);
}

// the lane's chunk of row `row`; zeros (and no access) when !holds
__device__ __forceinline__ float4 row4_load(const float* table, int64_t row, int D, int lig, bool holds) {
  float4 v = row4_zero();
  if (holds) v = *row4_ptr(table, row, D, lig);
  return v;
}

__device__ __forceinline__ void row4_store(float* table, int64_t row, int D, int lig, bool holds, float4 v) {
  if (holds) *reinterpret_cast<float4*>(table + row * D + 4 * lig) = v;
}

// The lane's share of a . b in row4_chain's order, on from acc.
__device__ __forceinline__ float row4_dot(float4 a, float4 b, float acc = 0.f) {
  return row4_chain(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, acc);
}
// per element: a - b, fmaf(a, x, y), a * x, m ? a : b (a ternary on the struct itself selects between two addresses: scratch)
__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 fma4(float a, float4 x, float4 y) {
  return make_float4(__fmaf_rn(a, x.x, y.x), __fmaf_rn(a, x.y, y.y), __fmaf_rn(a, x.z, y.z), __fmaf_rn(a, x.w, y.w));
}
__device__ __forceinline__ float4 mul4(float a, float4 x) {
  return make_float4(__fmul_rn(a, x.x), __fmul_rn(a, x.y), __fmul_rn(a, x.z), __fmul_rn(a, x.w));
}
__device__ __forceinline__ float4 sel4(bool m, float4 a, float4 b) {
  return make_float4(m ? a.x : b.x, m ? a.y : b.y, m ? a.z : b.z, m ? a.w : b.w);
}
// softplus(s) and sigmoid(s) from ex = expf(-|s|) <= 1: neither overflows; expf / log1pf are the precise forms.  A ranking
// loss softplus(-d) and its g = sigmoid(-d) are logistic(-d, loss, g).
__device__ __forceinline__ void logistic(float s, float& softplus, float& sigmoid) {
  const float ex = expf(-fabsf(s));
  softplus = fmaxf(s, 0.f) + log1pf(ex);
  sigmoid = __fdiv_rn(s >= 0.f ? 1.0f : ex, 1.0f + ex);
}

// The triple family (BPR, WARP, FPMC): the lane's chunks of the three gradient rows of (x, y_i, y_j) under the scalar g,
// g_u = reg x - g (y_i - y_j), g_i = reg y_i - g x, g_j = reg y_j + g x.
__device__ __forceinline__ void triple_grads(float4 x, float4 yi, float4 yj, float g, float reg, float4& gu,
                                             float4& gi, float4& gj) {
  const float4 df = sub4(yi, yj);
  gu = make_float4(reg * x.x - g * df.x, reg * x.y - g * df.y, reg * x.z - g * df.z, reg * x.w - g * df.w);
  gi = make_float4(reg * yi.x - g * x.x, reg * yi.y - g * x.y, reg * yi.z - g * x.z, reg * yi.w - g * x.w);
  gj = make_float4(reg * yj.x + g * x.x, reg * yj.y + g * x.y, reg * yj.z + g * x.z, reg * yj.w + g * x.w);
}

// [user rows ; positive rows ; negative rows] of triple t of B, one row per occurrence; nothing when grads is null
__device__ __forceinline__ void triple_store(float* grads, int64_t t, int64_t B, int D, int lig, bool holds, float4 gu,
                                             float4 gi, float4 gj) {
  if (grads) {
    row4_store(grads, t, D, lig, holds, gu);
    row4_store(grads, B + t, D, lig, holds, gi);
    row4_store(grads, 2 * B + t, D, lig, holds, gj);
  }
}

}  // namespace esr
#endif  // __HIPCC__
