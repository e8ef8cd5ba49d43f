// optax.adam [upstream]: the per-element step and its lazy form (esr_optim.hip dense_adam_kernel and the kAdamStepLazy
// segment update, esr_adam.hip catch-up and flush kernels).
//
// A row that gets no gradient at step t still moves:  mu *= b1 ; nu *= b2 ; p -= lr (mu ibc1_t) / (sqrt(nu ibc2_t) + eps),
// a function of (p, mu, nu, t) alone.  The lazy form keeps last[row] = the step the row is current with and applies the
// missed steps when the row is next read (or when every row is, esr_adam_flush):
//   * a gap of n <= kAdamExact steps: n calls of adam_elem with a zero gradient and the fp32 bias corrections the host
//     passes esr_dense_adam for those steps -- the dense kernel's own operations, bit for bit;
//   * a longer gap: in fp64, mu *= b1^n, nu *= b2^n and  p -= lr mu sum_s a_s / (x r_s + eps)  with x = sqrt(nu),
//     a_s = b1^s ibc1_(t0+s), r_s = sqrt(b2^s ibc2_(t0+s)).  The sum is cut after kmax terms (the host picks kmax so that the
//     tail is below 1e-7 of the sum) and evaluated per element by one of two series whose coefficients are formed once per
//     row: in eps / (x r_s) when x is large, in x r_s / eps when x is small (both ratios <= kAdamTheta: the cut series is
//     within kAdamTheta^kAdamTerms of the sum).  Elements in the band between the two regimes sum the kmax terms directly.
//     The result is one rounding of the fp64 value: within 1e-6 |dp| + 1 ulp of an fp64 replay of the n steps.
#pragma once
#include <math.h>

#include "esr_common.h"

namespace esr {

// One element of one optax.adam step, with every rounding spelled out.  ONE definition for every kernel that applies it:
// dense_adam_kernel, the lazy catch-up and the lazy sparse step.  The moment updates are single fused multiply-adds --
// what dense_adam_kernel's float4 loop has always executed (the compiler contracted  b1 * m + omb1 * g  there) -- so no
// kernel's result depends on what the compiler fuses where it is inlined.
__device__ __forceinline__ void adam_elem(float& pv, float& m, float& v, float gv, float lr, float b1, float b2,
                                          float omb1, float omb2, float eps, float inv_bc1, float inv_bc2) {
  m = __fmaf_rn(b1, m, omb1 * gv);
  v = __fmaf_rn(b2, v, omb2 * gv * gv);
  pv -= lr * (m * inv_bc1) / (sqrtf(v * inv_bc2) + eps);
}
// The same step unfused: what dense_adam_kernel's scalar tail loop (the last numel % 4 elements of a table) executes.
// With a zero gradient the two forms agree bit for bit; with a gradient, an element of a table whose numel is not a
// multiple of 4 takes the form its flat index falls under in the dense kernel (adam_is_tail).
__device__ __forceinline__ void adam_elem_tail(float& pv, float& m, float& v, float gv, float lr, float b1, float b2,
                                               float omb1, float omb2, float eps, float inv_bc1, float inv_bc2) {
#pragma clang fp contract(off)
  m = b1 * m + omb1 * gv;
  v = b2 * v + omb2 * gv * gv;
  pv -= lr * (m * inv_bc1) / (sqrtf(v * inv_bc2) + eps);
}
// flat element index i of a [V, D] table: does dense_adam_kernel step it in its scalar tail?
__device__ __forceinline__ bool adam_is_tail(int64_t i, int64_t V, int D) { return i >= ((V * D) & ~(int64_t)3); }

constexpr int kAdamExact = ESR_ADAM_EXACT_STEPS;  // W: gaps of up to this many steps are replayed step by step (bit-exact)
constexpr int kAdamTerms = 12;       // terms of each series of the long-gap form
constexpr double kAdamTheta = 0.25;  // a series is used where its ratio is <= this: error <= 0.25^12 = 6e-8 relative

// Everything a lazy Adam kernel needs besides the tables.  ibc1[j] / ibc2[j] are the fp32 bias-correction reciprocals of
// step now - j, computed by the host exactly as esr_dense_adam computes them (zero for steps < 1).
struct AdamLazyArgs {
  float* nu[2];
  int32_t* last[2];
  float lr, b1, b2, eps;
  float ibc1[kAdamExact + 1], ibc2[kAdamExact + 1];
  int now;
  int kmax;
};

// the lanes of a G-lane row group hold one row: every lane gets the group's sum (xor butterfly: the same bits on every lane)
__device__ __forceinline__ double group_sum_d(double v, int G) {
  for (int off = 1; off < G; off <<= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// Bring a row held in registers (p, mu, nu) from step t0 up to step t1 with zero gradients.  Every lane of the row group
// must call it (the long-gap coefficients are summed across the group).
template <int VEC, int NCH>
__device__ __forceinline__ void adam_catchup(RowRegs<VEC, NCH>& w, RowRegs<VEC, NCH>& m, RowRegs<VEC, NCH>& v, int t0, int t1,
                                             const AdamLazyArgs& ax, int lig, int G) {
  const int n = t1 - t0;
  if (n <= 0) return;
  if (n <= kAdamExact) {
    float z = 0.f;
    asm volatile("" : "+v"(z));  // a gradient the compiler cannot fold: the dense kernel's operations on a loaded zero
    const float omb1 = 1.0f - ax.b1, omb2 = 1.0f - ax.b2;
    for (int t = t0 + 1; t <= t1; ++t) {
      const int j = ax.now - t;
      float i1 = 0.f, i2 = 0.f;
#pragma unroll
      for (int q = 0; q <= kAdamExact; ++q)  // constant indices into the kernarg struct (a runtime one goes through scratch)
        if (q == j) {
          i1 = ax.ibc1[q];
          i2 = ax.ibc2[q];
        }
#pragma unroll
      for (int k = 0; k < NCH; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          adam_elem(w.v[k][e], m.v[k][e], v.v[k][e], z, ax.lr, ax.b1, ax.b2, omb1, omb2, ax.eps, i1, i2);
    }
    return;
  }
  // ---- long gap: per-row coefficients (the G lanes split the terms), then O(1) per element outside the band
  const int K = min(n, ax.kmax);
  const double b1 = ax.b1, b2 = ax.b2, eps = ax.eps;
  const double b1t0 = pow(b1, (double)t0), b2t0 = pow(b2, (double)t0);
  double L[kAdamTerms], S[kAdamTerms];
#pragma unroll
  for (int k = 0; k < kAdamTerms; ++k) L[k] = S[k] = 0.0;
  {
    double b1s = pow(b1, (double)(lig + 1)), b2s = pow(b2, (double)(lig + 1));
    const double b1G = pow(b1, (double)G), b2G = pow(b2, (double)G);
    for (int s = lig + 1; s <= K; s += G) {
      const double a = b1s / (1.0 - b1t0 * b1s);
      const double r = sqrt(b2s / (1.0 - b2t0 * b2s));
      const double q = 1.0 / r;
      double tl = a * q, ts = a;
#pragma unroll
      for (int k = 0; k < kAdamTerms; ++k) {
        L[k] += tl;  // sum a_s / r_s^(k+1)
        S[k] += ts;  // sum a_s r_s^k
        tl *= q;
        ts *= r;
      }
      b1s *= b1G;
      b2s *= b2G;
    }
  }
#pragma unroll
  for (int k = 0; k < kAdamTerms; ++k) {
    L[k] = group_sum_d(L[k], G);
    S[k] = group_sum_d(S[k], G);
  }
  const double rmax = sqrt(b2 / (1.0 - b2t0 * b2));  // r_s falls with s
  const double b2K = pow(b2, (double)K);
  const double rmin = sqrt(b2K / (1.0 - b2t0 * b2K));
  const double b1n = pow(b1, (double)n), b2n = pow(b2, (double)n);
  const double lr = ax.lr;
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double mm = m.v[k][e], vv = v.v[k][e];
      const double x = sqrt(vv);
      double f;
      if (x * rmin * kAdamTheta >= eps) {  // eps / (x r_s) <= theta for every s
        const double u = eps / x;
        double acc = L[kAdamTerms - 1];
#pragma unroll
        for (int i = kAdamTerms - 2; i >= 0; --i) acc = L[i] - u * acc;
        f = acc / x;
      } else if (x * rmax <= kAdamTheta * eps) {  // x r_s / eps <= theta for every s
        const double u = x / eps;
        double acc = S[kAdamTerms - 1];
#pragma unroll
        for (int i = kAdamTerms - 2; i >= 0; --i) acc = S[i] - u * acc;
        f = acc / eps;
      } else {  // the band between: the terms themselves
        f = 0.0;
        double b1s = b1, b2s = b2;
        for (int s = 1; s <= K; ++s) {
          f += (b1s / (1.0 - b1t0 * b1s)) / (x * sqrt(b2s / (1.0 - b2t0 * b2s)) + eps);
          b1s *= b1;
          b2s *= b2;
        }
      }
      w.v[k][e] = (float)((double)w.v[k][e] - lr * mm * f);
      m.v[k][e] = (float)(mm * b1n);
      v.v[k][e] = (float)(vv * b2n);
    }
}

// Host: fill the scalar part of an AdamLazyArgs for step `now` (nu / last are the caller's).  The bias corrections of steps
// now - kAdamExact .. now are esr_dense_adam's own (fp64 on the host, rounded to fp32 reciprocals).  kmax = the number of
// terms of the long-gap sum: term s is at most rho^(s-1) / sqrt(1 - b2) times term 1 (rho = b1 / sqrt(b2)), so the tail after
// kmax terms is below 1e-7 of the sum; no cut when rho >= 1.
inline void adam_lazy_args(AdamLazyArgs& ax, float lr, float b1, float b2, float eps, int now) {
  ax.lr = lr;
  ax.b1 = b1;
  ax.b2 = b2;
  ax.eps = eps;
  ax.now = now;
  for (int j = 0; j <= kAdamExact; ++j) {
    const int64_t t = (int64_t)now - j;
    ax.ibc1[j] = ax.ibc2[j] = 0.f;
    if (t >= 1) {
      const double bc1 = 1.0 - pow((double)b1, (double)t);
      const double bc2 = 1.0 - pow((double)b2, (double)t);
      ax.ibc1[j] = (float)(1.0 / bc1);
      ax.ibc2[j] = (float)(1.0 / bc2);
    }
  }
  ax.kmax = 0x7fffffff;
  const double rho = (double)b1 / sqrt((double)b2);
  if (b1 <= 0.f) {
    ax.kmax = 1;
  } else if (rho < 1.0 && b2 < 1.f) {
    const double k = log(1e-7 * (1.0 - rho) * sqrt(1.0 - (double)b2)) / log(rho) + 1.0;
    if (k < 1e9) ax.kmax = std::max(1, (int)ceil(k));
  }
  ax.nu[0] = ax.nu[1] = nullptr;
  ax.last[0] = ax.last[1] = nullptr;
}

}  // namespace esr
