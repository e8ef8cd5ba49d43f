// WARP (Weston, Bengio, Usunier, IJCAI 2011) on the device: one fused kernel that samples the pair, scores the positive,
// searches the candidate stream for a negative that violates the margin, weights the step by the rank estimate and writes
// the loss and the three gradient rows.  The rule of one slot is esr_warp_sample.h's, which also holds the integer pieces
// and the per-lane chain this kernel calls; the update itself is the row-sparse engine (esr_sort.hip, esr_optim.hip) driven
// from factorization.WARP.
//
// Layout.  One slot per group of G lanes, G the power of two >= D / 4 (1 .. 32), as bpr_fwd_bwd_kernel: lane l of the
// group holds elements 4 l .. 4 l + 3 of a row as one float4 (lanes with 4 l >= D hold zeros), so every row load and every
// gradient store is 16 bytes per lane and 64 / G slots share a wave.  Every lane of a group computes the slot's Philox
// words and walks the binary search itself (the same addresses in all G lanes: one broadcast access), so control flow is
// uniform per group and the cross-lane sums never leave a group; a wave runs until its slowest group is done.
// x and y_i are loaded once and stay in registers across the search; the y_j of the violating trial is still in registers
// when the gradients are formed: no row is read twice.  A trial is a chain of dependent loads (up to 32 probes of the row,
// then the candidate's row); nothing but other waves hides it.
// A slot's outputs depend on its own stream, rows and parameters only: no reduction across slots, no float atomic, no
// grid-wide pass and nothing polled.  The only loops are the <= max_trials trials and the <= 32-probe search.
#include "esr_common.h"
#include "esr_warp_sample.h"

namespace esr {

constexpr int kWarpFailBadPosition = 1 << 30;  // as FAIL_BAD_POSITION of esr_als.hip
constexpr int64_t kWarpMaxBlocks = (int64_t)kMaxGrid * 16;

__device__ __forceinline__ float warp_group_dot(const float4& x, const float4& y, int G) {
  return group_sum(warp_lane_dot(x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w), G);
}

template <int G>
__global__ __launch_bounds__(kBlock) void warp_step_kernel(
    const float* __restrict__ user_table, int64_t nu, const float* __restrict__ item_table, uint32_t ni, int D,
    const int64_t* __restrict__ row_offsets, const int32_t* __restrict__ row_upos, const int32_t* __restrict__ row_ipos,
    uint32_t nnz, const float* __restrict__ rank_weight, uint64_t seed, uint32_t step, int64_t B, int max_trials, float margin,
    float reg, int32_t* __restrict__ out_u, int32_t* __restrict__ out_i, int32_t* __restrict__ out_j,
    int32_t* __restrict__ out_valid, int32_t* __restrict__ out_trials, float* __restrict__ loss_t, float* __restrict__ diff_t,
    float* __restrict__ grads, int32_t* __restrict__ failed) {
  constexpr int kGroups = kBlock / G;
  const int lig = threadIdx.x % G, nvec = D >> 2;
  const bool holds = lig < nvec;  // (D = 100: 25 of the 32 lanes hold a chunk)
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  const int64_t ngroups = (int64_t)gridDim.x * kGroups;
  for (int64_t t = (int64_t)blockIdx.x * kGroups + threadIdx.x / G; t < B; t += ngroups) {  // (uniform per group)
    uint32_t w[4];
    const WarpPair pr = warp_pick_pair(row_offsets, row_upos, row_ipos, nu, nnz, key, step, (uint32_t)t, w);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 gu = zero, gi = zero, gj = zero;
    float loss = 0.f, d = 0.f;
    int32_t j = 0, valid = 0, trials = 0;
    if (pr.i < 0 || (uint32_t)pr.i >= ni) {
      if (lig == 0) atomicOr(failed, kWarpFailBadPosition);
    } else {
      float4 x = zero, yi = zero, yj = zero;
      if (holds) {
        x = *reinterpret_cast<const float4*>(user_table + (int64_t)pr.u * D + 4 * lig);
        yi = *reinterpret_cast<const float4*>(item_table + (int64_t)pr.i * D + 4 * lig);
      }
      const float si = warp_group_dot(x, yi, G);
      for (int c = 0; c < max_trials && !valid; ++c) {
        j = warp_candidate(key, step, (uint32_t)t, c, ni, w);
        if (!bpr_row_has(row_ipos, pr.lo, pr.hi, j)) {
          trials += 1;
          if (holds) yj = *reinterpret_cast<const float4*>(item_table + (int64_t)j * D + 4 * lig);
          const float dd = __fsub_rn(si, warp_group_dot(x, yj, G));
          if (dd < margin) {
            valid = 1;
            d = dd;
          }
        }
      }
      if (valid) {
        const float wt = rank_weight[warp_rank(ni, pr.hi - pr.lo, trials)];
        loss = wt * (margin - d);
        const float4 df = make_float4(yi.x - yj.x, yi.y - yj.y, yi.z - yj.z, yi.w - yj.w);
        gu = make_float4(reg * x.x - wt * df.x, reg * x.y - wt * df.y, reg * x.z - wt * df.z, reg * x.w - wt * df.w);
        gi = make_float4(reg * yi.x - wt * x.x, reg * yi.y - wt * x.y, reg * yi.z - wt * x.z, reg * yi.w - wt * x.w);
        gj = make_float4(reg * yj.x + wt * x.x, reg * yj.y + wt * x.y, reg * yj.z + wt * x.z, reg * yj.w + wt * x.w);
      }
    }
    if (lig == 0) {
      out_u[t] = pr.u;
      out_i[t] = pr.i;
      out_j[t] = j;
      out_valid[t] = valid;
      out_trials[t] = trials;
      loss_t[t] = loss;
      if (diff_t) diff_t[t] = d;
    }
    if (grads && holds) {  // [user rows ; positive rows ; negative rows], one row per occurrence
      *reinterpret_cast<float4*>(grads + t * D + 4 * lig) = gu;
      *reinterpret_cast<float4*>(grads + (B + t) * D + 4 * lig) = gi;
      *reinterpret_cast<float4*>(grads + (2 * B + t) * D + 4 * lig) = gj;
    }
  }
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_warp_geometry(int* max_trials, int* max_rank, int* rank_multiple) {
  ESR_REQUIRE(max_trials && max_rank && rank_multiple, "esr_warp_geometry: null pointer");
  *max_trials = kWarpMaxTrials;
  *max_rank = kWarpMaxRank;
  *rank_multiple = kWarpRankMultiple;
  return ESR_OK;
}

int esr_warp_step(const float* user_table, int64_t nu, const float* item_table, int64_t ni, int D, const int64_t* row_offsets,
                  const int32_t* row_upos, const int32_t* row_ipos, int64_t nnz, const float* rank_weight, uint64_t seed,
                  uint32_t step, int64_t B, int max_trials, float margin, float reg, int32_t* out_u, int32_t* out_i,
                  int32_t* out_j, int32_t* out_valid, int32_t* out_trials, float* loss_t, float* diff_t, float* grads,
                  int32_t* failed, esr_stream_t stream) {
  TraceScope trace_scope_("esr_warp_step");
  const char* who = "esr_warp_step";
  ESR_REQUIRE(D >= kWarpRankMultiple && D <= kWarpMaxRank && D % kWarpRankMultiple == 0,
              "%s: D=%d is not a multiple of %d in [%d, %d]", who, D, kWarpRankMultiple, kWarpRankMultiple, kWarpMaxRank);
  ESR_REQUIRE(nnz >= 1 && nnz <= (int64_t)INT32_MAX && ni >= 1 && ni <= (int64_t)INT32_MAX && nu >= 1 &&
                  nu <= (int64_t)INT32_MAX && B >= 1 && B <= (int64_t)INT32_MAX,
              "%s: bad sizes nu=%lld ni=%lld nnz=%lld B=%lld (each in [1, 2^31 - 1]: nnz and ni are 32-bit multiply-high factors)",
              who, (long long)nu, (long long)ni, (long long)nnz, (long long)B);
  ESR_REQUIRE(max_trials >= 1 && max_trials <= kWarpMaxTrials, "%s: max_trials=%d outside [1, %d]", who, max_trials,
              kWarpMaxTrials);
  ESR_REQUIRE(margin >= -3.4028235e38f && margin <= 3.4028235e38f, "%s: margin=%g must be finite", who, (double)margin);
  ESR_REQUIRE(reg >= 0.f && reg <= 3.4028235e38f, "%s: reg=%g must be finite and not negative", who, (double)reg);
  ESR_REQUIRE(user_table && item_table && row_offsets && row_upos && row_ipos && rank_weight && out_u && out_i && out_j &&
                  out_valid && out_trials && loss_t && failed,
              "%s: null pointer", who);
  ESR_REQUIRE((((uintptr_t)user_table | (uintptr_t)item_table | (uintptr_t)grads) & 15) == 0 &&
                  ((uintptr_t)row_offsets & 7) == 0 &&
                  (((uintptr_t)row_upos | (uintptr_t)row_ipos | (uintptr_t)rank_weight | (uintptr_t)out_u | (uintptr_t)out_i |
                    (uintptr_t)out_j | (uintptr_t)out_valid | (uintptr_t)out_trials | (uintptr_t)loss_t | (uintptr_t)diff_t |
                    (uintptr_t)failed) & 3) == 0,
              "%s: misaligned pointer (tables and grads: 16 bytes, row_offsets: 8)", who);
  hipStream_t st = as_stream(stream);
  const int G = warp_lanes(D);
  const int grid = (int)std::min<int64_t>(cdiv(B, kBlock / G), kWarpMaxBlocks);
#define ESR_WARP_LAUNCH(GG)                                                                                                \
  ESR_KT("warp_step", st,                                                                                                  \
         hipLaunchKernelGGL(warp_step_kernel<GG>, dim3(grid), dim3(kBlock), 0, st, user_table, nu, item_table, (uint32_t)ni, \
                            D, row_offsets, row_upos, row_ipos, (uint32_t)nnz, rank_weight, seed, step, B, max_trials, margin, \
                            reg, out_u, out_i, out_j, out_valid, out_trials, loss_t, diff_t, grads, failed))
  switch (G) {
    case 1: ESR_WARP_LAUNCH(1); break;
    case 2: ESR_WARP_LAUNCH(2); break;
    case 4: ESR_WARP_LAUNCH(4); break;
    case 8: ESR_WARP_LAUNCH(8); break;
    case 16: ESR_WARP_LAUNCH(16); break;
    default: ESR_WARP_LAUNCH(32); break;
  }
#undef ESR_WARP_LAUNCH
  return check_launch(who);
}

}  // extern "C"
