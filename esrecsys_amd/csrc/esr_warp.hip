// WARP (Weston, Bengio, Usunier, IJCAI 2011) on the device: one fused kernel that samples the pair, scores the positive,
// searches the candidate stream for a negative that violates the margin, weights the step by the rank estimate and writes
// the loss and the three gradient rows.  The rule of one slot is esr_warp_sample.h's; its integer pieces are BPR's
// (bpr_pick_pair, bpr_candidate, bpr_row_has of esr_bpr_sample.h) and its per-lane chain is row4_dot; the update itself is the row-sparse engine (esr_sort.hip, esr_optim.hip) driven
// from factorization.WARP.
//
// Layout.  One slot per group of G lanes in the float4 row-group layout of esr_row4.h (as bpr_fwd_bwd_kernel, whose
// triple_grads / triple_store form and store the gradient rows here too).  Every lane of a group computes the slot's Philox
// words and walks the binary search itself (the same addresses in all G lanes: one broadcast access), so control flow is
// uniform per group and the cross-lane sums never leave a group; a wave runs until its slowest group is done.
// x and y_i are loaded once and stay in registers across the search; the y_j of the violating trial is still in registers
// when the gradients are formed: no row is read twice.  A trial is a chain of dependent loads (up to 32 probes of the row,
// then the candidate's row); nothing but other waves hides it.
// A slot's outputs depend on its own stream, rows and parameters only: no reduction across slots, no float atomic, no
// grid-wide pass and nothing polled.  The only loops are the <= max_trials trials and the <= 32-probe search.
#include "esr_common.h"
#include "esr_row4.h"
#include "esr_sampled.h"
#include "esr_warp_sample.h"

namespace esr {

__device__ __forceinline__ float warp_group_dot(const float4& x, const float4& y, int G) {
  return group_sum(row4_dot(x, y), G);
}

template <int G>
__global__ __launch_bounds__(kBlock) void warp_step_kernel(
    const float* __restrict__ user_table, int64_t nu, const float* __restrict__ item_table, uint32_t ni, int D,
    const int64_t* __restrict__ row_offsets, const int32_t* __restrict__ row_upos, const int32_t* __restrict__ row_ipos,
    uint32_t nnz, const float* __restrict__ rank_weight, uint64_t seed, uint32_t step, int64_t B, int max_trials, float margin,
    float reg, int32_t* __restrict__ out_u, int32_t* __restrict__ out_i, int32_t* __restrict__ out_j,
    int32_t* __restrict__ out_valid, int32_t* __restrict__ out_trials, float* __restrict__ loss_t, float* __restrict__ diff_t,
    float* __restrict__ grads, int32_t* __restrict__ failed) {
  const int lig = row4_lig<G>();
  const bool holds = row4_holds(lig, D);
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  const int64_t ngroups = row4_stride<G>();
  for (int64_t t = row4_first<G>(); t < B; t += ngroups) {  // (uniform per group)
    uint32_t w[4];
    const BprPair pr = bpr_pick_pair(row_offsets, row_upos, row_ipos, nu, nnz, key, step, (uint32_t)t, w);
    const float4 zero = row4_zero();
    float4 gu = zero, gi = zero, gj = zero;
    float loss = 0.f, d = 0.f;
    int32_t j = 0, valid = 0, trials = 0;
    if (pr.i < 0 || (uint32_t)pr.i >= ni) {
      if (lig == 0) atomicOr(failed, kFailBadPosition);
    } else {
      float4 x = zero, yi = zero, yj = zero;
      if (holds) {
        x = *row4_ptr(user_table, pr.u, D, lig);
        yi = *row4_ptr(item_table, pr.i, D, lig);
      }
      const float si = warp_group_dot(x, yi, G);
      for (int c = 0; c < max_trials && !valid; ++c) {
        j = bpr_candidate(key, step, (uint32_t)t, c, ni, w);
        if (!bpr_row_has(row_ipos, pr.lo, pr.hi, j)) {
          trials += 1;
          if (holds) yj = *row4_ptr(item_table, j, D, lig);
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
        triple_grads(x, yi, yj, wt, reg, gu, gi, gj);
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
    triple_store(grads, t, B, D, lig, holds, gu, gi, gj);
  }
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_warp_geometry(int* max_trials, int* max_rank, int* rank_multiple) {
  ESR_REQUIRE(max_trials && max_rank && rank_multiple, "esr_warp_geometry: null pointer");
  *max_trials = kWarpMaxTrials;
  *max_rank = kRow4MaxRank;
  *rank_multiple = kRow4RankMultiple;
  return ESR_OK;
}

int esr_warp_step(const float* user_table, int64_t nu, const float* item_table, int64_t ni, int D, const int64_t* row_offsets,
                  const int32_t* row_upos, const int32_t* row_ipos, int64_t nnz, const float* rank_weight, uint64_t seed,
                  uint32_t step, int64_t B, int max_trials, float margin, float reg, int32_t* out_u, int32_t* out_i,
                  int32_t* out_j, int32_t* out_valid, int32_t* out_trials, float* loss_t, float* diff_t, float* grads,
                  int32_t* failed, esr_stream_t stream) {
  TraceScope trace_scope_("esr_warp_step");
  const char* who = "esr_warp_step";
  if (int rc = check_rank(who, D)) return rc;
  if (int rc = check_sizes(who, {{"nu", nu}, {"ni", ni}, {"nnz", nnz}, {"B", B}}, ": nnz and ni are 32-bit multiply-high factors"))
    return rc;
  ESR_REQUIRE(max_trials >= 1 && max_trials <= kWarpMaxTrials, "%s: max_trials=%d outside [1, %d]", who, max_trials,
              kWarpMaxTrials);
  ESR_REQUIRE(margin >= -3.4028235e38f && margin <= 3.4028235e38f, "%s: margin=%g must be finite", who, (double)margin);
  if (int rc = check_reg(who, reg)) return rc;
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
  const int G = row4_lanes(D);
  const int grid = (int)std::min<int64_t>(cdiv(B, kBlock / G), kSampledMaxBlocks);
  ESR_DISPATCH_G(G, ESR_KT("warp_step", st,
                           hipLaunchKernelGGL(warp_step_kernel<GG>, dim3(grid), dim3(kBlock), 0, st, user_table, nu, item_table,
                                              (uint32_t)ni, D, row_offsets, row_upos, row_ipos, (uint32_t)nnz, rank_weight, seed,
                                              step, B, max_trials, margin, reg, out_u, out_i, out_j, out_valid, out_trials,
                                              loss_t, diff_t, grads, failed)));
  return check_launch(who);
}

}  // extern "C"
