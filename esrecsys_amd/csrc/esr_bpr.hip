// Bayesian Personalised Ranking (Rendle, Freudenthaler, Gantner, Schmidt-Thieme, UAI 2009) on the device: the triple
// sampler and the fused logistic forward / backward over three gathered rows.  The update itself is the row-sparse engine
// (esr_sort.hip, esr_optim.hip) driven from factorization.BPR.
//
// Sampler.  One lane per triple; the rule is bpr_sample_triple (esr_bpr_sample.h), a function of (seed, step, slot, CSR)
// alone, inside the sampler shell of esr_sampled.h (sample_slots: a workgroup on 256 consecutive slots of ONE step, one
// integer atomic per wave into dropped[k]).  Integer arithmetic only; the only loops are the 15 candidates and the
// 31-probe binary search; no workgroup waits on another and nothing is polled.
//
// Forward / backward.  One triple per group of G lanes in the float4 row-group layout of esr_row4.h: lane l of the group
// holds elements 4 l .. 4 l + 3 of the three rows as one float4 each.
//   Summation order of d = sum_k x[k] (yi[k] - yj[k]), a function of D alone: per lane the chain
//   fmaf(x[e], yi[e] - yj[e], acc) over e = 0, 1, 2, 3 from acc = 0 (row4_dot); then the butterfly over the G lanes with
//   strides 1, 2, 4, ... G / 2 (v + value of lane ^ stride), which leaves the same bits in every lane of the group.
//   loss_t = softplus(-d) and g = sigmoid(-d) are logistic(-d, ..) of esr_row4.h: with e = expf(-|d|) <= 1,
//   max(-d, 0) + log1pf(e) and (-d >= 0 ? 1 : e) / (1 + e); neither branch overflows.
// A triple's outputs depend on its own three rows, reg and D only: there is no reduction across triples, no float atomic
// and no grid-wide pass; the step's loss is summed from loss_t by the caller.
#include "esr_bpr_sample.h"
#include "esr_common.h"
#include "esr_row4.h"
#include "esr_sampled.h"

namespace esr {

__global__ __launch_bounds__(kBlock) void bpr_sample_kernel(const int64_t* __restrict__ row_offsets,
                                                            const int32_t* __restrict__ row_upos,
                                                            const int32_t* __restrict__ row_ipos, int64_t nu, uint32_t ni,
                                                            uint32_t nnz, uint64_t seed, uint32_t step0, int64_t K, int64_t B,
                                                            int64_t blocks_per_step, int32_t* __restrict__ out_u,
                                                            int32_t* __restrict__ out_i, int32_t* __restrict__ out_j,
                                                            int32_t* __restrict__ out_valid, int32_t* __restrict__ dropped) {
  sample_slots(K, B, blocks_per_step, dropped, [&](int64_t k, int64_t t, int64_t at) {
    const BprTriple r = bpr_sample_triple(row_offsets, row_upos, row_ipos, nu, ni, nnz, seed, step0 + (uint32_t)k, (uint32_t)t);
    out_u[at] = r.u;
    out_i[at] = r.i;
    out_j[at] = r.j;
    out_valid[at] = r.valid;
    return r.valid != 0;
  });
}

template <int G>
__global__ __launch_bounds__(kBlock) void bpr_fwd_bwd_kernel(const float* __restrict__ user_table, int64_t nu,
                                                             const float* __restrict__ item_table, int64_t ni, int D,
                                                             const int32_t* __restrict__ us, const int32_t* __restrict__ is,
                                                             const int32_t* __restrict__ js, const int32_t* __restrict__ valid,
                                                             int64_t B, float reg, float* __restrict__ loss_t,
                                                             float* __restrict__ diff_t, float* __restrict__ grads,
                                                             int32_t* __restrict__ failed) {
  const int lig = row4_lig<G>();
  const bool holds = row4_holds(lig, D);
  const int64_t ngroups = row4_stride<G>();
  for (int64_t t = row4_first<G>(); t < B; t += ngroups) {  // (uniform per group)
    float4 gu = row4_zero(), gi = gu, gj = gu;
    float loss = 0.f, d = 0.f;
    if (!valid || valid[t] != 0) {
      const int64_t u = us[t], i = is[t], j = js[t];
      if (u < 0 || u >= nu || i < 0 || i >= ni || j < 0 || j >= ni) {
        if (lig == 0) atomicOr(failed, kFailBadPosition);
      } else {
        float4 x = gu, yi = gu, yj = gu;
        if (holds) {
          x = *row4_ptr(user_table, u, D, lig);
          yi = *row4_ptr(item_table, i, D, lig);
          yj = *row4_ptr(item_table, j, D, lig);
        }
        d = group_sum(row4_dot(x, sub4(yi, yj)), G);
        float g;
        logistic(-d, loss, g);
        triple_grads(x, yi, yj, g, reg, gu, gi, gj);
      }
    }
    if (lig == 0) {
      loss_t[t] = loss;
      if (diff_t) diff_t[t] = d;
    }
    triple_store(grads, t, B, D, lig, holds, gu, gi, gj);
  }
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_bpr_geometry(int* max_tries, int* max_rank, int* rank_multiple) {
  ESR_REQUIRE(max_tries && max_rank && rank_multiple, "esr_bpr_geometry: null pointer");
  *max_tries = kBprMaxTries;
  *max_rank = kRow4MaxRank;
  *rank_multiple = kRow4RankMultiple;
  return ESR_OK;
}

int esr_bpr_sample(const int64_t* row_offsets, const int32_t* row_upos, const int32_t* row_ipos, int64_t nu, int64_t ni,
                   int64_t nnz, uint64_t seed, uint32_t step0, int64_t K, int64_t B, int32_t* out_u, int32_t* out_i,
                   int32_t* out_j, int32_t* out_valid, int32_t* dropped, esr_stream_t stream) {
  TraceScope trace_scope_("esr_bpr_sample");
  const char* who = "esr_bpr_sample";
  if (int rc = check_sizes(who, {{"nu", nu}, {"ni", ni}, {"nnz", nnz}}, ": nnz and ni are 32-bit multiply-high factors")) return rc;
  ESR_REQUIRE(row_offsets && row_upos && row_ipos && out_u && out_i && out_j && out_valid && dropped, "%s: null pointer", who);
  ESR_REQUIRE(((uintptr_t)row_offsets & 7) == 0 && (((uintptr_t)row_upos | (uintptr_t)row_ipos | (uintptr_t)out_u |
                                                     (uintptr_t)out_i | (uintptr_t)out_j | (uintptr_t)out_valid |
                                                     (uintptr_t)dropped) & 3) == 0,
              "%s: misaligned pointer", who);
  hipStream_t st = as_stream(stream);
  int grid;
  int64_t blocks_per_step;
  if (int rc = sample_plan(who, K, B, dropped, st, grid, blocks_per_step)) return rc;
  ESR_KT("bpr_sample", st,
         hipLaunchKernelGGL(bpr_sample_kernel, dim3(grid), dim3(kBlock), 0, st, row_offsets, row_upos, row_ipos, nu,
                            (uint32_t)ni, (uint32_t)nnz, seed, step0, K, B, blocks_per_step, out_u, out_i, out_j, out_valid,
                            dropped));
  return check_launch(who);
}

int esr_bpr_fwd_bwd(const float* user_table, int64_t nu, const float* item_table, int64_t ni, int D, const int32_t* u,
                    const int32_t* i, const int32_t* j, const int32_t* valid, int64_t B, float reg, float* loss_t,
                    float* diff_t, float* grads, int32_t* failed, esr_stream_t stream) {
  TraceScope trace_scope_("esr_bpr_fwd_bwd");
  const char* who = "esr_bpr_fwd_bwd";
  if (int rc = check_rank(who, D)) return rc;
  if (int rc = check_sizes(who, {{"nu", nu}, {"ni", ni}, {"B", B}})) return rc;
  if (int rc = check_reg(who, reg)) return rc;
  ESR_REQUIRE(user_table && item_table && u && i && j && loss_t && failed, "%s: null pointer", who);
  ESR_REQUIRE((((uintptr_t)user_table | (uintptr_t)item_table | (uintptr_t)grads) & 15) == 0 &&
                  (((uintptr_t)u | (uintptr_t)i | (uintptr_t)j | (uintptr_t)valid | (uintptr_t)loss_t | (uintptr_t)diff_t |
                    (uintptr_t)failed) & 3) == 0,
              "%s: misaligned pointer (tables and grads: 16 bytes)", who);
  hipStream_t st = as_stream(stream);
  const int G = row4_lanes(D), grid = grid_for_groups(B, G);
  ESR_DISPATCH_G(G, ESR_KT("bpr_fwd_bwd", st,
                           hipLaunchKernelGGL(bpr_fwd_bwd_kernel<GG>, dim3(grid), dim3(kBlock), 0, st, user_table, nu, item_table,
                                              ni, D, u, i, j, valid, B, reg, loss_t, diff_t, grads, failed)));
  return check_launch(who);
}

}  // extern "C"
