// Bayesian Personalised Ranking (Rendle, Freudenthaler, Gantner, Schmidt-Thieme, UAI 2009) on the device: the triple
// sampler and the fused logistic forward / backward over three gathered rows.  The update itself is the row-sparse engine
// (esr_sort.hip, esr_optim.hip) driven from factorization.BPR.
//
// Sampler.  One lane per triple; the rule is bpr_sample_triple (esr_bpr_sample.h), a function of (seed, step, slot, CSR)
// alone.  A workgroup serves 256 consecutive slots of ONE step, so the invalid triples of a wave are counted with a ballot
// and added to dropped[k] by one integer atomic per wave.  Integer arithmetic only; the only loops are the 15 candidates
// and the 31-probe binary search; no workgroup waits on another and nothing is polled.
//
// Forward / backward.  One triple per group of G lanes in the float4 row-group layout of esr_row4.h: lane l of the group
// holds elements 4 l .. 4 l + 3 of the three rows as one float4 each.
//   Summation order of d = sum_k x[k] (yi[k] - yj[k]), a function of D alone: per lane the chain
//   fmaf(x[e], yi[e] - yj[e], acc) over e = 0, 1, 2, 3 from acc = 0; then the butterfly over the G lanes with strides
//   1, 2, 4, ... G / 2 (v + value of lane ^ stride), which leaves the same bits in every lane of the group.
//   loss_t = max(-d, 0) + log1pf(expf(-|d|)), g = sigmoid(-d) = (d >= 0 ? e : 1) / (1 + e) with e = expf(-|d|) <= 1:
//   neither branch overflows; expf / log1pf are the precise forms.
// A triple's outputs depend on its own three rows, reg and D only: there is no reduction across triples, no float atomic
// and no grid-wide pass; the step's loss is summed from loss_t by the caller.
#include "esr_bpr_sample.h"
#include "esr_common.h"
#include "esr_row4.h"

namespace esr {

constexpr int kBprFailBadPosition = 1 << 30;  // as FAIL_BAD_POSITION of esr_als.hip
constexpr int64_t kBprMaxSampleBlocks = (int64_t)kMaxGrid * 16;

__global__ __launch_bounds__(kBlock) void bpr_sample_kernel(const int64_t* __restrict__ row_offsets,
                                                            const int32_t* __restrict__ row_upos,
                                                            const int32_t* __restrict__ row_ipos, int64_t nu, uint32_t ni,
                                                            uint32_t nnz, uint64_t seed, uint32_t step0, int64_t K, int64_t B,
                                                            int64_t blocks_per_step, int32_t* __restrict__ out_u,
                                                            int32_t* __restrict__ out_i, int32_t* __restrict__ out_j,
                                                            int32_t* __restrict__ out_valid, int32_t* __restrict__ dropped) {
  const int64_t nblocks = K * blocks_per_step;
  for (int64_t w = blockIdx.x; w < nblocks; w += gridDim.x) {  // (uniform per workgroup)
    const int64_t k = w / blocks_per_step, t = (w % blocks_per_step) * kBlock + threadIdx.x;
    bool bad = false;
    if (t < B) {
      const BprTriple r = bpr_sample_triple(row_offsets, row_upos, row_ipos, nu, ni, nnz, seed, step0 + (uint32_t)k, (uint32_t)t);
      const int64_t at = k * B + t;
      out_u[at] = r.u;
      out_i[at] = r.i;
      out_j[at] = r.j;
      out_valid[at] = r.valid;
      bad = !r.valid;
    }
    const unsigned long long mask = __ballot(bad);
    if ((threadIdx.x & (kWave - 1)) == 0 && mask) atomicAdd(dropped + k, (int32_t)__popcll(mask));
  }
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
        if (lig == 0) atomicOr(failed, kBprFailBadPosition);
      } else {
        float4 x = gu, yi = gu, yj = gu;
        if (holds) {
          x = *row4_ptr(user_table, u, D, lig);
          yi = *row4_ptr(item_table, i, D, lig);
          yj = *row4_ptr(item_table, j, D, lig);
        }
        const float4 df = make_float4(yi.x - yj.x, yi.y - yj.y, yi.z - yj.z, yi.w - yj.w);
        float acc = __fmaf_rn(x.x, df.x, 0.f);
        acc = __fmaf_rn(x.y, df.y, acc);
        acc = __fmaf_rn(x.z, df.z, acc);
        acc = __fmaf_rn(x.w, df.w, acc);
        d = group_sum(acc, G);
        const float e = expf(-fabsf(d));
        loss = fmaxf(-d, 0.f) + log1pf(e);
        const float g = __fdiv_rn(d >= 0.f ? e : 1.0f, 1.0f + e);  // sigmoid(-d)
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
  ESR_REQUIRE(nnz >= 1 && nnz <= (int64_t)INT32_MAX && ni >= 1 && ni <= (int64_t)INT32_MAX && nu >= 1 &&
                  nu <= (int64_t)INT32_MAX,
              "%s: bad sizes nu=%lld ni=%lld nnz=%lld (each in [1, 2^31 - 1]: nnz and ni are 32-bit multiply-high factors)", who,
              (long long)nu, (long long)ni, (long long)nnz);
  ESR_REQUIRE(K >= 1 && K <= (int64_t)INT32_MAX && B >= 1 && B <= (int64_t)INT32_MAX,
              "%s: bad sizes K=%lld B=%lld (each in [1, 2^31 - 1])", who, (long long)K, (long long)B);
  ESR_REQUIRE(row_offsets && row_upos && row_ipos && out_u && out_i && out_j && out_valid && dropped, "%s: null pointer", who);
  ESR_REQUIRE(((uintptr_t)row_offsets & 7) == 0 && (((uintptr_t)row_upos | (uintptr_t)row_ipos | (uintptr_t)out_u |
                                                     (uintptr_t)out_i | (uintptr_t)out_j | (uintptr_t)out_valid |
                                                     (uintptr_t)dropped) & 3) == 0,
              "%s: misaligned pointer", who);
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(dropped, 0, (size_t)K * sizeof(int32_t), st) != hipSuccess) return check_launch(who);
  const int64_t blocks_per_step = cdiv(B, kBlock);
  // (K * blocks_per_step < 2^31 * 2^23: no overflow)
  const int grid = (int)std::min<int64_t>(K * blocks_per_step, kBprMaxSampleBlocks);
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
  ESR_REQUIRE(D >= kRow4RankMultiple && D <= kRow4MaxRank && D % kRow4RankMultiple == 0,
              "%s: D=%d is not a multiple of %d in [%d, %d]", who, D, kRow4RankMultiple, kRow4RankMultiple, kRow4MaxRank);
  ESR_REQUIRE(nu >= 1 && nu <= (int64_t)INT32_MAX && ni >= 1 && ni <= (int64_t)INT32_MAX && B >= 1 && B <= (int64_t)INT32_MAX,
              "%s: bad sizes nu=%lld ni=%lld B=%lld (each in [1, 2^31 - 1])", who, (long long)nu, (long long)ni, (long long)B);
  ESR_REQUIRE(reg >= 0.f && reg <= 3.0e38f, "%s: reg=%g must be finite and not negative", who, (double)reg);
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
