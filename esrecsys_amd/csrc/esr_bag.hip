// Bag tables on the device: the weighted sum of feature rows that composes a user or an item of the hybrid model (Kula,
// "Metadata Embeddings for User and Item Cold-start Recommendations", 2015) and its transpose, which hands the composed rows'
// gradients back to the features as one row per occurrence for the row-sparse engine (esr_sort.hip, esr_optim.hip).  The
// rule of both is esr_bag_rule.h's; factorization.HybridBPR drives them around the unchanged esr_bpr_fwd_bwd.
//
// Layout: one selected bag per group of G lanes in the float4 row-group layout of esr_row4.h.
//
// Sum.  The group walks its bag's occurrences in ascending order; per element the chain acc = fmaf(w[k], E[feat[k], c], acc)
// from +0.0f.  The feat / weight words and the rows of kBagUnroll occurrences are loaded together before their four chain
// steps run in order: only the loads are batched.  An element is a function of its own bag and column alone.
//
// Expand.  The group of selected bag r keeps that bag's gradient row in registers and writes output rows out_offsets[r] ..
// out_offsets[r + 1] - 1 (clamped into [0, M]): output row q is occurrence off[b] + (q - out_offsets[r]).  Every output
// row of the range is written, so out_offsets that partition [0, M) leave no row unwritten; an output position without an
// occurrence (out_offsets that are not the scan of the bags' lengths) is refused like a bad position.
//
// Refusals.  A bag number outside [0, n_bags) or a feature position outside [0, nf) sets bit 30 of *failed (one integer
// atomic per group), reads no row and writes zeros: the whole row of the sum, the one output row of the expansion, whose
// out_feat is 0 so that the engine is never handed a position outside the table.
//
// The only loops are the bag's length and the grid stride; no group waits on another, no float atomic, no LDS, nothing
// polled.  Registers (hipcc -O3, gfx950, no scratch): DESIGN.md section 4l.
#include "esr_bag_rule.h"
#include "esr_common.h"
#include "esr_row4.h"

namespace esr {

__device__ __forceinline__ float4 bag_step4(float w, float4 e, float4 acc) {
  return make_float4(bag_step(w, e.x, acc.x), bag_step(w, e.y, acc.y), bag_step(w, e.z, acc.z), bag_step(w, e.w, acc.w));
}

template <int G>
__global__ __launch_bounds__(kBlock) void bag_sum_kernel(const float* __restrict__ table, int64_t nf, int D,
                                                         const int64_t* __restrict__ bag_offsets,
                                                         const int32_t* __restrict__ bag_feat,
                                                         const float* __restrict__ bag_weight, int64_t nnz, int64_t n_bags,
                                                         const int32_t* __restrict__ rows, int64_t n, float* __restrict__ out,
                                                         int32_t* __restrict__ failed) {
  const int lig = row4_lig<G>();
  const bool holds = row4_holds(lig, D);
  const int64_t ngroups = row4_stride<G>();
  for (int64_t r = row4_first<G>(); r < n; r += ngroups) {  // (uniform per group)
    const int64_t b = rows ? (int64_t)rows[r] : r;
    float4 acc = row4_zero();
    bool bad = !bag_number_ok(b, n_bags);
    if (!bad) {
      const BagSpan s = bag_span(bag_offsets, b, nnz);
      int64_t k = s.lo;
      for (; k + kBagUnroll <= s.hi; k += kBagUnroll) {
        int64_t f[kBagUnroll];
        float w[kBagUnroll];
        float4 e[kBagUnroll];
#pragma unroll
        for (int q = 0; q < kBagUnroll; ++q) {
          f[q] = bag_feat[k + q];
          w[q] = bag_weight ? bag_weight[k + q] : 1.0f;
        }
#pragma unroll
        for (int q = 0; q < kBagUnroll; ++q) {
          const bool ok = bag_feat_ok(f[q], nf);
          bad |= !ok;
          e[q] = row4_load(table, f[q], D, lig, ok && holds);
        }
#pragma unroll
        for (int q = 0; q < kBagUnroll; ++q) acc = bag_step4(w[q], e[q], acc);
      }
      for (; k < s.hi; ++k) {
        const int64_t f = bag_feat[k];
        const float w = bag_weight ? bag_weight[k] : 1.0f;
        const bool ok = bag_feat_ok(f, nf);
        bad |= !ok;
        acc = bag_step4(w, row4_load(table, f, D, lig, ok && holds), acc);
      }
    }
    if (bad) {
      acc = row4_zero();
      if (lig == 0) atomicOr(failed, kBagFailBad);
    }
    row4_store(out, r, D, lig, holds, acc);
  }
}

template <int G>
__global__ __launch_bounds__(kBlock) void bag_expand_kernel(const float* __restrict__ table, int64_t nf, int D,
                                                            const int64_t* __restrict__ bag_offsets,
                                                            const int32_t* __restrict__ bag_feat,
                                                            const float* __restrict__ bag_weight, int64_t nnz, int64_t n_bags,
                                                            const int32_t* __restrict__ rows,
                                                            const float* __restrict__ grad_rows,
                                                            const int32_t* __restrict__ valid,
                                                            const int64_t* __restrict__ out_offsets, int64_t n, int64_t M,
                                                            float reg, int32_t* __restrict__ out_feat,
                                                            float* __restrict__ out_grads, int32_t* __restrict__ failed) {
  const int lig = row4_lig<G>();
  const bool holds = row4_holds(lig, D);
  const int64_t ngroups = row4_stride<G>();
  for (int64_t r = row4_first<G>(); r < n; r += ngroups) {  // (uniform per group)
    const int64_t b = rows ? (int64_t)rows[r] : r;
    int64_t q0 = out_offsets[r], q1 = out_offsets[r + 1];
    q0 = q0 < 0 ? 0 : (q0 > M ? M : q0);
    q1 = q1 < q0 ? q0 : (q1 > M ? M : q1);
    BagSpan s;
    s.lo = s.hi = 0;
    bool bad = !bag_number_ok(b, n_bags);
    if (!bad) s = bag_span(bag_offsets, b, nnz);
    bad |= (s.hi - s.lo) != (q1 - q0);  // (a bad bag number with no output rows is still refused: the first test stands)
    const bool live = !valid || valid[r] != 0;
    float4 g = row4_zero();
    if (live && holds) g = *row4_ptr(grad_rows, r, D, lig);
    for (int64_t q = q0; q < q1; ++q) {
      const int64_t k = s.lo + (q - q0);
      int64_t f = 0;
      float4 o = row4_zero();
      if (k < s.hi) {
        f = bag_feat[k];
        if (!bag_feat_ok(f, nf)) {
          bad = true;
          f = 0;
        } else if (live && holds) {
          const float w = bag_weight ? bag_weight[k] : 1.0f;
          const float4 e = *row4_ptr(table, f, D, lig);
          o = make_float4(bag_expand_elem(w, g.x, reg, e.x), bag_expand_elem(w, g.y, reg, e.y),
                          bag_expand_elem(w, g.z, reg, e.z), bag_expand_elem(w, g.w, reg, e.w));
        }
      }
      if (lig == 0) out_feat[q] = (int32_t)f;
      // (row4_store's text, spelled out: through the helper this loop's address arithmetic is scheduled differently)
      if (holds) *reinterpret_cast<float4*>(out_grads + q * D + 4 * lig) = o;
    }
    if (bad && lig == 0) atomicOr(failed, kBagFailBad);
  }
}

// what the two entry points check alike; 0 when the arguments stand
static int bag_table_args(const char* who, const float* table, int64_t nf, int D, const int64_t* bag_offsets,
                          const int32_t* bag_feat, const float* bag_weight, int64_t nnz, int64_t n_bags, const int32_t* rows,
                          int64_t n, int32_t* failed) {
  ESR_REQUIRE(D >= kBagRankMultiple && D <= kBagMaxRank && D % kBagRankMultiple == 0,
              "%s: D=%d is not a multiple of %d in [%d, %d]", who, D, kBagRankMultiple, kBagRankMultiple, kBagMaxRank);
  ESR_REQUIRE(nf >= 1 && nf <= (int64_t)INT32_MAX && nnz >= 1 && nnz <= (int64_t)INT32_MAX && n_bags >= 1 &&
                  n_bags <= (int64_t)INT32_MAX && n >= 0 && n <= (int64_t)INT32_MAX,
              "%s: bad sizes nf=%lld nnz=%lld n_bags=%lld n=%lld (each in [1, 2^31 - 1]; n may be 0)", who, (long long)nf,
              (long long)nnz, (long long)n_bags, (long long)n);
  ESR_REQUIRE(table && bag_offsets && bag_feat && failed, "%s: null pointer", who);
  ESR_REQUIRE(((uintptr_t)table & 15) == 0 && ((uintptr_t)bag_offsets & 7) == 0 &&
                  (((uintptr_t)bag_feat | (uintptr_t)bag_weight | (uintptr_t)rows | (uintptr_t)failed) & 3) == 0,
              "%s: misaligned pointer (tables and row outputs: 16 bytes, int64 arrays: 8)", who);
  return ESR_OK;
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_bag_geometry(int* max_rank, int* rank_multiple) {
  ESR_REQUIRE(max_rank && rank_multiple, "esr_bag_geometry: null pointer");
  *max_rank = kBagMaxRank;
  *rank_multiple = kBagRankMultiple;
  return ESR_OK;
}

int esr_bag_sum(const float* table, int64_t nf, int D, const int64_t* bag_offsets, const int32_t* bag_feat,
                const float* bag_weight, int64_t nnz, int64_t n_bags, const int32_t* rows, int64_t n, float* out,
                int32_t* failed, esr_stream_t stream) {
  TraceScope trace_scope_("esr_bag_sum");
  const char* who = "esr_bag_sum";
  if (int rc = bag_table_args(who, table, nf, D, bag_offsets, bag_feat, bag_weight, nnz, n_bags, rows, n, failed)) return rc;
  ESR_REQUIRE(out, "%s: null pointer", who);
  ESR_REQUIRE(((uintptr_t)out & 15) == 0, "%s: misaligned pointer (tables and row outputs: 16 bytes, int64 arrays: 8)", who);
  ESR_REQUIRE(rows || n <= n_bags, "%s: n=%lld exceeds n_bags=%lld without rows", who, (long long)n, (long long)n_bags);
  if (n == 0) return ESR_OK;
  hipStream_t st = as_stream(stream);
  const int G = row4_lanes(D), grid = grid_for_groups(n, G);
  ESR_DISPATCH_G(G, ESR_KT("bag_sum", st,
                           hipLaunchKernelGGL(bag_sum_kernel<GG>, dim3(grid), dim3(kBlock), 0, st, table, nf, D, bag_offsets,
                                              bag_feat, bag_weight, nnz, n_bags, rows, n, out, failed)));
  return check_launch(who);
}

int esr_bag_expand(const float* table, int64_t nf, int D, const int64_t* bag_offsets, const int32_t* bag_feat,
                   const float* bag_weight, int64_t nnz, int64_t n_bags, const int32_t* rows, const float* grad_rows,
                   const int32_t* valid, const int64_t* out_offsets, int64_t n, int64_t M, float reg, int32_t* out_feat,
                   float* out_grads, int32_t* failed, esr_stream_t stream) {
  TraceScope trace_scope_("esr_bag_expand");
  const char* who = "esr_bag_expand";
  if (int rc = bag_table_args(who, table, nf, D, bag_offsets, bag_feat, bag_weight, nnz, n_bags, rows, n, failed)) return rc;
  ESR_REQUIRE(M >= 0 && M <= (int64_t)INT32_MAX, "%s: bad sizes M=%lld (the expanded occurrences, in [0, 2^31 - 1])", who,
              (long long)M);
  ESR_REQUIRE(reg >= 0.f && reg <= 3.0e38f, "%s: reg=%g must be finite and not negative", who, (double)reg);
  ESR_REQUIRE(grad_rows && out_offsets && (M == 0 || (out_feat && out_grads)), "%s: null pointer", who);
  ESR_REQUIRE((((uintptr_t)grad_rows | (uintptr_t)out_grads) & 15) == 0 && ((uintptr_t)out_offsets & 7) == 0 &&
                  (((uintptr_t)valid | (uintptr_t)out_feat) & 3) == 0,
              "%s: misaligned pointer (tables and row outputs: 16 bytes, int64 arrays: 8)", who);
  ESR_REQUIRE(rows || n <= n_bags, "%s: n=%lld exceeds n_bags=%lld without rows", who, (long long)n, (long long)n_bags);
  if (n == 0) return ESR_OK;
  hipStream_t st = as_stream(stream);
  const int G = row4_lanes(D), grid = grid_for_groups(n, G);
  ESR_DISPATCH_G(G, ESR_KT("bag_expand", st,
                           hipLaunchKernelGGL(bag_expand_kernel<GG>, dim3(grid), dim3(kBlock), 0, st, table, nf, D, bag_offsets,
                                              bag_feat, bag_weight, nnz, n_bags, rows, grad_rows, valid, out_offsets, n, M, reg,
                                              out_feat, out_grads, failed)));
  return check_launch(who);
}

}  // extern "C"
