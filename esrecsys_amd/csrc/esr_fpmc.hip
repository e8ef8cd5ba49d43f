// Factorised Personalised Markov Chain (Rendle, Freudenthaler, Schmidt-Thieme, WWW 2010) trained with the BPR step on the
// device: the slot sampler and the fused logistic forward / backward over 5 + c gathered rows.  The update itself is the
// row-sparse engine (esr_sort.hip, esr_optim.hip) driven from factorization.FPMC.
//
// Model.  score(u, event, i) = U_u . A_i + m . Bn_i, m the bag (esr_bag_rule.h) of the c <= 8 items just before the
// event, oldest first, every weight w = 1.0f / c:  m = fmaf(w, P[l], m) from +0.0f over the context in order.
//
// Sampler.  One lane per slot; the rule is fpmc_sample_slot (esr_fpmc_sample.h), a function of (seed, step, slot, the two
// CSRs, window) alone, inside the sampler shell of esr_sampled.h (sample_slots).  Integer arithmetic only; the only loops
// are BPR's 15 candidates and 31-probe binary search (bpr_walk_negative); no workgroup waits on another, nothing is polled.
//
// Forward / backward.  One slot per group of G lanes in the float4 row-group layout of esr_row4.h.  The group reads its
// slot's words and its c context ids, then issues the 5 + c row loads (at most 13 float4 per lane) before the first use:
// a gather kernel of this shape lives on the loads it keeps in flight.
//   Summation order of d, a function of D alone: per lane from acc = 0 the chain fmaf(x[e], a_i[e] - a_j[e], acc) over
//   e = 0 .. 3, then fmaf(m[e], bn_i[e] - bn_j[e], acc) over e = 0 .. 3 (two row4_dot, the second on from the first); then
//   the butterfly of group_sum over the G lanes.  loss_t and g = sigmoid(-d) are logistic(-d, ..) of esr_row4.h.
//   Rows: triple_grads(x, a_i, a_j, g, reg) for U_u, A_i, A_j; triple_grads(m, bn_i, bn_j, g, reg) for Bn_i, Bn_j, and its
//   first output with reg = 0 is g_m; context occurrence n gets bag_expand_elem(w, g_m, reg, P[l_n]) per element.
// Occurrence n of slot t is row 5 B + ctx_offsets[t] + n of grads and entry ctx_offsets[t] + n of ctx_ids; the caller
// hands in ctx_offsets = the exclusive scan of c (the convention of esr_bag_expand).  Every row of a slot's range is
// written whatever becomes of the slot: valid = 0 gives zero rows under the real ids, so the layout is the draw's alone.
// A slot's outputs depend on its own rows, reg and D only: no reduction across slots, no float atomic, no LDS, no
// scratch, no grid-wide pass; the step's loss is summed from loss_t by the caller.
#include "esr_bag_rule.h"
#include "esr_common.h"
#include "esr_fpmc_sample.h"
#include "esr_row4.h"
#include "esr_sampled.h"

namespace esr {

__global__ __launch_bounds__(kBlock) void fpmc_sample_kernel(
    const int64_t* __restrict__ seq_offsets, const int32_t* __restrict__ seq_upos, const int32_t* __restrict__ seq_ipos,
    uint32_t nnz_seq, const int64_t* __restrict__ row_offsets, const int32_t* __restrict__ row_ipos, int64_t nnz_seen,
    int64_t nu, uint32_t ni, int window, uint64_t seed, uint32_t step0, int64_t K, int64_t B, int64_t blocks_per_step,
    int32_t* __restrict__ out_u, int32_t* __restrict__ out_e, int32_t* __restrict__ out_c, int32_t* __restrict__ out_i,
    int32_t* __restrict__ out_j, int32_t* __restrict__ out_valid, int32_t* __restrict__ dropped) {
  sample_slots(K, B, blocks_per_step, dropped, [&](int64_t k, int64_t t, int64_t at) {
    const FpmcSlot r = fpmc_sample_slot(seq_offsets, seq_upos, seq_ipos, nnz_seq, row_offsets, row_ipos, nnz_seen, nu, ni,
                                        window, seed, step0 + (uint32_t)k, (uint32_t)t);
    out_u[at] = r.u;
    out_e[at] = r.e;
    out_c[at] = r.c;
    out_i[at] = r.i;
    out_j[at] = r.j;
    out_valid[at] = r.valid;
    return r.valid != 0;
  });
}

__device__ __forceinline__ float4 fpmc_step4(float w, float4 e, float4 acc) {
  return make_float4(bag_step(w, e.x, acc.x), bag_step(w, e.y, acc.y), bag_step(w, e.z, acc.z), bag_step(w, e.w, acc.w));
}

template <int G>
__global__ __launch_bounds__(kBlock) void fpmc_fwd_bwd_kernel(
    const float* __restrict__ user_table, int64_t nu, const float* __restrict__ item_table,
    const float* __restrict__ next_table, const float* __restrict__ prev_table, int64_t ni, int D,
    const int32_t* __restrict__ seq_ipos, int64_t nnz_seq, const int32_t* __restrict__ us, const int32_t* __restrict__ es,
    const int32_t* __restrict__ cs, const int32_t* __restrict__ is, const int32_t* __restrict__ js,
    const int32_t* __restrict__ valid, int64_t B, const int64_t* __restrict__ ctx_offsets, int64_t M, float reg,
    float* __restrict__ loss_t, float* __restrict__ diff_t, float* __restrict__ grads, int32_t* __restrict__ ctx_ids,
    int32_t* __restrict__ failed) {
  const int lig = row4_lig<G>();
  const bool holds = row4_holds(lig, D);
  const int64_t ngroups = row4_stride<G>();
  for (int64_t t = row4_first<G>(); t < B; t += ngroups) {  // (uniform per group)
    const int64_t u = us[t], e = es[t], i = is[t], j = js[t];
    int c = cs[t];
    int64_t q0 = 0, q1 = 0;
    if (grads) {
      q0 = ctx_offsets[t], q1 = ctx_offsets[t + 1];
      q0 = q0 < 0 ? 0 : (q0 > M ? M : q0);
      q1 = q1 < q0 ? q0 : (q1 > M ? M : q1);
    }
    // the slot's own words: an event outside the sequences, a context that is longer than the window, reaches before
    // event 0 or does not fill its range of output rows is refused like a position outside its table (and reads nothing)
    bool bad = e < 0 || e >= nnz_seq || c < 0 || c > kFpmcMaxWindow || (int64_t)c > e || (grads && q1 - q0 != (int64_t)c);
    if (bad) c = 0;
    int64_t l[kFpmcMaxWindow];
#pragma unroll
    for (int n = 0; n < kFpmcMaxWindow; ++n) {
      l[n] = n < c ? (int64_t)seq_ipos[e - c + n] : 0;
      if (l[n] < 0 || l[n] >= ni) {
        bad = true;
        l[n] = 0;
      }
    }
    bad |= u < 0 || u >= nu || i < 0 || i >= ni || j < 0 || j >= ni;
    const bool live = !bad && (!valid || valid[t] != 0);
    float4 gu = row4_zero(), gai = gu, gaj = gu, gbi = gu, gbj = gu, gm = gu;
    float4 p[kFpmcMaxWindow];
    float loss = 0.f, d = 0.f, w = 0.f;
    if (live) {
      float4 x = gu, ai = gu, aj = gu, bi = gu, bj = gu;
      if (holds) {
        x = *row4_ptr(user_table, u, D, lig);
        ai = *row4_ptr(item_table, i, D, lig);
        aj = *row4_ptr(item_table, j, D, lig);
        bi = *row4_ptr(next_table, i, D, lig);
        bj = *row4_ptr(next_table, j, D, lig);
      }
#pragma unroll
      for (int n = 0; n < kFpmcMaxWindow; ++n) p[n] = row4_load(prev_table, l[n], D, lig, holds && n < c);
      if (c > 0) w = __fdiv_rn(1.0f, (float)c);
      float4 m = row4_zero();
#pragma unroll
      for (int n = 0; n < kFpmcMaxWindow; ++n)
        if (n < c) m = fpmc_step4(w, p[n], m);
      d = group_sum(row4_dot(m, sub4(bi, bj), row4_dot(x, sub4(ai, aj))), G);
      float g;
      logistic(-d, loss, g);
      triple_grads(x, ai, aj, g, reg, gu, gai, gaj);
      float4 unused_i, unused_j;
      triple_grads(m, bi, bj, g, 0.f, gm, unused_i, unused_j);
      float4 unused_m;
      triple_grads(m, bi, bj, g, reg, unused_m, gbi, gbj);
    }
    if (lig == 0) {
      loss_t[t] = loss;
      if (diff_t) diff_t[t] = d;
      if (bad) atomicOr(failed, kFailBadPosition);
    }
    if (grads) {
      triple_store(grads, t, B, D, lig, holds, gu, gai, gaj);
      row4_store(grads, 3 * B + t, D, lig, holds, gbi);
      row4_store(grads, 4 * B + t, D, lig, holds, gbj);
      float* rows = grads + 5 * B * D;
#pragma unroll
      for (int n = 0; n < kFpmcMaxWindow; ++n) {
        const int64_t q = q0 + n;
        if (q < q1) {
          float4 o = row4_zero();
          if (live && n < c)
            o = make_float4(bag_expand_elem(w, gm.x, reg, p[n].x), bag_expand_elem(w, gm.y, reg, p[n].y),
                            bag_expand_elem(w, gm.z, reg, p[n].z), bag_expand_elem(w, gm.w, reg, p[n].w));
          if (lig == 0) ctx_ids[q] = (int32_t)l[n];
          row4_store(rows, q, D, lig, holds, o);
        }
      }
      // (a range longer than the window -- ctx_offsets that are not the scan of c -- was refused above: zeros under id 0)
      for (int64_t q = q0 + kFpmcMaxWindow; q < q1; ++q) {
        if (lig == 0) ctx_ids[q] = 0;
        row4_store(rows, q, D, lig, holds, row4_zero());
      }
    }
  }
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_fpmc_geometry(int* max_window, int* max_rank, int* rank_multiple) {
  ESR_REQUIRE(max_window && max_rank && rank_multiple, "esr_fpmc_geometry: null pointer");
  *max_window = kFpmcMaxWindow;
  *max_rank = kRow4MaxRank;
  *rank_multiple = kRow4RankMultiple;
  return ESR_OK;
}

int esr_fpmc_sample(const int64_t* seq_offsets, const int32_t* seq_upos, const int32_t* seq_ipos, int64_t nnz_seq,
                    const int64_t* row_offsets, const int32_t* row_ipos, int64_t nnz_seen, int64_t nu, int64_t ni, int window,
                    uint64_t seed, uint32_t step0, int64_t K, int64_t B, int32_t* out_u, int32_t* out_e, int32_t* out_c,
                    int32_t* out_i, int32_t* out_j, int32_t* out_valid, int32_t* dropped, esr_stream_t stream) {
  TraceScope trace_scope_("esr_fpmc_sample");
  const char* who = "esr_fpmc_sample";
  if (int rc = check_sizes(who, {{"nu", nu}, {"ni", ni}, {"nnz_seq", nnz_seq}, {"nnz_seen", nnz_seen}},
                           ": nnz_seq and ni are 32-bit multiply-high factors"))
    return rc;
  ESR_REQUIRE(nu + 3 * ni <= (int64_t)INT32_MAX, "%s: nu + 3 ni = %lld exceeds 2^31 - 1 (the virtual row space of the update)",
              who, (long long)(nu + 3 * ni));
  ESR_REQUIRE(window >= 1 && window <= kFpmcMaxWindow, "%s: window=%d outside [1, %d]", who, window, kFpmcMaxWindow);
  ESR_REQUIRE(seq_offsets && seq_upos && seq_ipos && row_offsets && row_ipos && out_u && out_e && out_c && out_i && out_j &&
                  out_valid && dropped,
              "%s: null pointer", who);
  ESR_REQUIRE((((uintptr_t)seq_offsets | (uintptr_t)row_offsets) & 7) == 0 &&
                  (((uintptr_t)seq_upos | (uintptr_t)seq_ipos | (uintptr_t)row_ipos | (uintptr_t)out_u | (uintptr_t)out_e |
                    (uintptr_t)out_c | (uintptr_t)out_i | (uintptr_t)out_j | (uintptr_t)out_valid | (uintptr_t)dropped) & 3) == 0,
              "%s: misaligned pointer (int64 arrays: 8 bytes)", who);
  hipStream_t st = as_stream(stream);
  int grid;
  int64_t blocks_per_step;
  if (int rc = sample_plan(who, K, B, dropped, st, grid, blocks_per_step)) return rc;
  ESR_KT("fpmc_sample", st,
         hipLaunchKernelGGL(fpmc_sample_kernel, dim3(grid), dim3(kBlock), 0, st, seq_offsets, seq_upos, seq_ipos,
                            (uint32_t)nnz_seq, row_offsets, row_ipos, nnz_seen, nu, (uint32_t)ni, window, seed, step0, K, B,
                            blocks_per_step, out_u, out_e, out_c, out_i, out_j, out_valid, dropped));
  return check_launch(who);
}

int esr_fpmc_fwd_bwd(const float* user_table, int64_t nu, const float* item_table, const float* next_table,
                     const float* prev_table, int64_t ni, int D, const int32_t* seq_ipos, int64_t nnz_seq, const int32_t* u,
                     const int32_t* e, const int32_t* c, const int32_t* i, const int32_t* j, const int32_t* valid, int64_t B,
                     const int64_t* ctx_offsets, int64_t M, float reg, float* loss_t, float* diff_t, float* grads,
                     int32_t* ctx_ids, int32_t* failed, esr_stream_t stream) {
  TraceScope trace_scope_("esr_fpmc_fwd_bwd");
  const char* who = "esr_fpmc_fwd_bwd";
  if (int rc = check_rank(who, D)) return rc;
  if (int rc = check_sizes(who, {{"nu", nu}, {"ni", ni}, {"nnz_seq", nnz_seq}, {"B", B}})) return rc;
  ESR_REQUIRE(nu + 3 * ni <= (int64_t)INT32_MAX, "%s: nu + 3 ni = %lld exceeds 2^31 - 1 (the virtual row space of the update)",
              who, (long long)(nu + 3 * ni));
  ESR_REQUIRE(M >= 0 && M <= (int64_t)INT32_MAX, "%s: bad sizes M=%lld (the context occurrences, in [0, 2^31 - 1])", who,
              (long long)M);
  if (int rc = check_reg(who, reg)) return rc;
  ESR_REQUIRE(user_table && item_table && next_table && prev_table && seq_ipos && u && e && c && i && j && loss_t && failed,
              "%s: null pointer", who);
  ESR_REQUIRE(!grads || (ctx_offsets && (M == 0 || ctx_ids)), "%s: null pointer (grads without ctx_offsets or ctx_ids)", who);
  ESR_REQUIRE((((uintptr_t)user_table | (uintptr_t)item_table | (uintptr_t)next_table | (uintptr_t)prev_table |
                (uintptr_t)grads) & 15) == 0 &&
                  ((uintptr_t)ctx_offsets & 7) == 0 &&
                  (((uintptr_t)seq_ipos | (uintptr_t)u | (uintptr_t)e | (uintptr_t)c | (uintptr_t)i | (uintptr_t)j |
                    (uintptr_t)valid | (uintptr_t)loss_t | (uintptr_t)diff_t | (uintptr_t)ctx_ids | (uintptr_t)failed) & 3) == 0,
              "%s: misaligned pointer (tables and grads: 16 bytes, ctx_offsets: 8)", who);
  hipStream_t st = as_stream(stream);
  const int G = row4_lanes(D), grid = grid_for_groups(B, G);
  ESR_DISPATCH_G(G, ESR_KT("fpmc_fwd_bwd", st,
                           hipLaunchKernelGGL(fpmc_fwd_bwd_kernel<GG>, dim3(grid), dim3(kBlock), 0, st, user_table, nu,
                                              item_table, next_table, prev_table, ni, D, seq_ipos, nnz_seq, u, e, c, i, j,
                                              valid, B, ctx_offsets, M, reg, loss_t, diff_t, grads, ctx_ids, failed)));
  return check_launch(who);
}

}  // extern "C"
