// Skip-gram with negative sampling (Mikolov, Sutskever, Chen, Corrado, Dean, NIPS 2013; item2vec, Barkan and Koenigstein
// 2016) on the device: the slot sampler and the fused logistic forward / backward over 2 + K gathered rows.  The update
// itself is the row-sparse engine (esr_sort.hip, esr_optim.hip) driven from factorization.SGNS.
//
// Model.  Two tables of ni rows: in_table holds the centre vectors v, out_table the context vectors w.  A slot is a centre
// c, a context item o and K <= 16 noise items n_k;  s_o = v_c . w_o,  s_k = v_c . w_{n_k},  m_k = (n_k != o), and
//   loss_t = softplus(-s_o) + sum_k m_k softplus(s_k)          (the L2 term enters the gradient rows only, as in BPR).
//
// Sampler.  One lane per slot; the rule is sgns_sample_slot (esr_sgns_sample.h), a function of (seed, step, slot, the
// sequence CSR, window, K, the noise table) alone, inside the sampler shell of esr_sampled.h (sample_slots).  Integer
// arithmetic only; the only loops are the window's turns and the K noise items; no workgroup waits on another, nothing is
// polled.
//
// Forward / backward.  One slot per group of G lanes in the float4 row-group layout of esr_row4.h.  The group reads its
// slot's 2 + K ids, then issues the 2 + K row loads (at most 18 float4 per lane) before the first use: a gather kernel of
// this shape lives on the loads it keeps in flight.
//   A score, a function of D alone: per lane from acc = 0 the chain fmaf(v[e], w[e], acc) over e = 0 .. 3 (row4_dot), then
//   the butterfly of group_sum over the G lanes.
//   logistic of esr_row4.h: with ex = expf(-|s|), softplus(s) = max(s, 0) + log1pf(ex), sigmoid(s) = (s >= 0 ? 1 : ex) /
//   (1 + ex); the positive takes both at -s_o, so a_o = -sigmoid(-s_o) = sigmoid(s_o) - 1 and a_k = m_k sigmoid(s_k).
//   Order within a slot: the positive, then k ascending.  loss = softplus(-s_o), then loss += softplus(s_k) where m_k;
//   g_c = a_o * w_o, then g_c = fmaf(a_k, w_k, g_c) where m_k, last g_c = fmaf(reg, v, g_c), per element;
//   g_o = fmaf(a_o, v, reg * w_o);  g_n_k = fmaf(a_k, v, reg * w_k) where m_k, else zeros.
// grads is [centre rows ; positive rows ; noise rows k-major]: noise item k of slot t is row (2 + k) B + t.  valid = 0
// gives zero rows, zero loss and zero scores and reads no table row; an id outside [0, ni) sets bit 30 of *failed whatever
// valid says, and that slot gives zeros too.  A slot's outputs depend on its own rows, reg, K and D only: no reduction
// across slots, no float atomic, no LDS, no scratch, no grid-wide pass; the step's loss is summed from loss_t by the caller.
#include "esr_common.h"
#include "esr_row4.h"
#include "esr_sampled.h"
#include "esr_sgns_sample.h"

namespace esr {

__global__ __launch_bounds__(kBlock) void sgns_sample_kernel(
    const int64_t* __restrict__ seq_offsets, const int32_t* __restrict__ seq_upos, const int32_t* __restrict__ seq_ipos,
    uint32_t nnz_seq, int64_t nd, uint32_t ni, int window, int K, const uint32_t* __restrict__ noise_keep,
    const int32_t* __restrict__ noise_alias, uint64_t seed, uint32_t step0, int64_t steps, int64_t B,
    int64_t blocks_per_step, int32_t* __restrict__ out_c, int32_t* __restrict__ out_e, int32_t* __restrict__ out_o,
    int32_t* __restrict__ out_valid, int32_t* __restrict__ out_neg, int32_t* __restrict__ dropped) {
  sample_slots(steps, B, blocks_per_step, dropped, [&](int64_t k, int64_t t, int64_t at) {
    const SgnsSlot r = sgns_sample_slot(seq_offsets, seq_upos, seq_ipos, nnz_seq, nd, ni, window, K, noise_keep, noise_alias,
                                        seed, step0 + (uint32_t)k, (uint32_t)t, out_neg + at * K);
    out_c[at] = r.c;
    out_e[at] = r.e;
    out_o[at] = r.o;
    out_valid[at] = r.valid;
    return r.valid != 0;
  });
}

// K is a template argument: with K in a register every guard k < K of the three unrolled loops became a lane mask or a
// select that the compiler kept alive across the kernel (201 VGPRs, a hundred scalar registers parked in vector lanes).
// As built: no scratch and no VGPR spill at any (G, K); about 40 + 9 K VGPRs, so under 128 up to K = 9 (74 to 82 at K = 5)
// and 185 at K = 16, where two waves per SIMD remain.  Forcing four waves there (launch bounds) spills: not done.
template <int G, int K>
__global__ __launch_bounds__(kBlock) void sgns_fwd_bwd_kernel(
    const float* __restrict__ in_table, const float* __restrict__ out_table, int64_t ni, int D,
    const int32_t* __restrict__ cs, const int32_t* __restrict__ os, const int32_t* __restrict__ negs,
    const int32_t* __restrict__ valid, int64_t B, float reg, float* __restrict__ loss_t, float* __restrict__ diff_t,
    float* __restrict__ grads, int32_t* __restrict__ failed) {
  const int lig = row4_lig<G>();
  const bool holds = row4_holds(lig, D);
  const int64_t ngroups = row4_stride<G>();
  for (int64_t t = row4_first<G>(); t < B; t += ngroups) {  // (uniform per group)
    const int32_t c = cs[t], o = os[t];
    // (ni <= 2^31 - 1: one unsigned comparison refuses a negative id too)
    bool bad = (uint32_t)c >= (uint32_t)ni || (uint32_t)o >= (uint32_t)ni;
    int32_t n[K];
    uint32_t differs = 0;  // bit k: m_k
#pragma unroll
    for (int k = 0; k < K; ++k) {
      n[k] = negs[t * K + k];
      if ((uint32_t)n[k] >= (uint32_t)ni) {
        bad = true;
        n[k] = 0;
      }
      differs |= (uint32_t)(n[k] != o) << k;
    }
    float* const diff = diff_t && lig == 0 ? diff_t + t * (K + 1) : nullptr;
    float* row = grads && holds ? grads + t * D + 4 * lig : nullptr;  // the slot's row of the part of grads at hand
    const int64_t pitch = B * D;                                      // from there to its row of the next part
    if (!bad && (!valid || valid[t] != 0)) {
      float4 v = row4_zero(), wo = v;
      if (holds) {
        v = *row4_ptr(in_table, c, D, lig);
        wo = *row4_ptr(out_table, o, D, lig);
      }
      float4 w[K];
#pragma unroll
      for (int k = 0; k < K; ++k) w[k] = row4_load(out_table, n[k], D, lig, holds);
      __builtin_amdgcn_sched_barrier(0);  // (every row load is issued above this line)
      const float so = group_sum(row4_dot(v, wo), G);
      float loss, sig;
      logistic(-so, loss, sig);
      const float ao = -sig;  // sigmoid(s_o) - 1
      float4 gc = mul4(ao, wo);
      float* const centre = row;
      if (row) *reinterpret_cast<float4*>(row += pitch) = fma4(ao, v, mul4(reg, wo));
      if (diff) diff[0] = so;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float sk = group_sum(row4_dot(v, w[k]), G);
        const bool m = (differs >> k) & 1u;
        float sp, ak;
        logistic(sk, sp, ak);
        loss += m ? sp : 0.f;
        const float4 next = fma4(ak, w[k], gc), gn = fma4(ak, v, mul4(reg, w[k]));
        gc = sel4(m, next, gc);
        if (row) *reinterpret_cast<float4*>(row += pitch) = sel4(m, gn, row4_zero());
        if (diff) diff[1 + k] = sk;
      }
      if (centre) *reinterpret_cast<float4*>(centre) = fma4(reg, v, gc);
      if (lig == 0) loss_t[t] = loss;
    } else {
      if (lig == 0) {
        loss_t[t] = 0.f;
        if (bad) atomicOr(failed, kFailBadPosition);
      }
      for (int k = 0; k < K + 2; ++k) {
        if (row) *reinterpret_cast<float4*>(row + k * pitch) = row4_zero();
        if (diff && k <= K) diff[k] = 0.f;
      }
    }
  }
}

}  // namespace esr

namespace esr {

// the launch of sgns_fwd_bwd_kernel<G, K> for K in [1, kSgnsMaxNegatives]
template <int G>
static void sgns_launch(int K, int grid, hipStream_t st, const float* in_table, const float* out_table, int64_t ni, int D,
                        const int32_t* c, const int32_t* o, const int32_t* neg, const int32_t* valid, int64_t B, float reg,
                        float* loss_t, float* diff_t, float* grads, int32_t* failed) {
#define ESR_SGNS_CASE(N)                                                                                                 \
  case N:                                                                                                                \
    hipLaunchKernelGGL((sgns_fwd_bwd_kernel<G, N>), dim3(grid), dim3(kBlock), 0, st, in_table, out_table, ni, D, c, o, neg, \
                       valid, B, reg, loss_t, diff_t, grads, failed);                                                    \
    break;
  switch (K) {
    ESR_SGNS_CASE(1) ESR_SGNS_CASE(2) ESR_SGNS_CASE(3) ESR_SGNS_CASE(4) ESR_SGNS_CASE(5) ESR_SGNS_CASE(6) ESR_SGNS_CASE(7)
    ESR_SGNS_CASE(8) ESR_SGNS_CASE(9) ESR_SGNS_CASE(10) ESR_SGNS_CASE(11) ESR_SGNS_CASE(12) ESR_SGNS_CASE(13)
    ESR_SGNS_CASE(14) ESR_SGNS_CASE(15) ESR_SGNS_CASE(16)
  }
#undef ESR_SGNS_CASE
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_sgns_geometry(int* max_window, int* max_negatives, int* max_rank, int* rank_multiple) {
  ESR_REQUIRE(max_window && max_negatives && max_rank && rank_multiple, "esr_sgns_geometry: null pointer");
  *max_window = kSgnsMaxWindow;
  *max_negatives = kSgnsMaxNegatives;
  *max_rank = kRow4MaxRank;
  *rank_multiple = kRow4RankMultiple;
  return ESR_OK;
}

int esr_sgns_sample(const int64_t* seq_offsets, const int32_t* seq_upos, const int32_t* seq_ipos, int64_t nnz_seq, int64_t nd,
                    int64_t ni, int window, int negatives, const uint32_t* noise_keep, const int32_t* noise_alias,
                    uint64_t seed, uint32_t step0, int64_t K, int64_t B, int32_t* out_c, int32_t* out_e, int32_t* out_o,
                    int32_t* out_valid, int32_t* out_neg, int32_t* dropped, esr_stream_t stream) {
  TraceScope trace_scope_("esr_sgns_sample");
  const char* who = "esr_sgns_sample";
  if (int rc = check_sizes(who, {{"nd", nd}, {"ni", ni}, {"nnz_seq", nnz_seq}}, ": nnz_seq and ni are 32-bit multiply-high factors"))
    return rc;
  ESR_REQUIRE(2 * ni <= (int64_t)INT32_MAX, "%s: 2 ni = %lld exceeds 2^31 - 1 (the virtual row space of the update)", who,
              (long long)(2 * ni));
  ESR_REQUIRE(window >= 1 && window <= kSgnsMaxWindow, "%s: window=%d outside [1, %d]", who, window, kSgnsMaxWindow);
  ESR_REQUIRE(negatives >= 1 && negatives <= kSgnsMaxNegatives, "%s: negatives=%d outside [1, %d]", who, negatives,
              kSgnsMaxNegatives);
  ESR_REQUIRE(seq_offsets && seq_upos && seq_ipos && noise_keep && noise_alias && out_c && out_e && out_o && out_valid &&
                  out_neg && dropped,
              "%s: null pointer", who);
  ESR_REQUIRE(((uintptr_t)seq_offsets & 7) == 0 &&
                  (((uintptr_t)seq_upos | (uintptr_t)seq_ipos | (uintptr_t)noise_keep | (uintptr_t)noise_alias |
                    (uintptr_t)out_c | (uintptr_t)out_e | (uintptr_t)out_o | (uintptr_t)out_valid | (uintptr_t)out_neg |
                    (uintptr_t)dropped) & 3) == 0,
              "%s: misaligned pointer (seq_offsets: 8 bytes)", who);
  hipStream_t st = as_stream(stream);
  int grid;
  int64_t blocks_per_step;
  if (int rc = sample_plan(who, K, B, dropped, st, grid, blocks_per_step)) return rc;
  ESR_KT("sgns_sample", st,
         hipLaunchKernelGGL(sgns_sample_kernel, dim3(grid), dim3(kBlock), 0, st, seq_offsets, seq_upos, seq_ipos,
                            (uint32_t)nnz_seq, nd, (uint32_t)ni, window, negatives, noise_keep, noise_alias, seed, step0, K, B,
                            blocks_per_step, out_c, out_e, out_o, out_valid, out_neg, dropped));
  return check_launch(who);
}

int esr_sgns_fwd_bwd(const float* in_table, const float* out_table, int64_t ni, int D, const int32_t* c, const int32_t* o,
                     const int32_t* neg, const int32_t* valid, int64_t B, int negatives, float reg, float* loss_t,
                     float* diff_t, float* grads, int32_t* failed, esr_stream_t stream) {
  TraceScope trace_scope_("esr_sgns_fwd_bwd");
  const char* who = "esr_sgns_fwd_bwd";
  if (int rc = check_rank(who, D)) return rc;
  if (int rc = check_sizes(who, {{"ni", ni}, {"B", B}})) return rc;
  ESR_REQUIRE(2 * ni <= (int64_t)INT32_MAX, "%s: 2 ni = %lld exceeds 2^31 - 1 (the virtual row space of the update)", who,
              (long long)(2 * ni));
  ESR_REQUIRE(negatives >= 1 && negatives <= kSgnsMaxNegatives, "%s: negatives=%d outside [1, %d]", who, negatives,
              kSgnsMaxNegatives);
  ESR_REQUIRE((int64_t)(2 + negatives) * B <= (int64_t)INT32_MAX,
              "%s: (2 + negatives) B = %lld gradient rows exceed 2^31 - 1", who, (long long)((int64_t)(2 + negatives) * B));
  if (int rc = check_reg(who, reg)) return rc;
  ESR_REQUIRE(in_table && out_table && c && o && neg && loss_t && failed, "%s: null pointer", who);
  ESR_REQUIRE((((uintptr_t)in_table | (uintptr_t)out_table | (uintptr_t)grads) & 15) == 0 &&
                  (((uintptr_t)c | (uintptr_t)o | (uintptr_t)neg | (uintptr_t)valid | (uintptr_t)loss_t | (uintptr_t)diff_t |
                    (uintptr_t)failed) & 3) == 0,
              "%s: misaligned pointer (tables and grads: 16 bytes)", who);
  hipStream_t st = as_stream(stream);
  const int G = row4_lanes(D), grid = grid_for_groups(B, G);
  ESR_DISPATCH_G(G, ESR_KT("sgns_fwd_bwd", st,
                           sgns_launch<GG>(negatives, grid, st, in_table, out_table, ni, D, c, o, neg, valid, B, reg, loss_t,
                                           diff_t, grads, failed)));
  return check_launch(who);
}

}  // extern "C"
