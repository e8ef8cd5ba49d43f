// Diversity re-ranking by Maximal Marginal Relevance (Carbonell and Goldstein, "The Use of MMR, Diversity-Based Reranking
// for Reordering Documents and Producing Summaries", SIGIR 1998) and intra-list similarity (Ziegler, McNee, Konstan, Lausen,
// "Improving Recommendation Lists Through Topic Diversification", WWW 2005) of ONE query, as scalar code.  Plain C++ with no
// HIP dependency of its own: the kernels of esr_rerank.hip take the pieces (rerank_length, rerank_present, rerank_value,
// rerank_better, the lane chain of rerank_sim, the geometry) from here, and a stand-alone host program
// (tests/host/rerank_rule_host.cpp) compiles the whole rule, rerank_mmr_query and rerank_ils_query, for the host.
//
// Inputs.  rows float32 [ni, D], D a multiple of 4 in [4, 128]; cand int32 [width] item POSITIONS into rows; rel float32
// [width]; the list's length L = clamp(length, 0, width) (width when there are no lengths); 1 <= width <= 1024;
// 1 <= n_out <= width; lam in [0, 1] and oml = 1.0f - lam in float32.
//
// sim(a, b) is the dot product of two rows in the summation order of the triple kernels (warp_row_dot of
// esr_warp_sample.h): lane l holds elements 4 l .. 4 l + 3 (lanes with 4 l >= D hold zeros), per lane the chain
// acc = fmaf(A[4 l + e], B[4 l + e], acc) over e = 0 .. 3 from +0.0f, then the butterfly over the G lanes with strides
// 1, 2, ... G / 2, G the power of two >= D / 4.  A function of D and the two rows alone, symmetric bit for bit.
//
// MMR.  1. Candidate c < L is ABSENT when cand[c] lies outside [0, ni) (kRerankFailPos, bit 30) or rel[c] is not finite
//          (kRerankFailRel, bit 29); an absent candidate is never picked and its row is never read.
//       2. Round t = 0 .. n_out - 1 over the present candidates not yet picked: p[c] = 0.0f in round 0 and m[c] after,
//          v[c] = fmaf(lam, rel[c], -(oml * p[c])); the pick is the greatest v, ties to the smallest c: the comparison
//          v > best || (v == best && c < best_c) started from (-inf, kRerankNone = -1), so that a v of -inf or NaN is never
//          picked.  When nothing is picked the list ends.  out_pos[t] = c, out_item[t] = cand[c], out_rel[t] = rel[c],
//          out_value[t] = v[c].
//       3. After pick s every present unpicked c: m[c] = sim(c, s) when t = 0, else fmaxf(m[c], sim(c, s)).
//       4. out_length = the picks; the slots behind hold -1 / -1 / 0 / 0.
//    With lam = 1 this is the stable sort by rel descending.  The output is a function of the query's own (cand, rel, L),
//    rows, lam and n_out.
//
// ILS.  ks: 1 to 8 strictly ascending cutoffs >= 1, kmax = min(ks[last], L).  For position i < kmax, r_i = the fp64 sum over
//    present j < i in ascending j of (double)sim(i, j) (0 when i is absent); P_i = P_(i-1) + r_i in ascending i in fp64; n_k =
//    the present candidates among the first min(k, L); ils[k] = float32(P_(min(k, L) - 1) / (n_k (n_k - 1) / 2)) and
//    valid[k] = 1, or 0 and valid[k] = 0 with fewer than two present candidates.  Presence is the position test alone.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "esr_row4.h"
#include "esr_warp_sample.h"

namespace esr {

constexpr int kRerankMaxRank = kRow4MaxRank, kRerankRankMultiple = kRow4RankMultiple;
constexpr int kRerankMaxWidth = 1024;          // kSelectMaxK: the widest list retrieve_topk selects
constexpr int kRerankMaxCutoffs = 8;           // as esr_eval.hip
constexpr int kRerankFailPos = 1 << 30;        // a position outside the table (as FAIL_BAD_POSITION of esr_als.hip)
constexpr int kRerankFailRel = 1 << 29;        // a relevance that is not finite
constexpr int kRerankNone = -1;                // "no candidate" of the argmax
constexpr int kRerankStageBytes = 128 * 1024;  // the rows of a query are staged in LDS when width * D * 4 is within this
constexpr int kRerankStateBytes = 16;          // LDS per candidate beside the rows: m, rel, position, flags
constexpr int kRerankPresent = 1, kRerankPicked = 2;

// the launch form and its dynamic LDS: functions of (width, D) alone.  Rows (<= 128 KiB) and state (<= 16 KiB) leave 16 KiB
// of a CU's 160 KiB to the static exchange words with one workgroup resident.
ESR_HD inline bool rerank_staged(int width, int D) { return (int64_t)width * D * 4 <= (int64_t)kRerankStageBytes; }
ESR_HD inline int rerank_lds_bytes(int width, int D) {
  return width * kRerankStateBytes + (rerank_staged(width, D) ? width * D * 4 : 0);
}

ESR_HD inline int rerank_length(const int32_t* lengths, int64_t q, int width) {
  if (!lengths) return width;
  const int32_t l = lengths[q];
  return l < 0 ? 0 : (l > width ? width : l);
}

// the failure bits of candidate (pos, rel): 0 = present
ESR_HD inline int rerank_absent_bits(int32_t pos, float rel, int64_t ni) {
  int bits = 0;
  if (pos < 0 || (int64_t)pos >= ni) bits |= kRerankFailPos;
  if (!(fabsf(rel) <= FLT_MAX)) bits |= kRerankFailRel;
  return bits;
}

ESR_HD inline float rerank_value(float lam, float oml, float rel, float p) {
  const float pen = oml * p;  // (rounded on its own: the fmaf below takes it negated)
  return fmaf(lam, rel, -pen);
}

ESR_HD inline bool rerank_better(float v, int c, float best, int best_c) { return v > best || (v == best && c < best_c); }

ESR_HD inline float rerank_sim(const float* a, const float* b, int D) { return warp_row_dot(a, b, D); }

// The MMR of one query.  state int32[width] and m float[width] are scratch.  Returns the failure bits.
ESR_HD inline int rerank_mmr_query(const float* rows, int64_t ni, int D, const int32_t* cand, const float* rel, int L,
                                   int n_out, float lam, int32_t* state, float* m, int32_t* out_pos, int32_t* out_item,
                                   float* out_rel, float* out_value, int32_t* out_length) {
  const float oml = 1.0f - lam;
  int failed = 0;
  for (int c = 0; c < L; ++c) {
    const int bits = rerank_absent_bits(cand[c], rel[c], ni);
    failed |= bits;
    state[c] = bits ? 0 : kRerankPresent;
    m[c] = 0.0f;
  }
  int t = 0;
  for (; t < n_out; ++t) {
    float best = -INFINITY;
    int best_c = kRerankNone;
    for (int c = 0; c < L; ++c) {
      if (state[c] != kRerankPresent) continue;
      const float v = rerank_value(lam, oml, rel[c], t == 0 ? 0.0f : m[c]);
      if (rerank_better(v, c, best, best_c)) best = v, best_c = c;
    }
    if (best_c == kRerankNone) break;
    out_pos[t] = best_c, out_item[t] = cand[best_c], out_rel[t] = rel[best_c], out_value[t] = best;
    state[best_c] |= kRerankPicked;
    const float* s = rows + (int64_t)cand[best_c] * D;
    for (int c = 0; c < L; ++c) {
      if (state[c] != kRerankPresent) continue;
      const float sim = rerank_sim(rows + (int64_t)cand[c] * D, s, D);
      m[c] = t == 0 ? sim : fmaxf(m[c], sim);
    }
  }
  *out_length = t;
  for (; t < n_out; ++t) out_pos[t] = -1, out_item[t] = -1, out_rel[t] = 0.0f, out_value[t] = 0.0f;
  return failed;
}

// The intra-list similarity of one query at nk cutoffs.  Returns the failure bits.
ESR_HD inline int rerank_ils_query(const float* rows, int64_t ni, int D, const int32_t* cand, int L, const int32_t* ks, int nk,
                                   float* ils, int32_t* valid) {
  const int kmax = ks[nk - 1] < L ? ks[nk - 1] : L;
  int failed = 0, n = 0, j = 0;
  double P = 0.0;
  for (int i = 0; i <= kmax; ++i) {  // (position i closes every cutoff whose min(k, L) is i)
    for (; j < nk && (ks[j] < L ? ks[j] : L) == i; ++j) {
      const bool ok = n >= 2;
      ils[j] = ok ? (float)(P / ((double)n * (double)(n - 1) * 0.5)) : 0.0f;
      valid[j] = ok;
    }
    if (i == kmax) break;
    if (cand[i] < 0 || (int64_t)cand[i] >= ni) {
      failed |= kRerankFailPos;
      continue;
    }
    double r = 0.0;
    const float* a = rows + (int64_t)cand[i] * D;
    for (int jj = 0; jj < i; ++jj)
      if (cand[jj] >= 0 && (int64_t)cand[jj] < ni) r += (double)rerank_sim(a, rows + (int64_t)cand[jj] * D, D);
    P += r;
    n += 1;
  }
  return failed;
}

}  // namespace esr
