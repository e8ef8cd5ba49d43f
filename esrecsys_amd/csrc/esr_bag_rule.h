// The rule of a bag table -- the weighted sum of feature rows that composes an entity of the hybrid model (Kula,
// "Metadata Embeddings for User and Item Cold-start Recommendations", 2015) and its transpose for the optimiser.  Plain C++
// with no HIP dependency of its own: the kernels of esr_bag.hip and a stand-alone host program
// (tests/host/bag_rule_host.cpp) include the same text.
//
// A bag table is a CSR over entities: bag_offsets int64[n_bags + 1], bag_feat int32[nnz] (row positions into a feature
// table E float[nf, D]) and bag_weight float[nnz] or null (every weight 1).
//   sum     out[c] = acc after acc = fmaf(w[k], E[feat[k], c], acc) for k = off[b] .. off[b + 1] - 1 ascending, from +0.0f.
//   expand  for occurrence k of bag b and the bag's gradient row g: row[c] = fmaf(w[k], g[c], reg * E[feat[k], c]).
// The row bounds are clamped into [0, nnz] (no-ops on a CSR as described), so an ill-formed CSR gives a wrong row and never
// a read outside the arrays; a feature position outside [0, nf) or a bag number outside [0, n_bags) is refused by the
// caller of these pieces (bag_feat_ok, bag_number_ok) and reads nothing.
#pragma once
#include <math.h>
#include <stdint.h>

#include "esr_row4.h"

namespace esr {

constexpr int kBagMaxRank = kRow4MaxRank, kBagRankMultiple = kRow4RankMultiple;  // (tests/host name these)
constexpr int kBagFailBad = 1 << 30;  // as FAIL_BAD_POSITION of esr_als.hip
constexpr int kBagUnroll = 4;         // feature rows whose loads the sum kernel issues together (the fmaf chain keeps its order)

struct BagSpan {
  int64_t lo, hi;  // occurrences [lo, hi) of bag_feat / bag_weight
};

ESR_HD inline bool bag_number_ok(int64_t b, int64_t n_bags) { return b >= 0 && b < n_bags; }
ESR_HD inline bool bag_feat_ok(int64_t f, int64_t nf) { return f >= 0 && f < nf; }

// the occurrences of bag b, 0 <= b < n_bags
ESR_HD inline BagSpan bag_span(const int64_t* bag_offsets, int64_t b, int64_t nnz) {
  BagSpan s;
  s.lo = bag_offsets[b];
  s.hi = bag_offsets[b + 1];
  s.lo = s.lo < 0 ? 0 : (s.lo > nnz ? nnz : s.lo);
  s.hi = s.hi < s.lo ? s.lo : (s.hi > nnz ? nnz : s.hi);
  return s;
}

// one step of the sum's chain
ESR_HD inline float bag_step(float w, float e, float acc) { return fmaf(w, e, acc); }

// one element of an expanded gradient row
ESR_HD inline float bag_expand_elem(float w, float g, float reg, float e) {
  const float l2 = reg * e;  // (rounded once on its own: no a * b + c for the compiler to contract)
  return fmaf(w, g, l2);
}

// Row b of the composition in full, the way one lane group walks it: false (and a zero row) when the bag number or one of
// its feature positions is refused.  The kernel runs this chain per element with the loads of kBagUnroll rows batched.
ESR_HD inline bool bag_sum_row(const float* table, int64_t nf, int D, const int64_t* bag_offsets, const int32_t* bag_feat,
                               const float* bag_weight, int64_t nnz, int64_t n_bags, int64_t b, float* out) {
  for (int c = 0; c < D; ++c) out[c] = 0.0f;
  if (!bag_number_ok(b, n_bags)) return false;
  const BagSpan s = bag_span(bag_offsets, b, nnz);
  for (int64_t k = s.lo; k < s.hi; ++k)
    if (!bag_feat_ok(bag_feat[k], nf)) return false;
  for (int64_t k = s.lo; k < s.hi; ++k) {
    const float w = bag_weight ? bag_weight[k] : 1.0f;
    const float* e = table + (int64_t)bag_feat[k] * D;
    for (int c = 0; c < D; ++c) out[c] = bag_step(w, e[c], out[c]);
  }
  return true;
}

// Output row q - q0 of selected bag b in full (q0 = the bag's first output position): the feature position it is for
// (0 when refused) and the gradient row; false when the occurrence is refused -- a bag number or feature position outside
// its table, or an output position the bag has no occurrence for.  live = 0 (valid[r] == 0): a zero row, E is not read.
ESR_HD inline bool bag_expand_row(const float* table, int64_t nf, int D, const int64_t* bag_offsets, const int32_t* bag_feat,
                                  const float* bag_weight, int64_t nnz, int64_t n_bags, int64_t b, int64_t within,
                                  const float* grad_row, int live, float reg, int32_t* out_feat, float* out_row) {
  for (int c = 0; c < D; ++c) out_row[c] = 0.0f;
  *out_feat = 0;
  if (!bag_number_ok(b, n_bags)) return false;
  const BagSpan s = bag_span(bag_offsets, b, nnz);
  const int64_t k = s.lo + within;
  if (within < 0 || k >= s.hi || !bag_feat_ok(bag_feat[k], nf)) return false;
  *out_feat = bag_feat[k];
  if (!live) return true;
  const float w = bag_weight ? bag_weight[k] : 1.0f;
  const float* e = table + (int64_t)bag_feat[k] * D;
  for (int c = 0; c < D; ++c) out_row[c] = bag_expand_elem(w, grad_row[c], reg, e[c]);
  return true;
}

}  // namespace esr
