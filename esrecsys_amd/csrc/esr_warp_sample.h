// WARP (Weston, Bengio, Usunier, "WSABIE: Scaling Up To Large Vocabulary Image Annotation", IJCAI 2011): the search for
// a margin-violating negative, the rank estimate and the rank-weighted hinge step of ONE slot, as scalar code.  Plain C++
// with no HIP dependency of its own: the kernel of esr_warp.hip takes its integer pieces (bpr_pick_pair and
// bpr_candidate of esr_bpr_sample.h, warp_rank) and its per-lane chain (warp_lane_dot, the row4_chain of esr_row4.h)
// through this file, and a stand-alone host program (tests/host/warp_sample_host.cpp) compiles the whole rule, warp_slot, for the host.
//
// The rule.  Inputs: the CSR of seen pairs by user (row_offsets[nu + 1], row_upos[nnz], row_ipos[nnz], item positions
// ascending and distinct within a row), user_table [nu, D] and item_table [ni, D] float32 with D a multiple of 4 in
// [4, 128], max_trials T in [1, 255], margin (finite), reg (finite, not negative) and a rank-weight table
// rank_weight float32 [ni + 1].  For slot t of global step s under `seed`:
//   1. Philox stream: exactly that of bpr_sample_triple.  Block b = philox4x32_10((t, s, b, 0), (seed lo, seed hi)).  Word
//      0 of block 0 picks the pair, p = (word * nnz) >> 32, u = row_upos[p] (clamped as there), i = row_ipos[p].
//      Candidate c = 0, 1, ... is word (c + 1) & 3 of block (c + 1) >> 2, j = (word * ni) >> 32.  A block is computed
//      when its first word is needed.  For c < 15 the candidates are BPR's.
//   2. Positive score: s_i = x_u . y_i in the summation order of bpr_fwd_bwd_kernel applied to one row instead of a
//      difference: "lane" l holds elements 4 l .. 4 l + 3 (lanes with 4 l >= D hold zeros); per lane the chain
//      fmaf(x[e], y[e], acc) over e = 0..3 from 0; then the butterfly over the G lanes with strides 1, 2, ... G / 2
//      (v[l] + v[l ^ stride]), G the power of two >= D / 4.  A function of D alone.
//   3. The search: walk candidates c = 0 .. T - 1 in order.  A candidate in u's row (bpr_row_has) is skipped and not
//      counted.  Otherwise N += 1, s_j = x_u . y_j in the same order and d = s_i - s_j as one float32 subtraction.  The
//      first candidate with d < margin (strict) is the negative and the search ends there.  If no candidate violates, the
//      slot has valid = 0, its j is the last candidate walked, its trials is N (which may be 0), and its loss, d and
//      three gradient rows are zero.
//   4. Rank weight: for a valid slot r = max(1, (ni - len_u) / N) in integer division, len_u the row length of u;
//      w = rank_weight[r], loss_t = w * (margin - d), g_u = reg x - w (y_i - y_j), g_i = reg y_i - w x,
//      g_j = reg y_j + w x, written as rows t, B + t and 2 B + t of grads.
//   5. Nothing else enters: a slot is a function of (seed, s, t, CSR, the two tables, T, margin, reg, rank_weight) alone --
//      not of B, of the grid or of the slots that share its wave.  No reduction across slots, no float atomic, no
//      grid-wide pass, nothing polled; the only loops are the <= T trials and the <= 32-probe search.  A position outside
//      a table (i of an ill-formed CSR; u is clamped, j is in [0, ni) by construction) sets `bad` -- bit 30 of `failed` in
//      the kernel -- and the slot reads no row: j = 0, valid = 0, trials = 0 and zeros.
#pragma once
#include <math.h>
#include <stdint.h>

#include "esr_bpr_sample.h"
#include "esr_philox.h"
#include "esr_row4.h"

namespace esr {

constexpr int kWarpMaxTrials = 255;  // candidate c is word c + 1 of the slot's stream: blocks 0 .. 63
constexpr int kWarpMaxRank = kRow4MaxRank, kWarpRankMultiple = kRow4RankMultiple;  // (tests/host name these)

// Step 1 is bpr_pick_pair and bpr_candidate (esr_bpr_sample.h).  Step 2, one lane's chain over its four elements:
ESR_HD inline float warp_lane_dot(float x0, float x1, float x2, float x3, float y0, float y1, float y2, float y3) {
  return row4_chain(x0, x1, x2, x3, y0, y1, y2, y3, 0.f);
}

// Step 4, the rank estimate of a valid slot (N >= 1): in [1, max(1, ni)], an index into rank_weight[ni + 1].
ESR_HD inline int64_t warp_rank(uint32_t ni, int64_t row_len, int32_t N) {
  const int64_t r = ((int64_t)ni - row_len) / (int64_t)N;
  return r < 1 ? 1 : r;
}

// Step 2 whole, as the kernel's lanes compute it: x and y hold D floats.
ESR_HD inline float warp_row_dot(const float* x, const float* y, int D) {
  const int G = row4_lanes(D), nvec = D >> 2;
  float v[32], n[32];
  for (int l = 0; l < G; ++l)
    v[l] = l < nvec ? warp_lane_dot(x[4 * l], x[4 * l + 1], x[4 * l + 2], x[4 * l + 3], y[4 * l], y[4 * l + 1], y[4 * l + 2],
                                    y[4 * l + 3])
                    : warp_lane_dot(0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
  for (int stride = 1; stride < G; stride <<= 1) {
    for (int l = 0; l < G; ++l) n[l] = v[l] + v[l ^ stride];
    for (int l = 0; l < G; ++l) v[l] = n[l];
  }
  return v[0];
}

struct WarpSlot {
  int32_t u, i, j, valid, trials, bad;
  float s_i, d, w, loss;
};

// The whole rule for one slot.  grads3 (may be null) receives the three gradient rows [g_u ; g_i ; g_j], 3 D floats.
ESR_HD inline WarpSlot warp_slot(const float* user_table, int64_t nu, const float* item_table, uint32_t ni, int D,
                          const int64_t* row_offsets, const int32_t* row_upos, const int32_t* row_ipos, uint32_t nnz,
                          const float* rank_weight, uint64_t seed, uint32_t step, uint32_t t, int max_trials, float margin,
                          float reg, float* grads3) {
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  const BprPair pr = bpr_pick_pair(row_offsets, row_upos, row_ipos, nu, nnz, key, step, t, w);
  WarpSlot r;
  r.u = pr.u;
  r.i = pr.i;
  r.j = 0;
  r.valid = r.trials = 0;
  r.s_i = r.d = r.w = r.loss = 0.f;
  r.bad = pr.i < 0 || (int64_t)pr.i >= (int64_t)ni;
  if (grads3)
    for (int e = 0; e < 3 * D; ++e) grads3[e] = 0.f;
  if (r.bad) return r;
  const float *x = user_table + (int64_t)pr.u * D, *yi = item_table + (int64_t)pr.i * D, *yj = yi;
  r.s_i = warp_row_dot(x, yi, D);
  for (int c = 0; c < max_trials; ++c) {
    r.j = bpr_candidate(key, step, t, c, ni, w);
    if (bpr_row_has(row_ipos, pr.lo, pr.hi, r.j)) continue;
    r.trials += 1;
    yj = item_table + (int64_t)r.j * D;
    const float d = r.s_i - warp_row_dot(x, yj, D);
    if (d < margin) {
      r.valid = 1;
      r.d = d;
      break;
    }
  }
  if (!r.valid) return r;
  r.w = rank_weight[warp_rank(ni, pr.hi - pr.lo, r.trials)];
  r.loss = r.w * (margin - r.d);
  if (grads3)
    for (int e = 0; e < D; ++e) {
      grads3[e] = reg * x[e] - r.w * (yi[e] - yj[e]);
      grads3[D + e] = reg * yi[e] - r.w * x[e];
      grads3[2 * D + e] = reg * yj[e] + r.w * x[e];
    }
  return r;
}

}  // namespace esr
