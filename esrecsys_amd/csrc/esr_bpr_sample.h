// The triple sampler of Bayesian Personalised Ranking (Rendle et al., UAI 2009): one (user, seen item, unseen item) triple
// per slot, drawn from Philox4x32-10 and the CSR of the seen pairs.  Plain integer C++ with no HIP dependency of its own:
// the kernel of esr_bpr.hip, the host side of the library and a stand-alone host program (tests/host/bpr_sample_host.cpp)
// include the same text.
#pragma once
#include <stdint.h>

#include "esr_philox.h"

namespace esr {

constexpr int kBprMaxTries = 15;  // negative candidates per triple: words 1..3 of Philox block 0, all of blocks 1, 2 and 3

struct BprTriple {
  int32_t u, i, j, valid;
};

// Is item position j among row_ipos[lo, hi) (ascending, distinct)?  A lower-bound search: hi - lo <= 2^31 - 1 entries are
// decided in at most 31 probes; the loop is bounded besides, so no input can make it spin.
ESR_HD inline bool bpr_row_has(const int32_t* row_ipos, int64_t lo, int64_t hi, int32_t j) {
  const int64_t end = hi;
  for (int probe = 0; probe < 32 && lo < hi; ++probe) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (row_ipos[mid] < j) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && row_ipos[lo] == j;
}

// A user clamped into [0, nu) and its row of the CSR clamped into [0, nnz]: no-ops on a well-formed CSR, so an ill-formed
// one gives a wrong draw but never a read outside the arrays.
struct BprRow {
  int32_t u;
  int64_t lo, hi;
};
ESR_HD inline BprRow bpr_user_row(const int64_t* row_offsets, int64_t u, int64_t nu, int64_t nnz) {
  u = u < 0 ? 0 : (u >= nu ? nu - 1 : u);
  int64_t lo = row_offsets[u], hi = row_offsets[u + 1];
  lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
  hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
  return {(int32_t)u, lo, hi};
}

// The seen pair of slot t of step `step`: w receives Philox block 0 of the slot, its word 0 picks the pair (p < nnz by
// construction) and its words 1..3 are candidates 0..2.
struct BprPair {
  int32_t u, i;
  int64_t lo, hi;  // u's row
};
ESR_HD inline BprPair bpr_pick_pair(const int64_t* row_offsets, const int32_t* row_upos, const int32_t* row_ipos, int64_t nu,
                                    uint32_t nnz, const uint32_t key[2], uint32_t step, uint32_t t, uint32_t w[4]) {
  const uint32_t counter[4] = {t, step, 0u, 0u};
  philox4x32_10(counter, key, w);
  const uint32_t p = (uint32_t)(((uint64_t)w[0] * nnz) >> 32);
  const BprRow row = bpr_user_row(row_offsets, row_upos[p], nu, (int64_t)nnz);
  return {row.u, row_ipos[p], row.lo, row.hi};
}

// Candidate c = 0, 1, ... of the slot: word (c + 1) & 3 of block (c + 1) >> 2, j = (word * ni) >> 32.  w holds the block
// of candidate c - 1 on entry and is refreshed when c + 1 is a block's first word.
ESR_HD inline int32_t bpr_candidate(const uint32_t key[2], uint32_t step, uint32_t t, int c, uint32_t ni, uint32_t w[4]) {
  const int word = (c + 1) & 3;
  if (word == 0) {
    const uint32_t counter[4] = {t, step, (uint32_t)(c + 1) >> 2, 0u};
    philox4x32_10(counter, key, w);
  }
  const uint32_t v = word == 0 ? w[0] : (word == 1 ? w[1] : (word == 2 ? w[2] : w[3]));  // (no runtime-indexed array)
  return (int32_t)(((uint64_t)v * ni) >> 32);
}

// The negative of a slot whose block 0 is in w: candidates 0 .. kBprMaxTries - 1 in order, the first one that is not in
// row_ipos[lo, hi) with valid = 1; if all are in the row, the last one with valid = 0.
ESR_HD inline int32_t bpr_walk_negative(const int32_t* row_ipos, int64_t lo, int64_t hi, const uint32_t key[2], uint32_t step,
                                        uint32_t t, uint32_t ni, uint32_t w[4], int32_t& valid) {
  int32_t j = 0;
  valid = 0;
  for (int c = 0; c < kBprMaxTries && !valid; ++c) {
    j = bpr_candidate(key, step, t, c, ni, w);
    valid = !bpr_row_has(row_ipos, lo, hi, j);
  }
  return j;
}

// The triple of slot t of global step s under `seed`.  The seen pairs are a CSR by user: row_offsets[nu + 1], and per
// pair its user position row_upos[nnz] and item position row_ipos[nnz], the item positions ascending within a row and the
// pairs distinct.  1 <= nnz <= 2^31 - 1 and 1 <= ni <= 2^31 - 1 (both enter a multiply-high as 32-bit factors).
//   Philox block b = philox4x32_10(counter (t, s, b, 0), key (seed low, seed high)).
//   Word 0 of block 0 picks the pair: p = (word * nnz) >> 32, u = row_upos[p], i = row_ipos[p].
//   The 15 words that follow -- words 1..3 of block 0, then words 0..3 of blocks 1, 2 and 3 -- are the negative candidates
//   in order, j = (word * ni) >> 32; the first one that is not in u's row is the negative and the triple is valid.  If
//   all 15 are in the row the triple carries the last candidate and valid = 0.
// Nothing else enters: a triple is a function of (seed, s, t, the CSR) alone.  The multiply-high maps 2^32 words onto n
// values, floor or ceil of 2^32 / n words each: the relative bias of the pair draw is at most nnz / 2^32, that of a
// candidate at most ni / 2^32.
// The pieces above are the only text of these rules: FPMC's slot (esr_fpmc_sample.h) and WARP's search
// (esr_warp_sample.h) call the same bpr_user_row / bpr_pick_pair / bpr_candidate / bpr_walk_negative.
ESR_HD inline BprTriple bpr_sample_triple(const int64_t* row_offsets, const int32_t* row_upos, const int32_t* row_ipos,
                                          int64_t nu, uint32_t ni, uint32_t nnz, uint64_t seed, uint32_t step, uint32_t t) {
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  const BprPair pr = bpr_pick_pair(row_offsets, row_upos, row_ipos, nu, nnz, key, step, t, w);
  BprTriple r;
  r.u = pr.u;
  r.i = pr.i;
  r.j = bpr_walk_negative(row_ipos, pr.lo, pr.hi, key, step, t, ni, w, r.valid);
  return r;
}

}  // namespace esr
