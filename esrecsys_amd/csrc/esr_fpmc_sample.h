// The slot sampler of the Factorised Personalised Markov Chain (Rendle, Freudenthaler, Schmidt-Thieme, WWW 2010) trained
// with the BPR step: one (user, event, context length, next item, unseen item) slot drawn from Philox4x32-10, the users'
// sequences in time order and BPR's CSR of the seen pairs.  Plain integer C++ with no HIP dependency of its own: the
// kernel of esr_fpmc.hip and a stand-alone host program (tests/host/fpmc_sample_host.cpp) include the same text.
#pragma once
#include <stdint.h>

#include "esr_bpr_sample.h"

namespace esr {

constexpr int kFpmcMaxWindow = 8;  // context items per event: the row loads one lane keeps in flight beside the five others

struct FpmcSlot {
  int32_t u, e, c, i, j, valid;
};

// The slot t of global step s under `seed`.  The sequences are a CSR by user in time order, repeats kept: seq_offsets
// [nu + 1], and per event its user position seq_upos[nnz_seq] and item position seq_ipos[nnz_seq].  The seen pairs are
// BPR's CSR (esr_bpr_sample.h): row_offsets[nu + 1], row_ipos[nnz_seen] ascending and distinct within a row.
// 1 <= nnz_seq, ni <= 2^31 - 1 (both enter a multiply-high as 32-bit factors), 1 <= window <= kFpmcMaxWindow.
//   Philox block b = philox4x32_10(counter (t, s, b, 0), key (seed low, seed high)): BPR's stream.
//   Word 0 of block 0 picks the event: e = (word * nnz_seq) >> 32, u = seq_upos[e], i = seq_ipos[e]; its place in u's
//   sequence is pos = e - seq_offsets[u] and its context the c = min(pos, window) events e - c .. e - 1, oldest first.
//   The 15 words that follow are BPR's negative candidates in BPR's order, j = (word * ni) >> 32, tested with bpr_row_has
//   against u's seen row; the first one that is not in the row is the negative and the slot is valid.  If all 15 are in
//   the row the slot carries the last candidate and valid = 0.
// Nothing else enters: a slot is a function of (seed, s, t, the two CSRs, window) alone.  The relative bias of the event
// draw is at most nnz_seq / 2^32, that of a candidate at most ni / 2^32.
// e < nnz_seq by construction; u and its seen row are clamped by bpr_user_row, the start of its sequence into [0, e]
// (no-ops on CSRs as described), so an ill-formed CSR gives a wrong slot but never a read outside the arrays, and
// c <= e - start: the context never crosses into the events of the user before.  The negative is bpr_walk_negative's.
ESR_HD inline FpmcSlot fpmc_sample_slot(const int64_t* seq_offsets, const int32_t* seq_upos, const int32_t* seq_ipos,
                                        uint32_t nnz_seq, const int64_t* row_offsets, const int32_t* row_ipos,
                                        int64_t nnz_seen, int64_t nu, uint32_t ni, int window, uint64_t seed, uint32_t step,
                                        uint32_t t) {
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  const uint32_t counter[4] = {t, step, 0u, 0u};
  uint32_t w[4];
  philox4x32_10(counter, key, w);
  const int64_t e = (int64_t)(((uint64_t)w[0] * nnz_seq) >> 32);
  const BprRow row = bpr_user_row(row_offsets, seq_upos[e], nu, nnz_seen);
  FpmcSlot r;
  r.u = row.u;
  r.e = (int32_t)e;
  r.i = seq_ipos[e];
  int64_t start = seq_offsets[row.u];
  start = start < 0 ? 0 : (start > e ? e : start);
  const int64_t pos = e - start;
  r.c = (int32_t)(pos < (int64_t)window ? pos : (int64_t)window);
  r.j = bpr_walk_negative(row_ipos, row.lo, row.hi, key, step, t, ni, w, r.valid);
  return r;
}

}  // namespace esr
