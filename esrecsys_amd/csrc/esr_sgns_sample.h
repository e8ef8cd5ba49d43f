// The slot sampler of skip-gram with negative sampling (Mikolov et al., NIPS 2013; item2vec, Barkan and Koenigstein 2016):
// one (centre item, context item of the same document, K noise items) slot drawn from Philox4x32-10, the documents'
// sequences in order and a Walker / Vose alias table of the noise distribution.  Plain integer C++ with no HIP dependency
// of its own: the kernel of esr_sgns.hip and a stand-alone host program (tests/host/sgns_sample_host.cpp) include the same
// text.
#pragma once
#include <stdint.h>

#include "esr_philox.h"

namespace esr {

constexpr int kSgnsMaxWindow = 32;     // the largest context distance
constexpr int kSgnsMaxNegatives = 16;  // noise items per slot: the row loads one lane keeps in flight beside the two others

struct SgnsSlot {
  int32_t c, e, o, valid;
};

// The slot t of global step s under `seed`.  The documents are a CSR in order, repeats kept: seq_offsets[nd + 1], and per
// event its document seq_upos[nnz_seq] and item position seq_ipos[nnz_seq].  The noise table is noise_keep uint32[ni] and
// noise_alias int32[ni]: column n yields item n for a word below noise_keep[n] and item noise_alias[n] otherwise; a full
// column is stored as noise_alias[n] == n.  1 <= nnz_seq, ni <= 2^31 - 1 (both enter a multiply-high as 32-bit factors),
// 1 <= window <= kSgnsMaxWindow, 1 <= K <= kSgnsMaxNegatives.
//   Philox block b = philox4x32_10(counter (t, s, b, 0), key (seed low, seed high)): BPR's counter layout.
//   Word 0 of block 0 picks the event: e = (word * nnz_seq) >> 32, the centre c = seq_ipos[e]; its document is
//   u = seq_upos[e], the events [seq_offsets[u], seq_offsets[u + 1]).
//   Word 1 of block 0 picks the distance d in [1, window] with weight window - d + 1 (word2vec's shrunk window: a pair at
//   distance d is trained with probability (window - d + 1) / window):  r = (word * (window (window + 1) / 2)) >> 32, and d
//   is the first distance whose running weight window + (window - 1) + .. exceeds r -- an integer loop of at most window
//   turns.
//   The top bit of word 2 of block 0 picks the side: p = e + d when set, e - d otherwise.  If p lies outside the document
//   the slot has valid = 0 and carries o = c; else o = seq_ipos[p].  The context never crosses a document boundary.
//   Noise item k takes words 2 (k & 1) and 2 (k & 1) + 1 of block 1 + (k >> 1): the first picks the column
//   n = (word * ni) >> 32, the second the item: n if word < noise_keep[n], noise_alias[n] otherwise.
// Nothing else enters: a slot is a function of (seed, s, t, the sequence CSR, window, K, the noise table) alone.  The
// relative bias of the event draw is at most nnz_seq / 2^32, that of the distance window (window + 1) / 2^33, that of a
// column ni / 2^32.
// e < nnz_seq and n < ni by construction; u is clamped into [0, nd), the document's start into [0, e] and its end into
// [e + 1, nnz_seq] (no-ops on a CSR as described), so an ill-formed CSR gives a wrong slot but never a read outside the
// arrays.  neg points at the slot's K entries.
ESR_HD inline SgnsSlot sgns_sample_slot(const int64_t* seq_offsets, const int32_t* seq_upos, const int32_t* seq_ipos,
                                        uint32_t nnz_seq, int64_t nd, uint32_t ni, int window, int K,
                                        const uint32_t* noise_keep, const int32_t* noise_alias, uint64_t seed, uint32_t step,
                                        uint32_t t, int32_t* neg) {
  const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t counter[4] = {t, step, 0u, 0u}, w[4];
  philox4x32_10(counter, key, w);
  const int64_t e = (int64_t)(((uint64_t)w[0] * nnz_seq) >> 32);
  SgnsSlot r;
  r.e = (int32_t)e;
  r.c = seq_ipos[e];
  int64_t u = seq_upos[e];
  u = u < 0 ? 0 : (u >= nd ? nd - 1 : u);
  int64_t start = seq_offsets[u], end = seq_offsets[u + 1];
  start = start < 0 ? 0 : (start > e ? e : start);
  end = end < e + 1 ? e + 1 : (end > (int64_t)nnz_seq ? (int64_t)nnz_seq : end);
  uint32_t rem = (uint32_t)(((uint64_t)w[1] * (uint32_t)(window * (window + 1) / 2)) >> 32), weight = (uint32_t)window;
  int d = 1;
  for (int turn = 1; turn < window && rem >= weight; ++turn) {
    rem -= weight;
    --weight;
    ++d;
  }
  const int64_t p = (w[2] >> 31) ? e + d : e - d;
  r.valid = p >= start && p < end;
  r.o = r.valid ? seq_ipos[p] : r.c;
  for (int k = 0; k < K; ++k) {
    if ((k & 1) == 0) {
      counter[2] = 1u + ((uint32_t)k >> 1);
      philox4x32_10(counter, key, w);
    }
    const uint32_t n = (uint32_t)(((uint64_t)w[2 * (k & 1)] * ni) >> 32);
    neg[k] = w[2 * (k & 1) + 1] < noise_keep[n] ? (int32_t)n : noise_alias[n];
  }
  return r;
}

}  // namespace esr
