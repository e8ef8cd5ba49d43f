// Offline evaluation of ranked lists against held-out truth sets: esr_eval_ranking (the reference's protocol is
// spotify/make_training.py:74-98 -- the first tracks are the context, the rest are to be predicted -- and its trainer
// reports the recall of the next tracks among the 500 best, train_spotify.py:113-131).  One launch scores nq lists at up
// to 8 cutoffs: hits, first hit, precision, recall, reciprocal rank, average precision and nDCG.
//   per query   one workgroup.  The truth ids go into an open-addressing table in LDS (recall_at_k_kernel's idiom,
//               esr_retrieve.hip) whose slots hold the id and the FIRST list position that found it; equal ids share a
//               slot, so the claimed slots are the distinct truth size.  The list positions r < min(length, kmax) probe the
//               table (atomicMin of r into the slot); after a barrier position r is a hit if its id was found and
//               (count_repeats or the slot's first position is r).  The hits of 64 consecutive positions are one wave's
//               ballot: a bitmap in LDS, written without atomics.
//   the walk    ONE lane walks the bitmap in ascending rank with c = hits so far, ap_sum += (double)c / r and
//               dcg += disc[r - 1] at each hit of 1-based rank r, and emits every cutoff as it passes it.  disc[r - 1] =
//               1 / log2(r + 1) and cum_disc = [0, cumsum(disc)] are made by the caller in float64 and only read here:
//               the device evaluates no logarithm.  Every float is ONE fp64 expression -- a division of two exactly
//               converted integers, or of a running fp64 sum by one -- rounded once to f32; there is no product next to
//               a sum, so nothing is left for fp contraction to fuse and the bits are those of a NumPy restatement.
//   sizes       the table of a query has the smallest power of two >= 2 x its listed truth length (at least 64, at most
//               what the launch allocated from the caller's bound max_truth): short truth sets do not pay for the longest.
// Every loop is bounded (a probe by the slot count); no kernel waits on another workgroup.
#include "esr_common.h"

namespace esr {

constexpr int kEvalMaxTruth = 4096;    // distinct truth ids of a query: 8192 slots of 8 bytes = 64 KiB at load <= 1/2
constexpr int kEvalMaxWidth = 4096;    // list positions a workgroup keeps a hit bit for
constexpr int kEvalMaxCutoffs = 8;
constexpr int kEvalMinSlots = 64;
constexpr int kEvalWords = kEvalMaxWidth / 64;
constexpr unsigned long long kEvalFailNegative = 2;  // as the pair table's bit 2
constexpr unsigned long long kEvalFailOffsets = 4;   // truth_offsets outside [0, n], falling, or a set above max_truth
constexpr unsigned long long kEvalFailFull = 8;      // more than kEvalMaxTruth distinct truth ids

struct EvalArgs {
  const int32_t* rec;
  int64_t pitch;
  int width;
  const int32_t* rec_len;
  const int32_t* truth;
  int64_t n;
  const int64_t* toff;
  int64_t nq;
  int max_truth, slots;
  int nk, kmax, kideal;
  int32_t ks[kEvalMaxCutoffs];
  const double *disc, *cum;
  int count_repeats, listed;
  int32_t *hits, *first_hit, *valid;
  float *precision, *recall, *rr, *ap, *ndcg;
  unsigned long long* fail;
};

static size_t eval_lds_bytes(int slots) { return 8 * (size_t)slots + 8 * (size_t)kEvalWords + 16; }
static int eval_slots(int max_truth) {
  const int want = 2 * std::min(std::max(max_truth, 0), kEvalMaxTruth);
  int s = kEvalMinSlots;
  while (s < want) s <<= 1;
  return s;
}

__global__ __launch_bounds__(kBlock) void eval_ranking_kernel(EvalArgs a) {
  constexpr int kPer = kEvalMaxWidth / kBlock;
  extern __shared__ __attribute__((aligned(16))) char eval_lds[];
  int2* tab = (int2*)eval_lds;                                                   // {id, first position}; empty id = -1
  unsigned long long* bits = (unsigned long long*)(eval_lds + 8 * (size_t)a.slots);
  int* s_distinct = (int*)(bits + kEvalWords);
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  for (int64_t q = blockIdx.x; q < a.nq; q += gridDim.x) {  // (q and everything read per query: the same in all threads)
    __syncthreads();  // the previous query's readers are done with the LDS
    const int64_t t0 = a.toff[q], t1 = a.toff[q + 1];
    const bool bad = t0 < 0 || t1 < t0 || t1 > a.n || t1 - t0 > (int64_t)a.max_truth;  // refused on the host
    const int listed = bad ? 0 : (int)(t1 - t0);
    int slots = kEvalMinSlots;
    while (slots < 2 * listed && slots < a.slots) slots <<= 1;
    const unsigned mask = (unsigned)slots - 1u;
    const int shift = __clz(slots) + 1;  // 32 - log2(slots): the hash keeps the product's TOP bits
    for (int i = tid; i < slots; i += kBlock) tab[i] = make_int2(-1, INT32_MAX);
    if (tid < kEvalWords) bits[tid] = 0ull;
    if (tid == 0) *s_distinct = 0;
    __syncthreads();
    int mine = 0;
    unsigned long long f = bad ? kEvalFailOffsets : 0ull;
    for (int i = tid; i < listed; i += kBlock) {
      const int32_t v = a.truth[t0 + i];
      if (v < 0) {
        f |= kEvalFailNegative;
        continue;
      }
      unsigned h = ((unsigned)v * 2654435761u) >> shift;
      int tries = 0;
      for (; tries < slots; ++tries) {
        const int old = atomicCAS(&tab[h].x, -1, v);
        if (old == -1) ++mine;
        if (old == -1 || old == v) break;
        h = (h + 1u) & mask;
      }
      if (tries == slots) f |= kEvalFailFull;
    }
    if (mine) atomicAdd(s_distinct, mine);
    __syncthreads();
    const int distinct = *s_distinct;
    if (distinct > kEvalMaxTruth) f |= kEvalFailFull;
    if (f) atomicOr(a.fail, f);
    int len = a.rec_len ? a.rec_len[q] : a.width;
    len = len < 0 ? 0 : len;
    const int lim = len < a.kmax ? len : a.kmax;  // kmax <= width
    int found[kPer];
#pragma unroll
    for (int c = 0; c < kPer; ++c) {
      found[c] = -1;
      const int r = c * kBlock + tid;
      if (r < lim) {
        const int32_t v = a.rec[q * a.pitch + r];
        if (v >= 0) {
          unsigned h = ((unsigned)v * 2654435761u) >> shift;
          for (int tries = 0; tries < slots; ++tries) {
            const int t = tab[h].x;
            if (t == v) {
              found[c] = (int)h;
              atomicMin(&tab[h].y, r);
            }
            if (t == v || t == -1) break;
            h = (h + 1u) & mask;
          }
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kPer; ++c) {
      if (c * kBlock < lim) {  // whole waves: the ballot needs them
        const int r = c * kBlock + tid;
        const bool hit = found[c] >= 0 && (a.count_repeats || tab[found[c]].y == r);
        const unsigned long long w = __ballot(hit);
        if (lane == 0) bits[r >> 6] = w;
      }
    }
    __syncthreads();
    if (tid == 0) {
      const int n_rel = a.listed ? listed : distinct;
      const bool ok = !bad && n_rel > 0;
      int c = 0, first = 0, j = 0;
      double ap_sum = 0.0, dcg = 0.0;
      auto emit = [&](int jj) {
        const int k = a.ks[jj];
        const int64_t o = q * a.nk + jj;
        a.hits[o] = c;
        a.precision[o] = ok ? (float)((double)c / (double)k) : 0.f;
        a.recall[o] = ok ? (float)((double)c / (double)n_rel) : 0.f;
        a.rr[o] = first ? (float)(1.0 / (double)first) : 0.f;
        if (!a.count_repeats) {
          const int m = k < n_rel ? k : n_rel;
          a.ap[o] = ok ? (float)(ap_sum / (double)m) : 0.f;
          a.ndcg[o] = ok ? (float)(dcg / a.cum[m < a.kideal ? m : a.kideal]) : 0.f;
        }
      };
      if (ok) {
        const int nwords = (lim + 63) >> 6;
        for (int w = 0; w < nwords && j < a.nk; ++w) {
          unsigned long long word = bits[w];
          while (word && j < a.nk) {
            const int r = w * 64 + __ffsll((long long)word);  // 1-based rank
            word &= word - 1ull;
            while (j < a.nk && a.ks[j] < r) emit(j++);
            if (j == a.nk) break;
            ++c;
            if (!first) first = r;
            ap_sum += (double)c / (double)r;
            dcg += a.disc[r - 1];
          }
        }
      }
      while (j < a.nk) emit(j++);
      a.first_hit[q] = first;
      a.valid[q] = ok ? 1 : 0;
    }
  }
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_eval_max_truth(void) { return kEvalMaxTruth; }
int esr_eval_max_width(void) { return kEvalMaxWidth; }

int esr_eval_ranking(const int32_t* rec_ids, int64_t rec_pitch, int width, const int32_t* rec_lengths,
                     const int32_t* truth, int64_t n, const int64_t* truth_offsets, int64_t nq, int max_truth,
                     const int32_t* ks, int nk, const double* disc, const double* cum_disc, int count_repeats,
                     int listed_size, int32_t* hits, int32_t* first_hit, int32_t* valid, float* precision, float* recall,
                     float* rr, float* ap, float* ndcg, unsigned long long* fail, esr_stream_t stream) {
  TraceScope trace_scope_("esr_eval_ranking");
  ESR_REQUIRE(ks && nk >= 1 && nk <= kEvalMaxCutoffs, "esr_eval_ranking: nk=%d cutoffs not in [1, %d] (or null ks)", nk,
              kEvalMaxCutoffs);
  for (int j = 0; j < nk; ++j)
    ESR_REQUIRE(ks[j] >= 1 && (j == 0 || ks[j] > ks[j - 1]),
                "esr_eval_ranking: ks must be strictly ascending and >= 1 (ks[%d]=%d)", j, ks[j]);
  ESR_REQUIRE(width >= 1 && width <= kEvalMaxWidth, "esr_eval_ranking: list width=%d not in [1, %d]", width, kEvalMaxWidth);
  ESR_REQUIRE(rec_pitch >= width, "esr_eval_ranking: row pitch %lld below the width %d", (long long)rec_pitch, width);
  ESR_REQUIRE(nq >= 0 && nq <= (int64_t)INT32_MAX && n >= 0 && max_truth >= 0,
              "esr_eval_ranking: bad sizes nq=%lld n=%lld max_truth=%d", (long long)nq, (long long)n, max_truth);
  ESR_REQUIRE((count_repeats == 0 || count_repeats == 1) && (listed_size == 0 || listed_size == 1),
              "esr_eval_ranking: count_repeats=%d or truth size=%d (0 distinct, 1 listed) is not 0 or 1", count_repeats,
              listed_size);
  if (nq == 0) return ESR_OK;
  ESR_REQUIRE(rec_ids && truth_offsets && disc && cum_disc && fail, "esr_eval_ranking: null pointer");
  ESR_REQUIRE(n == 0 || truth, "esr_eval_ranking: null pointer (truth)");
  ESR_REQUIRE(hits && first_hit && valid && precision && recall && rr, "esr_eval_ranking: null pointer (outputs)");
  ESR_REQUIRE(count_repeats || (ap && ndcg), "esr_eval_ranking: null pointer (ap, ndcg: written unless count_repeats)");
  EvalArgs a;
  a.rec = rec_ids, a.pitch = rec_pitch, a.width = width, a.rec_len = rec_lengths;
  a.truth = truth, a.n = n, a.toff = truth_offsets, a.nq = nq;
  a.max_truth = max_truth, a.slots = eval_slots(max_truth);
  a.nk = nk, a.kmax = std::min(ks[nk - 1], width), a.kideal = std::min(ks[nk - 1], max_truth);
  for (int j = 0; j < kEvalMaxCutoffs; ++j) a.ks[j] = j < nk ? ks[j] : INT32_MAX;
  a.disc = disc, a.cum = cum_disc, a.count_repeats = count_repeats, a.listed = listed_size;
  a.hits = hits, a.first_hit = first_hit, a.valid = valid;
  a.precision = precision, a.recall = recall, a.rr = rr, a.ap = ap, a.ndcg = ndcg, a.fail = fail;
  hipStream_t st = as_stream(stream);
  static bool attr_set = false;  // the largest table and its bitmap are above the 64 KiB a kernel gets unasked
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)eval_ranking_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)eval_lds_bytes(2 * kEvalMaxTruth)) != hipSuccess) {
      set_error("esr_eval_ranking: cannot raise the LDS limit");
      return ESR_ELAUNCH;
    }
    attr_set = true;
  }
  if (hipMemsetAsync(fail, 0, sizeof(unsigned long long), st) != hipSuccess) return check_launch("esr_eval_ranking");
  ESR_KT("eval_ranking", st,
         hipLaunchKernelGGL(eval_ranking_kernel, dim3((int)std::min<int64_t>(kMaxGrid, nq)), dim3(kBlock),
                            eval_lds_bytes(a.slots), st, a));
  return check_launch("esr_eval_ranking");
}

}  // extern "C"
