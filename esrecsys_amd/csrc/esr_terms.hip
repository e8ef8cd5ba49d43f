// Term statistics, the dictionary lookup and tf-idf documents from token-id streams (the reference's
// wikipedia/make_dictionary.py:67-117, token_dictionary.py:58-64 and count_terms.py:32-74, Python dictionary loops
// there): esr_terms_*.  Everything is reduce-by-key on integers in the pair table of esr_cooccur_table.h.
//   accumulate  one lane per token of a launch (whole documents [doc_begin, doc_end)); the SCRATCH table of the launch
//               receives key = document in launch << 32 | id with sum = tf.  The id is the raw id (statistics) or, with
//               a lookup table, the dictionary index of the raw id -- a raw id the lookup does not hold (outside the
//               dictionary, or a stopword the caller left out of it) adds nothing.  Equal keys of a wave are merged by
//               a ballot before the atomic, as cooccur_accumulate_kernel does: a document that is one token repeated
//               100 000 times is 1 563 adds on one slot, not 100 000.
//   fold        statistics: every occupied scratch slot (document, id, tf) adds tf to the persistent key id << 32 | 0
//               (frequency) and 1 to id << 32 | 1 (document frequency).  Contention on a hot id is per document, and
//               nothing persistent grows with the number of documents.
//   stats       the persistent table's ids with both sums as uint64 (esr_cooccur_finalize would round them to float);
//               the caller sorts the ids with esr_segment_sort_ids.
//   lookup      a pair table with key = raw id and sum = dictionary index, built once per dictionary; no dense
//               2^31-entry array.  esr_terms_lookup maps a token array through it (index_of / embedding index).
//   tfidf rows  after esr_cooccur_finalize has ordered the scratch keys by (document, index) and esr_run_offsets has cut
//               them into rows: one wave per row reads every tf back from the scratch table as uint64, forms
//               tf * idf[index] in fp64, sums the squares lane-strided and by a fixed butterfly, and stores
//               float32(tfidf * (1 / sqrt(norm))).  No float atomics: two runs give the same bits.
// uint64 counts throughout: nothing depends on the order of the atomics or on how the corpus is cut into launches.
// Every loop is bounded by a size checked on the host or by a table's capacity; no kernel waits on another workgroup.
#include "esr_cooccur_table.h"

namespace esr {

constexpr unsigned long long kFailBadBucket = 32;  // esr_terms_lookup's own word: an oov bucket outside [0, 65536)

__global__ __launch_bounds__(kBlock) void terms_accumulate_kernel(const int32_t* __restrict__ tokens,
                                                                 const int64_t* __restrict__ doc_offsets,
                                                                 int64_t doc_begin, int64_t doc_end, int64_t tok_begin,
                                                                 int64_t tok_end, CooccurTable lookup, int use_lookup,
                                                                 CooccurTable t) {
  const int lane = threadIdx.x & (kWave - 1);
  // the host planned [tok_begin, tok_end) (inside [0, N)) from ITS copy of the offsets: the device's must agree
  if (doc_offsets[doc_begin] != tok_begin || doc_offsets[doc_end] != tok_end) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(t.fail, kFailBadOffsets);
    return;
  }
  // (whole waves stay in the loop together: wave_merge_add needs every lane of the wave)
  const int64_t span = tok_end - tok_begin;
  const int64_t rounds = (span + (int64_t)gridDim.x * kBlock - 1) / ((int64_t)gridDim.x * kBlock);
  for (int64_t r = 0; r < rounds; ++r) {
    const int64_t q = tok_begin + (r * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
    bool live = q < tok_end;
    unsigned long long key = 0;
    if (live) {
      const int64_t doc = doc_of(doc_offsets, doc_begin + 1, doc_end, q) - 1 - doc_begin;  // in the launch
      const int32_t tok = tokens[q];
      unsigned long long id = (unsigned long long)(uint32_t)tok;
      if (tok < 0) {
        atomicOr(t.fail, kFailNegativeId);
        live = false;
      } else if (use_lookup) {
        live = table_find(lookup, id, id);
      }
      key = ((unsigned long long)doc << 32) | id;
    }
    wave_merge_add(t, live, key, 1ull, lane);
  }
}

__global__ __launch_bounds__(kBlock) void terms_fold_kernel(CooccurTable scratch, CooccurTable t) {
  const int64_t cap = (int64_t)scratch.mask + 1;
  carry_fail(scratch, t);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < cap; i += (int64_t)gridDim.x * kBlock) {
    const unsigned long long k = scratch.keys[i];
    if (k == kEmptyKey) continue;
    const unsigned long long id = k << 32;
    table_add(t, id, scratch.sums[i]);
    table_add(t, id | 1ull, 1ull);
  }
}

__global__ __launch_bounds__(kBlock) void terms_stats_kernel(CooccurTable t, int64_t n_ids,
                                                            unsigned long long* __restrict__ counter,
                                                            int32_t* __restrict__ ids, int64_t* __restrict__ frequency,
                                                            int64_t* __restrict__ doc_frequency) {
  const int64_t cap = (int64_t)t.mask + 1;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < cap; i += (int64_t)gridDim.x * kBlock) {
    const unsigned long long k = t.keys[i];
    if (k == kEmptyKey || (uint32_t)k != 0u) continue;
    unsigned long long pos;
    if (!compact_claim(t, counter, n_ids, pos)) continue;
    unsigned long long df = 0;
    table_find(t, k | 1ull, df);
    ids[pos] = (int32_t)(k >> 32);
    frequency[pos] = (int64_t)t.sums[i];
    doc_frequency[pos] = (int64_t)df;
  }
}

__global__ __launch_bounds__(kBlock) void terms_lookup_build_kernel(const int32_t* __restrict__ keys,
                                                                   const int32_t* __restrict__ values, int64_t K,
                                                                   CooccurTable t) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < K; i += (int64_t)gridDim.x * kBlock) {
    const int32_t k = keys[i], v = values[i];
    if (k < 0 || v < 0) {
      atomicOr(t.fail, kFailNegativeId);
      continue;
    }
    table_add(t, (unsigned long long)(uint32_t)k, (unsigned long long)(uint32_t)v);
  }
}

// mode 0: the dictionary index, -1 outside.  mode 1: 1 + index, and 1 + size + bucket outside (bucket = oov_bucket[i],
// or the raw id's low 16 bits without one).
__global__ __launch_bounds__(kBlock) void terms_lookup_kernel(const int32_t* __restrict__ tokens, int64_t N,
                                                             CooccurTable lookup, int mode, int32_t size,
                                                             const int32_t* __restrict__ oov_bucket,
                                                             int32_t* __restrict__ out,
                                                             unsigned long long* __restrict__ fail) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < N; i += (int64_t)gridDim.x * kBlock) {
    const int32_t tok = tokens[i];
    unsigned long long index = 0;
    const bool found = tok >= 0 && table_find(lookup, (unsigned long long)(uint32_t)tok, index);
    if (tok < 0) atomicOr(fail, kFailNegativeId);
    int32_t r;
    if (mode == 0) {
      r = found ? (int32_t)index : -1;
    } else if (found) {
      r = 1 + (int32_t)index;
    } else {
      int32_t bucket = tok & 0xFFFF;
      if (oov_bucket) {
        bucket = oov_bucket[i];
        if (bucket < 0 || bucket > 0xFFFF) {
          atomicOr(fail, kFailBadBucket);
          bucket = 0;
        }
      }
      r = 1 + size + bucket;
    }
    out[i] = r;
  }
}

__device__ __forceinline__ double wave_sum_fixed(double v) {  // the same tree in every run
#pragma unroll
  for (int s = 1; s < kWave; s <<= 1) v += __shfl_xor(v, s, kWave);
  return v;
}

// Row r = entries [row_off[r], row_off[r + 1]) of `index` (ascending inside a row); its tf values sit in the scratch
// table under r << 32 | index.  One wave per row.
__global__ __launch_bounds__(kBlock) void terms_tfidf_rows_kernel(CooccurTable scratch,
                                                                 const int32_t* __restrict__ index,
                                                                 const int32_t* __restrict__ row_off, int64_t nrows,
                                                                 int64_t nnz, const double* __restrict__ idf, int64_t K,
                                                                 float* __restrict__ out) {
#pragma clang fp contract(off)  // tfidf * tfidf and the add round separately, as the reference's Python floats do
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
  const int64_t nwaves = (int64_t)gridDim.x * (kBlock / kWave);
  for (int64_t r = wave; r < nrows; r += nwaves) {  // r is the same in every lane of a wave
    int64_t a = row_off[r], b = row_off[r + 1];
    a = a < 0 ? 0 : (a > nnz ? nnz : a);  // whatever the offsets hold, every access stays in [0, nnz)
    b = b < a ? a : (b > nnz ? nnz : b);
    double acc = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
      const double norm = pass ? wave_sum_fixed(acc) : 0.0;
      const double inorm = norm > 0.0 ? 1.0 / sqrt(norm) : 0.0;
      for (int64_t i = a + lane; i < b; i += kWave) {
        const int32_t ix = index[i];
        unsigned long long tf = 0;
        double v = 0.0;
        if (ix >= 0 && ix < K && table_find(scratch, ((unsigned long long)r << 32) | (uint32_t)ix, tf))
          v = (double)tf * idf[ix];
        if (pass) out[i] = (float)(v * inorm);
        else acc += v * v;
      }
    }
  }
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_terms_accumulate(const int32_t* tokens, int64_t N, const int64_t* doc_offsets, int64_t ndocs, int64_t doc_begin,
                         int64_t doc_end, int64_t tok_begin, int64_t tok_end, const void* lookup,
                         int64_t lookup_capacity, void* scratch, int64_t capacity, esr_stream_t stream) {
  TraceScope trace_scope_("esr_terms_accumulate");
  ESR_REQUIRE_TABLE("esr_terms_accumulate", "capacity", capacity);
  if (lookup) ESR_REQUIRE_TABLE("esr_terms_accumulate", "lookup_capacity", lookup_capacity);
  ESR_REQUIRE(N >= 0 && ndocs >= 0, "esr_terms_accumulate: negative size N=%lld ndocs=%lld", (long long)N,
              (long long)ndocs);
  ESR_REQUIRE(0 <= doc_begin && doc_begin <= doc_end && doc_end <= ndocs,
              "esr_terms_accumulate: document range [%lld, %lld) not inside [0, ndocs=%lld)", (long long)doc_begin,
              (long long)doc_end, (long long)ndocs);
  ESR_REQUIRE(doc_end - doc_begin <= (int64_t)INT32_MAX, "esr_terms_accumulate: %lld documents in one call, at most 2^31 - 1",
              (long long)(doc_end - doc_begin));
  ESR_REQUIRE(0 <= tok_begin && tok_begin <= tok_end && tok_end <= N,
              "esr_terms_accumulate: token range [%lld, %lld) not inside [0, N=%lld)", (long long)tok_begin,
              (long long)tok_end, (long long)N);
  ESR_REQUIRE(scratch && doc_offsets, "esr_terms_accumulate: null pointer");
  if (tok_begin == tok_end || doc_begin == doc_end) return ESR_OK;
  ESR_REQUIRE(tokens, "esr_terms_accumulate: null pointer");
  hipStream_t st = as_stream(stream);
  const CooccurTable lk = lookup ? table_view(const_cast<void*>(lookup), lookup_capacity) : CooccurTable{};
  ESR_KT("terms_accumulate", st,
         hipLaunchKernelGGL(terms_accumulate_kernel, dim3(grid_for(tok_end - tok_begin)), dim3(kBlock), 0, st, tokens,
                            doc_offsets, doc_begin, doc_end, tok_begin, tok_end, lk, lookup ? 1 : 0,
                            table_view(scratch, capacity)));
  return check_launch("esr_terms_accumulate");
}

int esr_terms_fold(const void* scratch, int64_t scratch_capacity, void* table, int64_t capacity, esr_stream_t stream) {
  TraceScope trace_scope_("esr_terms_fold");
  ESR_REQUIRE(table_capacity_ok(scratch_capacity) && table_capacity_ok(capacity),
              "esr_terms_fold: capacities %lld, %lld must be powers of two >= 2", (long long)scratch_capacity,
              (long long)capacity);
  ESR_REQUIRE(scratch && table && scratch != table, "esr_terms_fold: null or aliased table");
  hipStream_t st = as_stream(stream);
  ESR_KT("terms_fold", st,
         hipLaunchKernelGGL(terms_fold_kernel, dim3(grid_for(scratch_capacity)), dim3(kBlock), 0, st,
                            table_view(const_cast<void*>(scratch), scratch_capacity), table_view(table, capacity)));
  return check_launch("esr_terms_fold");
}

int esr_terms_stats(void* table, int64_t capacity, int64_t n_ids, int32_t* ids, int64_t* frequency,
                    int64_t* doc_frequency, void* counter, esr_stream_t stream) {
  TraceScope trace_scope_("esr_terms_stats");
  ESR_REQUIRE_TABLE("esr_terms_stats", "capacity", capacity);
  ESR_REQUIRE(n_ids >= 0 && 2 * n_ids <= capacity, "esr_terms_stats: n_ids=%lld needs two slots each of capacity %lld",
              (long long)n_ids, (long long)capacity);
  ESR_REQUIRE(table, "esr_terms_stats: null pointer");
  if (n_ids == 0) return ESR_OK;
  ESR_REQUIRE(ids && frequency && doc_frequency && counter && ((uintptr_t)counter & 7) == 0,
              "esr_terms_stats: null (or misaligned) pointer");
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(counter, 0, 8, st) != hipSuccess) return check_launch("esr_terms_stats");
  ESR_KT("terms_stats", st,
         hipLaunchKernelGGL(terms_stats_kernel, dim3(grid_for(capacity)), dim3(kBlock), 0, st,
                            table_view(table, capacity), n_ids, (unsigned long long*)counter, ids, frequency,
                            doc_frequency));
  return check_launch("esr_terms_stats");
}

int esr_terms_lookup_build(const int32_t* keys, const int32_t* values, int64_t K, void* table, int64_t capacity,
                           esr_stream_t stream) {
  TraceScope trace_scope_("esr_terms_lookup_build");
  ESR_REQUIRE(table_capacity_ok(capacity) && K >= 0 && 2 * K <= capacity,
              "esr_terms_lookup_build: capacity=%lld must be a power of two >= max(2, 2 K), K=%lld", (long long)capacity,
              (long long)K);
  ESR_REQUIRE(table, "esr_terms_lookup_build: null pointer");
  if (K == 0) return ESR_OK;
  ESR_REQUIRE(keys && values, "esr_terms_lookup_build: null pointer");
  hipStream_t st = as_stream(stream);
  ESR_KT("terms_lookup_build", st,
         hipLaunchKernelGGL(terms_lookup_build_kernel, dim3(grid_for(K)), dim3(kBlock), 0, st, keys, values, K,
                            table_view(table, capacity)));
  return check_launch("esr_terms_lookup_build");
}

int esr_terms_lookup(const int32_t* tokens, int64_t N, const void* lookup, int64_t lookup_capacity, int mode,
                     int32_t size, const int32_t* oov_bucket, int32_t* out, void* fail, esr_stream_t stream) {
  TraceScope trace_scope_("esr_terms_lookup");
  ESR_REQUIRE_TABLE("esr_terms_lookup", "lookup_capacity", lookup_capacity);
  ESR_REQUIRE(mode == 0 || mode == 1, "esr_terms_lookup: mode=%d not 0 (index) or 1 (embedding index)", mode);
  ESR_REQUIRE(N >= 0 && size >= 0 && size <= INT32_MAX - 65537, "esr_terms_lookup: bad sizes N=%lld size=%d",
              (long long)N, (int)size);
  ESR_REQUIRE(lookup && fail && ((uintptr_t)fail & 7) == 0, "esr_terms_lookup: null (or misaligned) pointer");
  if (N == 0) return ESR_OK;
  ESR_REQUIRE(tokens && out, "esr_terms_lookup: null pointer");
  hipStream_t st = as_stream(stream);
  ESR_KT("terms_lookup", st,
         hipLaunchKernelGGL(terms_lookup_kernel, dim3(grid_for(N)), dim3(kBlock), 0, st, tokens, N,
                            table_view(const_cast<void*>(lookup), lookup_capacity), mode, size, oov_bucket, out,
                            (unsigned long long*)fail));
  return check_launch("esr_terms_lookup");
}

int esr_terms_tfidf_rows(const void* scratch, int64_t capacity, const int32_t* index, const int32_t* row_off,
                         int64_t nrows, int64_t nnz, const double* idf, int64_t K, float* tfidf, esr_stream_t stream) {
  TraceScope trace_scope_("esr_terms_tfidf_rows");
  ESR_REQUIRE_TABLE("esr_terms_tfidf_rows", "capacity", capacity);
  ESR_REQUIRE(nrows >= 0 && nrows <= (int64_t)INT32_MAX && nnz >= 0 && nnz <= (int64_t)INT32_MAX && K >= 0,
              "esr_terms_tfidf_rows: bad sizes nrows=%lld nnz=%lld K=%lld", (long long)nrows, (long long)nnz,
              (long long)K);
  ESR_REQUIRE(scratch, "esr_terms_tfidf_rows: null pointer");
  if (nrows == 0 || nnz == 0) return ESR_OK;
  ESR_REQUIRE(index && row_off && idf && tfidf, "esr_terms_tfidf_rows: null pointer");
  hipStream_t st = as_stream(stream);
  const int grid = (int)std::min<int64_t>(kMaxGrid, cdiv(nrows, kBlock / kWave));
  ESR_KT("terms_tfidf_rows", st,
         hipLaunchKernelGGL(terms_tfidf_rows_kernel, dim3(grid), dim3(kBlock), 0, st,
                            table_view(const_cast<void*>(scratch), capacity), index, row_off, nrows, nnz, idf, K,
                            tfidf));
  return check_launch("esr_terms_tfidf_rows");
}

}  // extern "C"
