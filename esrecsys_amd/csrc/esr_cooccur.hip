// The GloVe co-occurrence matrix from token-id streams (the reference's wikipedia/make_cooccurrence.py:33-55, which is
// PySpark dictionary work): esr_cooccur_*.
//   window      position i of a document pairs with j in [max(0, i - W), min(n, i + W)) and adds 1 / |i - j| to the entry
//               (index = t[i], other = t[j]) when t[i] > t[j].  Per unordered position pair (p, q = p + d) that is: the
//               LATER token larger -> 1 / d for d <= W; the EARLIER token larger -> 1 / d for d <= W - 1 (the window
//               reaches W back and W - 1 forward); equal ids never pair; nothing crosses a document boundary.
//   arithmetic  fixed point: with L = lcm(1 .. W) the increment 1 / d is the integer L / d and an entry is a uint64 sum of
//               those -- independent of the order of the atomics and of how the corpus is cut into calls.  lcm(1 .. 22) =
//               232 792 560 < 2^28, so 2^36 window hits fit.  count = (float)((double)sum / (double)L).
//   table       the open-addressing pair table of esr_cooccur_table.h (shared with esr_dice.hip).
// Output order is (index, other) ascending -- slot order is a race -- by two stable passes of esr_segment_sort_ids.
#include "esr_cooccur_table.h"

namespace esr {

constexpr int kCooccurMaxW = 22;

static inline uint64_t lcm_upto(int W) {
  uint64_t l = 1;
  for (uint64_t d = 2; d <= (uint64_t)W; ++d) {
    uint64_t a = l, b = d;
    while (b) {
      const uint64_t r = a % b;
      a = b;
      b = r;
    }
    l = l / a * d;
  }
  return l;
}

__global__ __launch_bounds__(kBlock) void cooccur_init_kernel(CooccurTable t) {
  const int64_t cap = (int64_t)t.mask + 1;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < cap; i += (int64_t)gridDim.x * kBlock) {
    t.keys[i] = kEmptyKey;
    t.sums[i] = 0ull;
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) t.used[threadIdx.x] = 0ull;  // used, fail
}

struct WindowWeights {
  unsigned int w[kCooccurMaxW + 1];  // w[d] = lcm(1 .. W) / d
};

// One lane per position q of [tok_begin, tok_end); it walks the W positions behind q inside q's document.  For one
// distance d every lane of a wave adds the same weight, so equal keys in the wave are merged first (wave_merge_add).
__global__ __launch_bounds__(kBlock) void cooccur_accumulate_kernel(const int32_t* __restrict__ tokens, int64_t N,
                                                                   const int64_t* __restrict__ doc_offsets,
                                                                   int64_t ndocs, int64_t tok_begin, int64_t tok_end,
                                                                   int W, WindowWeights ww, CooccurTable t) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t first = doc_offsets[0], last = doc_offsets[ndocs];
  if (blockIdx.x == 0 && threadIdx.x == 0 && (first < 0 || last > N || first > last)) atomicOr(t.fail, kFailBadOffsets);
  // (whole waves stay in the loop together: wave_merge_add needs every lane of the wave)
  const int64_t span = tok_end - tok_begin;
  const int64_t rounds = (span + (int64_t)gridDim.x * kBlock - 1) / ((int64_t)gridDim.x * kBlock);
  for (int64_t r = 0; r < rounds; ++r) {
    const int64_t q = tok_begin + (r * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
    const bool in_doc = q < tok_end && q >= first && q < last;
    int64_t start = q;
    int32_t tq = 0;
    if (in_doc) {
      start = doc_offsets[doc_of(doc_offsets, 1, ndocs, q) - 1];
      start = start < 0 ? 0 : (start > q ? q : start);        // whatever the offsets hold, every read stays in [0, q]
      tq = tokens[q];
      if (tq < 0) atomicOr(t.fail, kFailNegativeId);
    }
    for (int d = 1; d <= W; ++d) {
      const int64_t p = q - d;
      bool live = in_doc && p >= start && tq >= 0;
      unsigned long long key = 0;
      if (live) {
        const int32_t tp = tokens[p];
        if (tp < 0) atomicOr(t.fail, kFailNegativeId);
        // later token larger: d <= W; earlier token larger: d <= W - 1
        live = tp >= 0 && tp != tq && (tq > tp || d < W);
        const uint32_t hi = (uint32_t)(tq > tp ? tq : tp), lo = (uint32_t)(tq > tp ? tp : tq);
        key = ((unsigned long long)hi << 32) | lo;
      }
      wave_merge_add(t, live, key, ww.w[d], lane);
    }
  }
}

__global__ __launch_bounds__(kBlock) void cooccur_rehash_kernel(CooccurTable src, CooccurTable dst) {
  const int64_t cap = (int64_t)src.mask + 1;
  carry_fail(src, dst);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < cap; i += (int64_t)gridDim.x * kBlock) {
    const unsigned long long k = src.keys[i];
    if (k != kEmptyKey) table_add(dst, k, src.sums[i]);
  }
}

__global__ __launch_bounds__(kBlock) void cooccur_compact_kernel(CooccurTable t, int64_t nnz,
                                                                unsigned long long* __restrict__ counter,
                                                                int32_t* __restrict__ index, int32_t* __restrict__ other,
                                                                unsigned long long* __restrict__ sum) {
  const int64_t cap = (int64_t)t.mask + 1;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < cap; i += (int64_t)gridDim.x * kBlock) {
    const unsigned long long k = t.keys[i];
    if (k == kEmptyKey) continue;
    unsigned long long pos;
    if (!compact_claim(t, counter, nnz, pos)) continue;
    index[pos] = (int32_t)(k >> 32);
    other[pos] = (int32_t)(uint32_t)k;
    sum[pos] = t.sums[i];
  }
}

__global__ __launch_bounds__(kBlock) void cooccur_gather_kernel(const int32_t* __restrict__ src,
                                                               const int32_t* __restrict__ perm, int64_t n,
                                                               int32_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    out[i] = src[perm[i]];
}

// entry k of the result = compacted entry perm1[perm2[k]]
__global__ __launch_bounds__(kBlock) void cooccur_emit_kernel(const int32_t* __restrict__ sorted_other,
                                                             const unsigned long long* __restrict__ sum,
                                                             const int32_t* __restrict__ perm1,
                                                             const int32_t* __restrict__ perm2, int64_t n, double L,
                                                             int32_t* __restrict__ out_other,
                                                             float* __restrict__ out_count) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int32_t a = perm2[i];
    out_other[i] = sorted_other[a];
    out_count[i] = (float)((double)sum[perm1[a]] / L);
  }
}

struct FinalizeWs {
  unsigned long long* counter;
  unsigned long long* sum;
  int32_t *index, *other, *sorted_other, *perm1, *index1, *perm2;
  void* sort_ws;
  size_t sort_ws_bytes;
};
static size_t finalize_layout(int64_t nnz, char* base, FinalizeWs* ws) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return p;
  };
  FinalizeWs w;
  const size_t n = (size_t)std::max<int64_t>(nnz, 1);
  w.counter = (unsigned long long*)take(256);
  w.sum = (unsigned long long*)take(8 * n);
  w.index = (int32_t*)take(4 * n);
  w.other = (int32_t*)take(4 * n);
  w.sorted_other = (int32_t*)take(4 * n);
  w.perm1 = (int32_t*)take(4 * n);
  w.index1 = (int32_t*)take(4 * n);
  w.perm2 = (int32_t*)take(4 * n);
  w.sort_ws_bytes = esr_segment_sort_workspace_bytes(nnz);
  w.sort_ws = take(w.sort_ws_bytes);
  if (ws) *ws = w;
  return off;
}

}  // namespace esr

using namespace esr;

extern "C" {

size_t esr_cooccur_table_bytes(int64_t capacity) {
  if (capacity <= 0) return kCooccurHeaderBytes;
  return kCooccurHeaderBytes + 16 * (size_t)capacity;
}

int esr_cooccur_table_init(void* table, int64_t capacity, esr_stream_t stream) {
  ESR_REQUIRE_TABLE("esr_cooccur_table_init", "capacity", capacity);
  ESR_REQUIRE(table && ((uintptr_t)table & 15) == 0, "esr_cooccur_table_init: null (or misaligned) table");
  hipStream_t st = as_stream(stream);
  ESR_KT("cooccur_init", st,
         hipLaunchKernelGGL(cooccur_init_kernel, dim3(grid_for(capacity)), dim3(kBlock), 0, st,
                            table_view(table, capacity)));
  return check_launch("esr_cooccur_table_init");
}

int esr_cooccur_accumulate(const int32_t* tokens, int64_t N, const int64_t* doc_offsets, int64_t ndocs,
                           int64_t tok_begin, int64_t tok_end, int context_window, void* table, int64_t capacity,
                           esr_stream_t stream) {
  TraceScope trace_scope_("esr_cooccur_accumulate");
  ESR_REQUIRE(context_window >= 1 && context_window <= kCooccurMaxW,
              "esr_cooccur_accumulate: context_window=%d not in [1, %d] (lcm(1..W) must leave room in a uint64 sum)",
              context_window, kCooccurMaxW);
  ESR_REQUIRE_TABLE("esr_cooccur_accumulate", "capacity", capacity);
  ESR_REQUIRE(N >= 0 && ndocs >= 0, "esr_cooccur_accumulate: negative size N=%lld ndocs=%lld", (long long)N,
              (long long)ndocs);
  ESR_REQUIRE(0 <= tok_begin && tok_begin <= tok_end && tok_end <= N,
              "esr_cooccur_accumulate: token range [%lld, %lld) not inside [0, N=%lld)", (long long)tok_begin,
              (long long)tok_end, (long long)N);
  ESR_REQUIRE(table && doc_offsets, "esr_cooccur_accumulate: null pointer");
  if (tok_begin == tok_end || ndocs == 0) return ESR_OK;
  ESR_REQUIRE(tokens, "esr_cooccur_accumulate: null pointer");
  WindowWeights ww;
  const uint64_t L = lcm_upto(context_window);
  ww.w[0] = 0;
  for (int d = 1; d <= kCooccurMaxW; ++d) ww.w[d] = d <= context_window ? (unsigned int)(L / (uint64_t)d) : 0u;
  hipStream_t st = as_stream(stream);
  ESR_KT("cooccur_accumulate", st,
         hipLaunchKernelGGL(cooccur_accumulate_kernel, dim3(grid_for(tok_end - tok_begin)), dim3(kBlock), 0, st, tokens,
                            N, doc_offsets, ndocs, tok_begin, tok_end, context_window, ww, table_view(table, capacity)));
  return check_launch("esr_cooccur_accumulate");
}

int esr_cooccur_rehash(const void* table, int64_t capacity, void* new_table, int64_t new_capacity,
                       esr_stream_t stream) {
  TraceScope trace_scope_("esr_cooccur_rehash");
  ESR_REQUIRE(table_capacity_ok(capacity) && table_capacity_ok(new_capacity) && new_capacity >= capacity,
              "esr_cooccur_rehash: capacities %lld -> %lld must be powers of two >= 2 that do not shrink",
              (long long)capacity, (long long)new_capacity);
  ESR_REQUIRE(table && new_table && table != new_table && ((uintptr_t)new_table & 15) == 0,
              "esr_cooccur_rehash: null, misaligned or aliased table");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(cooccur_init_kernel, dim3(grid_for(new_capacity)), dim3(kBlock), 0, st,
                     table_view(new_table, new_capacity));
  ESR_KT("cooccur_rehash", st,
         hipLaunchKernelGGL(cooccur_rehash_kernel, dim3(grid_for(capacity)), dim3(kBlock), 0, st,
                            table_view(const_cast<void*>(table), capacity), table_view(new_table, new_capacity)));
  return check_launch("esr_cooccur_rehash");
}

size_t esr_cooccur_finalize_workspace_bytes(int64_t nnz) { return finalize_layout(nnz, nullptr, nullptr); }

int esr_cooccur_finalize(void* table, int64_t capacity, int64_t nnz, int64_t num_ids, int context_window,
                         int32_t* index, int32_t* other, float* count, void* workspace, size_t workspace_bytes,
                         esr_stream_t stream) {
  TraceScope trace_scope_("esr_cooccur_finalize");
  ESR_REQUIRE(context_window >= 1 && context_window <= kCooccurMaxW,
              "esr_cooccur_finalize: context_window=%d not in [1, %d]", context_window, kCooccurMaxW);
  ESR_REQUIRE_TABLE("esr_cooccur_finalize", "capacity", capacity);
  ESR_REQUIRE(nnz >= 0 && nnz <= capacity && nnz < ((int64_t)1 << 30) && num_ids > 0 &&
                  num_ids <= ((int64_t)1 << 31),
              "esr_cooccur_finalize: bad sizes nnz=%lld (capacity %lld) num_ids=%lld", (long long)nnz,
              (long long)capacity, (long long)num_ids);
  ESR_REQUIRE(table, "esr_cooccur_finalize: null pointer");
  if (nnz == 0) return ESR_OK;
  ESR_REQUIRE(index && other && count && workspace, "esr_cooccur_finalize: null pointer");
  if (workspace_bytes < finalize_layout(nnz, nullptr, nullptr) || ((uintptr_t)workspace & 15)) {
    set_error("esr_cooccur_finalize: workspace %zu bytes < %zu required (or misaligned)", workspace_bytes,
              finalize_layout(nnz, nullptr, nullptr));
    return ESR_EWORKSPACE;
  }
  FinalizeWs ws;
  finalize_layout(nnz, (char*)workspace, &ws);
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(ws.counter, 0, 256, st) != hipSuccess) return check_launch("esr_cooccur_finalize");
  const int g = grid_for(nnz);
  ESR_KT("cooccur_compact", st,
         hipLaunchKernelGGL(cooccur_compact_kernel, dim3(grid_for(capacity)), dim3(kBlock), 0, st,
                            table_view(table, capacity), nnz, ws.counter, ws.index, ws.other, ws.sum));
  // ascending (index, other): stable by `other`, then stable by `index` of that order
  if (int rc = esr_segment_sort_ids(ws.other, nnz, num_ids, ws.sorted_other, ws.perm1, ws.sort_ws, ws.sort_ws_bytes,
                                    stream))
    return rc;
  hipLaunchKernelGGL(cooccur_gather_kernel, dim3(g), dim3(kBlock), 0, st, (const int32_t*)ws.index,
                     (const int32_t*)ws.perm1, nnz, ws.index1);
  if (int rc = esr_segment_sort_ids(ws.index1, nnz, num_ids, index, ws.perm2, ws.sort_ws, ws.sort_ws_bytes, stream))
    return rc;
  hipLaunchKernelGGL(cooccur_emit_kernel, dim3(g), dim3(kBlock), 0, st, (const int32_t*)ws.sorted_other,
                     (const unsigned long long*)ws.sum, (const int32_t*)ws.perm1, (const int32_t*)ws.perm2, nnz,
                     (double)lcm_upto(context_window), other, count);
  return check_launch("esr_cooccur_finalize");
}

}  // extern "C"
