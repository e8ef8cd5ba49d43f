// The set co-occurrence (Dice) matrix from id sets (the reference's wikipedia/make_dice.py:41-54, PySpark dictionary work
// there): esr_dice_*.
//   pairs       a document is the SET of its ids; with u = its sorted distinct ids every i < j adds 1 to the entry
//               (index = u[i], other = u[j]) -- index < other, the opposite orientation to the windowed matrix.  Fewer
//               than two distinct ids add nothing.
//   frequency   in the same pass every distinct id of a document adds 1 to the DIAGONAL key id << 32 | id, which no pair
//               can make: the number of documents whose set holds the id, kept in the same table.
//   arithmetic  uint64 counts in the pair table of esr_cooccur_table.h: independent of the order of the atomics and of how
//               the documents are cut into calls.  esr_cooccur_finalize with context_window = 1 (lcm = 1) orders the keys.
//   cap         a document holds at most kDiceMaxDoc ids (its sort lives in LDS); a longer one raises failure bit 16 and is
//               skipped whole -- never truncated.  This is the one deviation from the reference.
// Two launches per call.  dice_small_kernel: one wave per document of at most 64 ids (sorted and made unique across the
// lanes, no LDS) -- and for every longer document the list of its (document, triangle tile) work items.  dice_large_kernel:
// one workgroup per work item sorts the document in LDS and emits ITS tile of the triangle, so a 4096-id document's 8.4 M
// pairs are spread over 256 workgroups (each repeats the 16 KiB sort: ~80 LDS passes against 32 768 table accesses).
// No kernel waits on another workgroup; every loop is bounded by a size checked on the host or by the table's capacity.
#include "esr_cooccur_table.h"

namespace esr {

constexpr int kDiceMaxDoc = 4096;
constexpr int kDiceWaveDoc = kWave;       // at most this many ids: the wave path
constexpr int kDiceTilePairs = 32768;     // pairs of a large document's triangle per workgroup
constexpr int kDiceMaxTiles = (int)(((int64_t)kDiceMaxDoc * (kDiceMaxDoc - 1) / 2 + kDiceTilePairs - 1) / kDiceTilePairs);
constexpr int kDiceChunks = kDiceMaxDoc / kBlock;  // ids per thread of the large path
constexpr uint32_t kPadId = 0xFFFFFFFFu;  // sorts behind every id >= 0

struct DiceWork {
  int32_t doc;   // relative to doc_begin
  int32_t tile;
};
struct DiceWs {
  unsigned long long* count;  // work items appended
  DiceWork* work;
  int64_t cap;
};
static inline int64_t dice_work_items(int64_t N) {
  // a document of n > 64 ids has ceil(n (n - 1) / 2 / kDiceTilePairs) < n / 16 + 1 tiles, and there are at most N / 65
  return N / 16 + N / 64 + 2;
}
static size_t dice_layout(int64_t N, char* base, DiceWs* ws) {
  const int64_t items = dice_work_items(std::max<int64_t>(N, 0));
  if (ws) {
    ws->count = (unsigned long long*)base;
    ws->work = (DiceWork*)(base + 256);
    ws->cap = items;
  }
  return 256 + align_up(sizeof(DiceWork) * (size_t)items, 256);
}

// pair p of the triangle, column by column: p = j (j - 1) / 2 + i with i < j.  p < 2^23: the double root is exact at the
// column starts ((2 j - 1)^2 is a perfect square) and monotone between them; the two corrections are a safety net.
__device__ __forceinline__ void tri_decode(uint32_t p, int& i, int& j) {
  int c = (int)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5);
  if ((uint32_t)c * (uint32_t)(c - 1) / 2 > p) --c;
  if ((uint32_t)(c + 1) * (uint32_t)c / 2 <= p) ++c;
  j = c;
  i = (int)(p - (uint32_t)c * (uint32_t)(c - 1) / 2);
}

// ascending across the 64 lanes (bitonic network, 21 exchanges)
__device__ __forceinline__ uint32_t wave_sort(uint32_t v, int lane) {
#pragma unroll
  for (int k = 2; k <= kWave; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint32_t o = xor_lane(v, j);
      const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
      v = keep_min ? (v < o ? v : o) : (v < o ? o : v);
    }
  }
  return v;
}

__device__ __forceinline__ unsigned long long pair_key(uint32_t lo, uint32_t hi) {
  return ((unsigned long long)lo << 32) | hi;
}

// [a, a + n) of document d, or false (and the failure bit) when the offsets or the length cannot be used
__device__ __forceinline__ bool dice_doc(const int64_t* __restrict__ doc_offsets, int64_t N, int64_t d, bool report,
                                         const CooccurTable& t, int64_t& a, int& n) {
  a = doc_offsets[d];
  const int64_t b = doc_offsets[d + 1];
  if (a < 0 || b > N || a > b) {
    if (report) atomicOr(t.fail, kFailBadOffsets);
    return false;
  }
  if (b - a > kDiceMaxDoc) {
    if (report) atomicOr(t.fail, kFailDocTooLong);
    return false;
  }
  n = (int)(b - a);
  return true;
}

__global__ __launch_bounds__(kBlock) void dice_small_kernel(const int32_t* __restrict__ indices, int64_t N,
                                                           const int64_t* __restrict__ doc_offsets, int64_t doc_begin,
                                                           int64_t doc_end, CooccurTable t, DiceWs ws) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
  const int64_t nwaves = (int64_t)gridDim.x * (kBlock / kWave);
  for (int64_t d = doc_begin + wave; d < doc_end; d += nwaves) {  // d is the same in every lane of a wave
    int64_t a;
    int n;
    if (!dice_doc(doc_offsets, N, d, lane == 0, t, a, n)) continue;
    if (n > kDiceWaveDoc) {
      if (lane == 0) {
        const int tiles = (n * (n - 1) / 2 + kDiceTilePairs - 1) / kDiceTilePairs;  // n <= 4096: fits an int
        const unsigned long long pos = atomicAdd(ws.count, (unsigned long long)tiles);
        if (pos + (unsigned long long)tiles > (unsigned long long)ws.cap) {
          atomicOr(t.fail, kFailBadOffsets);  // more ids in the documents than N: the offsets overlap
        } else {
          for (int k = 0; k < tiles; ++k) ws.work[pos + k] = DiceWork{(int32_t)(d - doc_begin), k};
        }
      }
      continue;
    }
    uint32_t v = lane < n ? (uint32_t)indices[a + lane] : kPadId;
    if (__ballot(lane < n && (int32_t)v < 0)) {
      if (lane == 0) atomicOr(t.fail, kFailNegativeId);
      continue;
    }
    v = wave_sort(v, lane);
    const uint32_t prev = (uint32_t)__shfl_up((int)v, 1, kWave);
    const bool head = v != kPadId && (lane == 0 || v != prev);
    const int u = __popcll(__ballot(head));
    v = wave_sort(head ? v : kPadId, lane);  // the distinct ids, ascending, in lanes [0, u)
    if (lane < u) table_add(t, pair_key(v, v), 1ull);
    const int P = u * (u - 1) / 2;
    for (int p0 = 0; p0 < P; p0 += kWave) {  // inside a document all keys are distinct: lane by lane
      const int p = p0 + lane;
      int i = 0, j = 0;
      if (p < P) tri_decode((uint32_t)p, i, j);
      const uint32_t lo = (uint32_t)__shfl((int)v, i, kWave), hi = (uint32_t)__shfl((int)v, j, kWave);
      if (p < P) table_add(t, pair_key(lo, hi), 1ull);
    }
  }
}

__global__ __launch_bounds__(kBlock) void dice_large_kernel(const int32_t* __restrict__ indices, int64_t N,
                                                           const int64_t* __restrict__ doc_offsets, int64_t doc_begin,
                                                           int64_t doc_end, CooccurTable t, DiceWs ws) {
  __shared__ uint32_t s[kDiceMaxDoc];
  __shared__ int s_cnt[kDiceChunks * (kBlock / kWave)];  // heads per (chunk, wave), then their exclusive sums
  __shared__ int s_u;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
  const unsigned long long appended = *ws.count;
  const int64_t nwork = (int64_t)(appended < (unsigned long long)ws.cap ? appended : (unsigned long long)ws.cap);
  // (every condition up to the first barrier is the same in all threads of the workgroup)
  for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
    __syncthreads();  // the previous item's readers are done with s
    const DiceWork item = ws.work[w];
    if (item.doc < 0 || item.tile < 0 || item.tile >= kDiceMaxTiles || doc_begin + item.doc >= doc_end) continue;
    int64_t a;
    int n;
    if (!dice_doc(doc_offsets, N, doc_begin + item.doc, false, t, a, n) || n <= kDiceWaveDoc) continue;
    int m = kBlock;  // the sort's size: a power of two, a multiple of the workgroup
    while (m < n) m <<= 1;
    bool negative = false;
    for (int i = tid; i < m; i += kBlock) {
      const uint32_t v = i < n ? (uint32_t)indices[a + i] : kPadId;
      negative |= i < n && (int32_t)v < 0;
      s[i] = v;
    }
    if (__syncthreads_or(negative)) {
      if (tid == 0) atomicOr(t.fail, kFailNegativeId);
      continue;
    }
    // bitonic sort, ascending: exchange x pairs positions lo (bit j clear) and lo + j; consecutive x are consecutive
    // words of both, so a wave's accesses fall into distinct banks
    for (int k = 2; k <= m; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int x = tid; x < m / 2; x += kBlock) {
          const int lo = 2 * x - (x & (j - 1)), hi = lo + j;
          const uint32_t p = s[lo], q = s[hi];
          if ((p > q) == ((lo & k) == 0)) {
            s[lo] = q;
            s[hi] = p;
          }
        }
        __syncthreads();
      }
    }
    // distinct ids to the front, in place.  Position c * kBlock + tid (conflict-free); an id is a head when it differs
    // from its left neighbour; a head's rank = heads of earlier (chunk, wave) groups + earlier heads in its own.
    const int chunks = m / kBlock;
    uint32_t v[kDiceChunks];
    unsigned heads = 0;
#pragma unroll
    for (int c = 0; c < kDiceChunks; ++c) {
      v[c] = kPadId;
      if (c < chunks) {
        const int pos = c * kBlock + tid;
        v[c] = s[pos];
        const bool head = v[c] != kPadId && (pos == 0 || v[c] != s[pos - 1]);
        heads |= (unsigned)head << c;
        const int cnt = __popcll(__ballot(head));
        if (lane == 0) s_cnt[c * (kBlock / kWave) + wid] = cnt;
      }
    }
    __syncthreads();  // every id is in a register now: s may be overwritten
    if (wid == 0) {   // 64 = kDiceChunks * waves counts: one wave scans them
      const int groups = chunks * (kBlock / kWave);
      const int own = lane < groups ? s_cnt[lane] : 0;
      int incl = own;
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
        const int up = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += up;
      }
      if (lane < groups) s_cnt[lane] = incl - own;
      if (lane == kWave - 1) s_u = incl;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kDiceChunks; ++c) {
      if (c < chunks) {
        const bool head = (heads >> c) & 1u;
        const unsigned long long mask = __ballot(head);
        if (head) s[s_cnt[c * (kBlock / kWave) + wid] + __popcll(mask & ((1ull << lane) - 1ull))] = v[c];
      }
    }
    __syncthreads();
    const int u = s_u;
    if (item.tile == 0)
      for (int i = tid; i < u; i += kBlock) table_add(t, pair_key(s[i], s[i]), 1ull);
    const int64_t P = (int64_t)u * (u - 1) / 2;
    const int64_t p0 = (int64_t)item.tile * kDiceTilePairs;
    const int64_t p1 = P < p0 + kDiceTilePairs ? P : p0 + kDiceTilePairs;
    for (int64_t p = p0 + tid; p < p1; p += kBlock) {
      int i, j;
      tri_decode((uint32_t)p, i, j);
      table_add(t, pair_key(s[i], s[j]), 1ull);
    }
  }
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_dice_max_doc(void) { return kDiceMaxDoc; }

size_t esr_dice_workspace_bytes(int64_t N) { return dice_layout(N, nullptr, nullptr); }

int esr_dice_accumulate(const int32_t* indices, int64_t N, const int64_t* doc_offsets, int64_t ndocs,
                        int64_t doc_begin, int64_t doc_end, void* table, int64_t capacity, void* workspace,
                        size_t workspace_bytes, esr_stream_t stream) {
  TraceScope trace_scope_("esr_dice_accumulate");
  ESR_REQUIRE_TABLE("esr_dice_accumulate", "capacity", capacity);
  ESR_REQUIRE(N >= 0 && ndocs >= 0, "esr_dice_accumulate: negative size N=%lld ndocs=%lld", (long long)N,
              (long long)ndocs);
  ESR_REQUIRE(0 <= doc_begin && doc_begin <= doc_end && doc_end <= ndocs,
              "esr_dice_accumulate: document range [%lld, %lld) not inside [0, ndocs=%lld)", (long long)doc_begin,
              (long long)doc_end, (long long)ndocs);
  ESR_REQUIRE(doc_end - doc_begin <= (int64_t)INT32_MAX,
              "esr_dice_accumulate: %lld documents in one call, at most 2^31 - 1 (a document holds at most %d ids)",
              (long long)(doc_end - doc_begin), kDiceMaxDoc);
  ESR_REQUIRE(table && doc_offsets, "esr_dice_accumulate: null pointer");
  if (doc_begin == doc_end || N == 0) return ESR_OK;
  ESR_REQUIRE(indices && workspace, "esr_dice_accumulate: null pointer");
  if (workspace_bytes < dice_layout(N, nullptr, nullptr) || ((uintptr_t)workspace & 15)) {
    set_error("esr_dice_accumulate: workspace %zu bytes < %zu required (or misaligned)", workspace_bytes,
              dice_layout(N, nullptr, nullptr));
    return ESR_EWORKSPACE;
  }
  DiceWs ws;
  dice_layout(N, (char*)workspace, &ws);
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(ws.count, 0, 256, st) != hipSuccess) return check_launch("esr_dice_accumulate");
  const CooccurTable t = table_view(table, capacity);
  const int small_grid = (int)std::min<int64_t>(kMaxGrid, cdiv(doc_end - doc_begin, kBlock / kWave));
  ESR_KT("dice_small", st,
         hipLaunchKernelGGL(dice_small_kernel, dim3(small_grid), dim3(kBlock), 0, st, indices, N, doc_offsets,
                            doc_begin, doc_end, t, ws));
  // the work list's length stays on the device: a grid that covers its bound, workgroups without an item leave at once
  const int large_grid = (int)std::min<int64_t>(kMaxGrid, ws.cap);
  ESR_KT("dice_large", st,
         hipLaunchKernelGGL(dice_large_kernel, dim3(large_grid), dim3(kBlock), 0, st, indices, N, doc_offsets,
                            doc_begin, doc_end, t, ws));
  return check_launch("esr_dice_accumulate");
}

}  // extern "C"
