// Item-to-item neighbours from a pair table's (index, other, count) entries and an item-kNN recommender over the result:
// esr_neighbours_* and esr_itemknn_* (the reference's wikipedia/dump_dice.py:33-51 ranks the partners of a row by Dice
// score; train_txt2url.py's url_triplet_generator uses the same arithmetic).
//   row         of item x = ids[r]: the entries with index == x (orientation "stored"), or with index == x or other == x
//               and the partner at the other end ("both": the symmetric matrix the half table stands for).
//   score       dice: count / (df[other] + df[index]) in f32, one add and one correctly rounded division -- the bits of
//               make_dice.dice_scores; count: the joint count itself.
//   order       score descending, then partner id ascending: ONE uint64 per entry, (inverted order-preserving score bits)
//               << 32 | partner, ascending.  Partners are distinct inside a row, so the keys are and the k smallest of a
//               row are a pure function of the input: nothing depends on atomic order, on the grid or on the launch cut.
//   passes      degree (ids looked up by binary search, one integer atomic per end) -> exclusive scan -> fill (a row's
//               slots are handed out by an integer atomic: the order inside a list is arbitrary, the select fixes it)
//               -> select, by row length (nb_row_class, the ONE statement of the boundaries for host and kernels):
//                 <= 16    four rows per wave, each sorted across its 16 lanes      } bitonic network over DPP / swizzle /
//                 <= 64    one row per wave, sorted across the 64 lanes            } permlane exchanges, no LDS
//                 <= 2048  one workgroup per row: bitonic sort in LDS (24 KiB)
//                 above    one workgroup per row: 8-bit radix select of the k-th key over the row in global memory
//                          (8 passes), then the <= k keys at or below it are collected into LDS and sorted there.
//               Rows above 64 entries are listed by the scan (there are at most entries / 65 of them); the two wave
//               classes share a kernel that walks the rows four at a time and packs a quad whose rows all fit 16 lanes.
//   recommend   one workgroup per query: gather the neighbour lists of its history rows into LDS keyed (candidate,
//               history position * width + column), sort, sum every run of one candidate left to right IN THAT ORDER
//               (f32, one thread per run), drop history members (binary search in the sorted history), sort by
//               (score descending, candidate ascending), emit k.  The key fixes the summation order: bit-reproducible.
// No kernel waits on another workgroup; every loop is bounded by a size checked on the host or read from the scan.
#include "esr_cooccur_table.h"
#include "esr_rank_keys.h"  // the order key, find_id, lds_sort: shared with esr_ratings.hip

namespace esr {

constexpr int kNbPackRow = 16;                // four such rows share a wave
constexpr int kNbWaveRow = kWave;             // one wave, registers
constexpr int kNbBlockRow = 2048;             // one workgroup, LDS
constexpr int kNbClasses = 4;
constexpr int kItemKnnMaxEntries = 2048;      // history length x table width of one query: what the workgroup sorts
constexpr int kItemKnnMaxWidth = 1024;
constexpr unsigned long long kFailMissingId = 64;  // beside the pair table's bits 1..32
constexpr int kScanItems = 8, kScanTile = kBlock * kScanItems;

// the select class of a row of `len` entries: 0 packed wave, 1 wave, 2 workgroup, 3 streaming
__host__ __device__ inline int nb_row_class(int64_t len) {
  return len <= kNbPackRow ? 0 : len <= kNbWaveRow ? 1 : len <= kNbBlockRow ? 2 : 3;
}
static inline int nb_plan_bounds(int32_t* b) {  // the largest length of every class but the last
  b[0] = kNbPackRow, b[1] = kNbWaveRow, b[2] = kNbBlockRow;
  return kNbClasses - 1;
}

struct NbWs {
  unsigned long long* head;   // word 0: failure bits, word 1: rows listed as long
  int32_t *pos_i, *pos_o;     // the rows of an entry's two ends, -1: not in ids
  uint32_t* deg;              // entries per row; counted down to 0 again by the fill
  int64_t* offsets;           // [u + 1]
  unsigned long long* tile;   // per scan tile: its sum, then the sum of the tiles before it
  int32_t* long_rows;
  unsigned long long* keys;   // [E]
  float* cnt;                 // [E]
  int64_t E, ntiles, long_cap;
};
static size_t nb_layout(int64_t nnz, int64_t u, int both, char* base, NbWs* ws) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(std::max<size_t>(bytes, 1), 256);
    return p;
  };
  NbWs w;
  nnz = std::max<int64_t>(nnz, 0), u = std::max<int64_t>(u, 0);
  w.E = both ? 2 * nnz : nnz;
  w.ntiles = cdiv(u, kScanTile);
  w.long_cap = w.E / (kNbWaveRow + 1) + 1;
  w.head = (unsigned long long*)take(256);
  w.pos_i = (int32_t*)take(4 * (size_t)nnz);
  w.pos_o = (int32_t*)take(4 * (size_t)nnz);
  w.deg = (uint32_t*)take(4 * (size_t)u);
  w.offsets = (int64_t*)take(8 * (size_t)(u + 1));
  w.tile = (unsigned long long*)take(8 * (size_t)w.ntiles);
  w.long_rows = (int32_t*)take(4 * (size_t)w.long_cap);
  w.keys = (unsigned long long*)take(8 * (size_t)w.E);
  w.cnt = (float*)take(4 * (size_t)w.E);
  if (ws) *ws = w;
  return off;
}

// (key, pay) ascending by key inside every aligned group of S lanes (bitonic network, S a power of two <= 64)
template <int S>
__device__ __forceinline__ void lanes_sort(uint32_t& hi, uint32_t& lo, uint32_t& pay, int lane) {
#pragma unroll
  for (int k = 2; k <= S; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint32_t ohi = xor_lane(hi, j), olo = xor_lane(lo, j), opay = xor_lane(pay, j);
      const bool up = k == S || (lane & k) == 0;  // the last merge leaves every group ascending
      const bool keep_min = ((lane & j) == 0) == up;
      const bool o_less = ohi < hi || (ohi == hi && olo < lo);
      const bool o_more = ohi > hi || (ohi == hi && olo > lo);
      if (keep_min ? o_less : o_more) hi = ohi, lo = olo, pay = opay;
    }
  }
}

// ---- passes -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void nb_pad_kernel(int64_t total, int32_t* __restrict__ out_n, float* __restrict__ out_s,
                                                       float* __restrict__ out_c) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    out_n[i] = -1;
    out_s[i] = 0.f;
    out_c[i] = 0.f;
  }
}

__global__ __launch_bounds__(kBlock) void nb_degree_kernel(const int32_t* __restrict__ index, const int32_t* __restrict__ other,
                                                          int64_t nnz, const int32_t* __restrict__ ids, int64_t u, int both,
                                                          NbWs ws) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kBlock) {
    int32_t pi = find_id(ids, u, index[e]), po = find_id(ids, u, other[e]);
    if (pi < 0 || po < 0) {
      atomicOr(ws.head, kFailMissingId);
      pi = po = -1;  // the entry is left out of both rows
    } else {
      atomicAdd(&ws.deg[pi], 1u);
      if (both) atomicAdd(&ws.deg[po], 1u);
    }
    ws.pos_i[e] = pi;
    ws.pos_o[e] = po;
  }
}

__global__ __launch_bounds__(kBlock) void nb_tile_sums_kernel(int64_t u, NbWs ws) {
  __shared__ unsigned long long s_w[kBlock / kWave];
  for (int64_t t = blockIdx.x; t < ws.ntiles; t += gridDim.x) {
    unsigned long long v = 0;
    const int64_t r0 = t * kScanTile + (int64_t)threadIdx.x * kScanItems;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i)
      if (r0 + i < u) v += ws.deg[r0 + i];
    unsigned long long total;
    block_scan_excl(v, s_w, total);
    if (threadIdx.x == 0) ws.tile[t] = total;
  }
}

__global__ __launch_bounds__(kBlock) void nb_tile_scan_kernel(NbWs ws) {  // one workgroup
  __shared__ unsigned long long s_w[kBlock / kWave];
  unsigned long long carry = 0;
  for (int64_t t0 = 0; t0 < ws.ntiles; t0 += kBlock) {
    const int64_t t = t0 + threadIdx.x;
    const unsigned long long v = t < ws.ntiles ? ws.tile[t] : 0;
    unsigned long long total;
    const unsigned long long excl = block_scan_excl(v, s_w, total);
    if (t < ws.ntiles) ws.tile[t] = carry + excl;
    carry += total;
  }
}

// offsets, lengths = min(k, row length) and the list of the rows above one wave
__global__ __launch_bounds__(kBlock) void nb_offsets_kernel(int64_t u, int k, NbWs ws, int32_t* __restrict__ out_len) {
  __shared__ unsigned long long s_w[kBlock / kWave];
  for (int64_t t = blockIdx.x; t < ws.ntiles; t += gridDim.x) {
    const int64_t r0 = t * kScanTile + (int64_t)threadIdx.x * kScanItems;
    uint32_t d[kScanItems];
    unsigned long long v = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
      d[i] = r0 + i < u ? ws.deg[r0 + i] : 0u;
      v += d[i];
    }
    unsigned long long total;
    unsigned long long at = ws.tile[t] + block_scan_excl(v, s_w, total);
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
      const int64_t r = r0 + i;
      if (r < u) {
        ws.offsets[r] = (int64_t)at;
        out_len[r] = (int32_t)(d[i] < (uint32_t)k ? d[i] : (uint32_t)k);
        if (d[i] > (uint32_t)kNbWaveRow) {
          const unsigned long long pos = atomicAdd(ws.head + 1, 1ull);
          if (pos < (unsigned long long)ws.long_cap) ws.long_rows[pos] = (int32_t)r;
        }
        at += d[i];
        if (r == u - 1) ws.offsets[u] = (int64_t)at;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void nb_fill_kernel(const int32_t* __restrict__ index, const int32_t* __restrict__ other,
                                                        const float* __restrict__ count, int64_t nnz,
                                                        const float* __restrict__ df, int both, int dice, NbWs ws) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kBlock) {
    const int32_t pi = ws.pos_i[e], po = ws.pos_o[e];
    if (pi < 0 || po < 0) continue;
    const float c = count[e];
    const float s = dice ? __fdiv_rn(c, __fadd_rn(df[po], df[pi])) : c;
    // a row's slots from its end down to its start: deg returns to 0, old is in [1, row length]
    const int64_t a = ws.offsets[pi] + (int64_t)atomicSub(&ws.deg[pi], 1u) - 1;
    ws.keys[a] = nb_key(s, other[e]);
    ws.cnt[a] = c;
    if (both) {
      const int64_t b = ws.offsets[po] + (int64_t)atomicSub(&ws.deg[po], 1u) - 1;
      ws.keys[b] = nb_key(s, index[e]);
      ws.cnt[b] = c;
    }
  }
}

// rows of at most 64 entries, four consecutive rows per wave and round
__global__ __launch_bounds__(kBlock) void nb_select_wave_kernel(int64_t u, int k, NbWs ws, int32_t* __restrict__ out_n,
                                                               float* __restrict__ out_s, float* __restrict__ out_c) {
  constexpr int kPack = kWave / kNbPackRow;
  const int lane = threadIdx.x & (kWave - 1), sub = lane / kNbPackRow, l16 = lane & (kNbPackRow - 1);
  const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
  const int64_t nwaves = (int64_t)gridDim.x * (kBlock / kWave);
  const int64_t nquads = (u + kPack - 1) / kPack;
  for (int64_t q = wave; q < nquads; q += nwaves) {  // q is the same in every lane of a wave
    const int64_t r = q * kPack + sub;
    int64_t a = 0;
    int len = 0;  // above 64: any value above 64
    if (r < u) {
      a = ws.offsets[r];
      const int64_t n = ws.offsets[r + 1] - a;
      len = (int)(n < kNbWaveRow + 1 ? n : kNbWaveRow + 1);
    }
    if (__ballot(nb_row_class(len) != 0) == 0) {
      const bool live = l16 < len;
      const unsigned long long key = live ? ws.keys[a + l16] : kPadKey;
      uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key, pay = live ? __float_as_uint(ws.cnt[a + l16]) : 0u;
      lanes_sort<kNbPackRow>(hi, lo, pay, lane);
      if (l16 < len && l16 < k) {
        const int64_t o = r * k + l16;
        out_n[o] = (int32_t)lo;
        out_s[o] = score_of_bits(hi);
        out_c[o] = __uint_as_float(pay);
      }
      continue;
    }
    for (int s = 0; s < kPack; ++s) {  // (every condition is the same in all lanes)
      const int n = __shfl(len, s * kNbPackRow, kWave);
      if (n == 0 || nb_row_class(n) > 1) continue;
      const int64_t rr = q * kPack + s;
      const int64_t aa = ws.offsets[rr];
      const bool live = lane < n;
      const unsigned long long key = live ? ws.keys[aa + lane] : kPadKey;
      uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key, pay = live ? __float_as_uint(ws.cnt[aa + lane]) : 0u;
      lanes_sort<kWave>(hi, lo, pay, lane);
      if (lane < n && lane < k) {
        const int64_t o = rr * k + lane;
        out_n[o] = (int32_t)lo;
        out_s[o] = score_of_bits(hi);
        out_c[o] = __uint_as_float(pay);
      }
    }
  }
}

// rows above 64 entries, one workgroup per listed row
__global__ __launch_bounds__(kBlock) void nb_select_block_kernel(int64_t u, int k, NbWs ws, int32_t* __restrict__ out_n,
                                                                float* __restrict__ out_s, float* __restrict__ out_c) {
  __shared__ unsigned long long s_key[kNbBlockRow];
  __shared__ float s_pay[kNbBlockRow];
  __shared__ unsigned int s_hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned int s_rank, s_n;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const unsigned long long listed = ws.head[1];
  const int64_t nlong = (int64_t)(listed < (unsigned long long)ws.long_cap ? listed : (unsigned long long)ws.long_cap);
  for (int64_t w = blockIdx.x; w < nlong; w += gridDim.x) {  // (w, r, a, len: the same in all threads)
    __syncthreads();  // the previous row's readers are done with the LDS
    const int64_t r = ws.long_rows[w];
    if (r < 0 || r >= u) continue;
    const int64_t a = ws.offsets[r], len = ws.offsets[r + 1] - a;
    if (nb_row_class(len) < 2 || a < 0 || a + len > ws.E) continue;
    const int kk = (int)(len < k ? len : k);
    int n_in;
    if (nb_row_class(len) == 2) {
      n_in = (int)len;
      for (int i = tid; i < n_in; i += kBlock) {
        s_key[i] = ws.keys[a + i];
        s_pay[i] = ws.cnt[a + i];
      }
    } else {
      // the kk-th smallest key, a byte at a time from the top: among the keys that carry the prefix found so far, the
      // digit whose bucket holds rank s_rank (1-based)
      if (tid == 0) s_prefix = 0, s_rank = (unsigned int)kk;
      for (int p = 7; p >= 0; --p) {
        s_hist[tid] = 0;  // kBlock = 256 digits
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        for (int64_t i0 = 0; i0 < len; i0 += kBlock) {  // whole waves stay in the loop: the ballots need them
          const int64_t i = i0 + tid;
          const unsigned long long key = i < len ? ws.keys[a + i] : 0ull;
          const bool match = i < len && (p == 7 || (key >> (8 * (p + 1))) == prefix);
          const int digit = (int)((key >> (8 * p)) & 255u);
          // the top bytes of a row's scores mostly agree: lanes with the leader's digit make one LDS atomic together
          const unsigned long long alive = __ballot(match);
          if (alive) {
            const int leader = __ffsll((long long)alive) - 1;
            const int ld = __shfl(digit, leader, kWave);
            const bool same = match && digit == ld;
            const int cnt = __popcll(__ballot(same));
            if (lane == leader) atomicAdd(&s_hist[ld], (unsigned int)cnt);
            if (match && !same) atomicAdd(&s_hist[digit], 1u);
          }
        }
        __syncthreads();
        if (tid == 0) {
          unsigned int before = 0, rank = s_rank;
          int d = 0;
          for (; d < 255 && before + s_hist[d] < rank; ++d) before += s_hist[d];
          s_rank = rank - before;
          s_prefix = (prefix << 8) | (unsigned int)d;
        }
        __syncthreads();
      }
      const unsigned long long kth = s_prefix;
      if (tid == 0) s_n = 0;
      __syncthreads();
      for (int64_t i = tid; i < len; i += kBlock) {
        const unsigned long long key = ws.keys[a + i];
        if (key <= kth) {  // kk keys when they are distinct; never more than the LDS holds
          const unsigned int pos = atomicAdd(&s_n, 1u);
          if (pos < (unsigned int)kNbBlockRow) {
            s_key[pos] = key;
            s_pay[pos] = ws.cnt[a + i];
          }
        }
      }
      __syncthreads();
      n_in = (int)(s_n < (unsigned int)kNbBlockRow ? s_n : (unsigned int)kNbBlockRow);
    }
    const int m = pow2_at_least(n_in);
    for (int i = n_in + tid; i < m; i += kBlock) {
      s_key[i] = kPadKey;
      s_pay[i] = 0.f;
    }
    lds_sort(s_key, s_pay, m);
    for (int j = tid; j < kk && j < n_in; j += kBlock) {
      const unsigned long long key = s_key[j];
      const int64_t o = r * k + j;
      out_n[o] = (int32_t)(uint32_t)key;
      out_s[o] = score_of_bits((uint32_t)(key >> 32));
      out_c[o] = s_pay[j];
    }
  }
}

// ---- recommend ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void itemknn_recommend_kernel(
    const int32_t* __restrict__ t_ids, const int32_t* __restrict__ t_nb, const float* __restrict__ t_sc,
    const int32_t* __restrict__ t_len, int64_t u, int W, const int32_t* __restrict__ history, int64_t N,
    const int64_t* __restrict__ offsets, int64_t nq, int k, int exclude, int32_t* __restrict__ out_ids,
    float* __restrict__ out_sc, int32_t* __restrict__ out_len) {
  constexpr int kPer = kItemKnnMaxEntries / kBlock;
  __shared__ unsigned long long s_key[kItemKnnMaxEntries];
  __shared__ float s_val[kItemKnnMaxEntries];
  __shared__ int32_t s_hist[kItemKnnMaxEntries];
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {  // (q, a, H, n, m: the same in all threads)
    __syncthreads();  // the previous query's readers are done with the LDS
    const int64_t a = offsets[q], b = offsets[q + 1];
    if (a < 0 || b < a || b > N || (b - a) * W > kItemKnnMaxEntries) {  // refused on the host; never truncated here
      for (int j = tid; j < k; j += kBlock) out_ids[q * k + j] = -1, out_sc[q * k + j] = 0.f;
      if (tid == 0) out_len[q] = -1;
      continue;
    }
    const int H = (int)(b - a), n = H * W, m = pow2_at_least(n);
    if (tid == 0) s_cnt = 0;
    int mh = 2;
    if (exclude) {
      mh = pow2_at_least(H);
      for (int i = tid; i < mh; i += kBlock) s_hist[i] = i < H ? history[a + i] : INT32_MAX;
      lds_sort(s_hist, (int*)nullptr, mh);
    }
    for (int e = tid; e < m; e += kBlock) {
      unsigned long long key = kPadKey;
      float val = 0.f;
      if (e < n) {
        const int p = e / W, j = e - p * W;
        const int32_t row = find_id(t_ids, u, history[a + p]);
        if (row >= 0 && j < t_len[row]) {
          const int32_t cand = t_nb[(int64_t)row * W + j];
          if (cand >= 0) {
            key = ((unsigned long long)(uint32_t)cand << 32) | (uint32_t)e;  // e rises with the history position
            val = t_sc[(int64_t)row * W + j];
          }
        }
      }
      s_key[e] = key;
      s_val[e] = val;
    }
    lds_sort(s_key, s_val, m);
    // the head of every run of one candidate sums the run in key order = history position order
    unsigned long long nk[kPer];
    int kept = 0;
#pragma unroll
    for (int c = 0; c < kPer; ++c) {
      const int i = c * kBlock + tid;
      nk[c] = kPadKey;
      if (i < m) {
        const unsigned long long key = s_key[i];
        const uint32_t cand = (uint32_t)(key >> 32);
        if (key != kPadKey && (i == 0 || (uint32_t)(s_key[i - 1] >> 32) != cand)) {
          float sum = s_val[i];
          for (int j = i + 1; j < m && (uint32_t)(s_key[j] >> 32) == cand; ++j) sum = __fadd_rn(sum, s_val[j]);
          bool drop = false;
          if (exclude) {
            int lo = 0, hi = H;  // (the padding behind the H ids is never looked at)
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (s_hist[mid] < (int32_t)cand) lo = mid + 1; else hi = mid;
            }
            drop = lo < H && s_hist[lo] == (int32_t)cand;
          }
          if (!drop) {
            nk[c] = nb_key(sum, (int32_t)cand);
            ++kept;
          }
        }
      }
    }
    __syncthreads();  // every run is summed: the keys may be overwritten
    if (kept) atomicAdd(&s_cnt, kept);
#pragma unroll
    for (int c = 0; c < kPer; ++c) {
      const int i = c * kBlock + tid;
      if (i < m) s_key[i] = nk[c];
    }
    lds_sort(s_key, (float*)nullptr, m);
    const int kk = s_cnt < k ? s_cnt : k;
    for (int j = tid; j < k; j += kBlock) {
      const unsigned long long key = s_key[j < m ? j : 0];
      const bool live = j < kk;
      out_ids[q * k + j] = live ? (int32_t)(uint32_t)key : -1;
      out_sc[q * k + j] = live ? score_of_bits((uint32_t)(key >> 32)) : 0.f;
    }
    if (tid == 0) out_len[q] = kk;
  }
}

}  // namespace esr

using namespace esr;

extern "C" {

size_t esr_neighbours_workspace_bytes(int64_t nnz, int64_t u, int both) {
  return nb_layout(nnz, u, both != 0, nullptr, nullptr);
}

int esr_neighbours_plan_bounds(int32_t* bounds, int capacity) {
  int32_t b[kNbClasses];
  const int n = nb_plan_bounds(b);
  for (int i = 0; bounds && i < n && i < capacity; ++i) bounds[i] = b[i];
  return n;
}

int esr_neighbours_topk(const int32_t* index, const int32_t* other, const float* count, int64_t nnz, const int32_t* ids,
                        const float* df, int64_t u, int k, int both, int score, int32_t* out_neighbours,
                        float* out_scores, float* out_counts, int32_t* out_lengths, void* workspace,
                        size_t workspace_bytes, esr_stream_t stream) {
  TraceScope trace_scope_("esr_neighbours_topk");
  ESR_REQUIRE(k >= 1 && k <= kSelectMaxK, "esr_neighbours_topk: k=%d not in [1, %d]", k, kSelectMaxK);
  ESR_REQUIRE(nnz >= 0 && nnz < ((int64_t)1 << 30) && u >= 0 && u <= (int64_t)INT32_MAX,
              "esr_neighbours_topk: bad sizes nnz=%lld (at most 2^30 - 1) u=%lld (at most 2^31 - 1)", (long long)nnz,
              (long long)u);
  ESR_REQUIRE((both == 0 || both == 1) && (score == 0 || score == 1),
              "esr_neighbours_topk: orientation=%d (0 stored, 1 both) or score=%d (0 count, 1 dice) unknown", both, score);
  ESR_REQUIRE(nnz == 0 || u > 0, "esr_neighbours_topk: %lld entries but no ids", (long long)nnz);
  ESR_REQUIRE(workspace, "esr_neighbours_topk: null pointer (workspace)");
  if (u == 0) return ESR_OK;
  ESR_REQUIRE(ids && out_neighbours && out_scores && out_counts && out_lengths, "esr_neighbours_topk: null pointer");
  ESR_REQUIRE(nnz == 0 || (index && other && count), "esr_neighbours_topk: null pointer (entries)");
  ESR_REQUIRE(nnz == 0 || score == 0 || df, "esr_neighbours_topk: score dice needs df (null pointer)");
  const size_t need = nb_layout(nnz, u, both, nullptr, nullptr);
  if (workspace_bytes < need || ((uintptr_t)workspace & 15)) {
    set_error("esr_neighbours_topk: workspace %zu bytes < %zu required (or misaligned)", workspace_bytes, need);
    return ESR_EWORKSPACE;
  }
  NbWs ws;
  nb_layout(nnz, u, both, (char*)workspace, &ws);
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(ws.head, 0, 256, st) != hipSuccess || hipMemsetAsync(ws.deg, 0, 4 * (size_t)u, st) != hipSuccess)
    return check_launch("esr_neighbours_topk");
  ESR_KT("nb_pad", st,
         hipLaunchKernelGGL(nb_pad_kernel, dim3(grid_for(u * k)), dim3(kBlock), 0, st, u * k, out_neighbours, out_scores,
                            out_counts));
  if (nnz)
    ESR_KT("nb_degree", st,
           hipLaunchKernelGGL(nb_degree_kernel, dim3(grid_for(nnz)), dim3(kBlock), 0, st, index, other, nnz, ids, u, both,
                              ws));
  const int tile_grid = (int)std::min<int64_t>(kMaxGrid, ws.ntiles);
  ESR_KT("nb_scan", st, {
    hipLaunchKernelGGL(nb_tile_sums_kernel, dim3(tile_grid), dim3(kBlock), 0, st, u, ws);
    hipLaunchKernelGGL(nb_tile_scan_kernel, dim3(1), dim3(kBlock), 0, st, ws);
    hipLaunchKernelGGL(nb_offsets_kernel, dim3(tile_grid), dim3(kBlock), 0, st, u, k, ws, out_lengths);
  });
  if (nnz == 0) return check_launch("esr_neighbours_topk");
  ESR_KT("nb_fill", st,
         hipLaunchKernelGGL(nb_fill_kernel, dim3(grid_for(nnz)), dim3(kBlock), 0, st, index, other, count, nnz, df, both,
                            score, ws));
  const int wave_grid = (int)std::max<int64_t>(1, std::min<int64_t>(kMaxGrid, cdiv(cdiv(u, 4), kBlock / kWave)));
  ESR_KT("nb_select_wave", st,
         hipLaunchKernelGGL(nb_select_wave_kernel, dim3(wave_grid), dim3(kBlock), 0, st, u, k, ws, out_neighbours,
                            out_scores, out_counts));
  // the list's length stays on the device: a grid that covers its bound, workgroups without a row leave at once
  const int block_grid = (int)std::min<int64_t>(kMaxGrid, ws.long_cap);
  ESR_KT("nb_select_block", st,
         hipLaunchKernelGGL(nb_select_block_kernel, dim3(block_grid), dim3(kBlock), 0, st, u, k, ws, out_neighbours,
                            out_scores, out_counts));
  return check_launch("esr_neighbours_topk");
}

int esr_itemknn_max_entries(void) { return kItemKnnMaxEntries; }

int esr_itemknn_recommend(const int32_t* table_ids, const int32_t* table_neighbours, const float* table_scores,
                          const int32_t* table_lengths, int64_t u, int width, const int32_t* history, int64_t N,
                          const int64_t* offsets, int64_t nq, int k, int exclude_history, int32_t* out_ids,
                          float* out_scores, int32_t* out_lengths, esr_stream_t stream) {
  TraceScope trace_scope_("esr_itemknn_recommend");
  ESR_REQUIRE(k >= 1 && k <= kSelectMaxK, "esr_itemknn_recommend: k=%d not in [1, %d]", k, kSelectMaxK);
  ESR_REQUIRE(width >= 1 && width <= kItemKnnMaxWidth, "esr_itemknn_recommend: table width=%d not in [1, %d]", width,
              kItemKnnMaxWidth);
  ESR_REQUIRE(u >= 0 && u <= (int64_t)INT32_MAX && N >= 0 && nq >= 0 && nq <= (int64_t)INT32_MAX,
              "esr_itemknn_recommend: bad sizes u=%lld N=%lld nq=%lld", (long long)u, (long long)N, (long long)nq);
  ESR_REQUIRE(exclude_history == 0 || exclude_history == 1, "esr_itemknn_recommend: exclude_history=%d is not 0 or 1",
              exclude_history);
  if (nq == 0) return ESR_OK;
  ESR_REQUIRE(offsets && out_ids && out_scores && out_lengths, "esr_itemknn_recommend: null pointer");
  ESR_REQUIRE(N == 0 || history, "esr_itemknn_recommend: null pointer (history)");
  ESR_REQUIRE(u == 0 || (table_ids && table_neighbours && table_scores && table_lengths),
              "esr_itemknn_recommend: null pointer (table)");
  hipStream_t st = as_stream(stream);
  ESR_KT("itemknn_recommend", st,
         hipLaunchKernelGGL(itemknn_recommend_kernel, dim3((int)std::min<int64_t>(kMaxGrid, nq)), dim3(kBlock), 0, st,
                            table_ids, table_neighbours, table_scores, table_lengths, u, width, history, N, offsets, nq, k,
                            exclude_history, out_ids, out_scores, out_lengths));
  return check_launch("esr_itemknn_recommend");
}

}  // extern "C"
