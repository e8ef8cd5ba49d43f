// Explicit ratings: the Pearson user-similarity table and the user-kNN affinity over it (the collaborative-filtering job
// of the reference's book, chapter 5 "Data Processing": latest rating per pair -> deviations from the user's mean ->
// self-join on the item, reduce by user pair -> USim; then Aff over the nearest users): esr_usersim_* and esr_userknn_*.
//   input       the ratings as CSR by item: users int32[N] ascending inside an item, dev int32[N] the fixed-point deviation
//               of each rating from its user's mean (the host makes both; the scale cancels in the similarity).
//   pairs       an item with raters u_0 < ... < u_{n-1} adds, for every p < q, to the entry keyed u_p << 32 | u_q:
//               n += 1, P += dev_p dev_q (signed, two's complement), Qa += dev_p^2, Qb += dev_q^2.  Integer sums in the
//               wide pair table of esr_wide_table.h: independent of atomic order and of how the items are cut into calls.
//   work unit   a T x T tile of one item's upper triangle (T = kUsTile = 64 raters): an item with n >= 2 raters has
//               C = ceil(n / T) chunks and C (C + 1) / 2 tiles (chunk_p <= chunk_q; none below two raters), so one popular item spreads over the
//               grid.  The prefix of the tile counts over the items comes from the HOST (it holds the item offsets
//               already, for its launch plan); a wave finds its tile's item in it by binary search.  One wave per tile:
//               lane c holds column rater chunk_q T + c in registers, the wave walks the row raters of chunk_p (a
//               broadcast load each) and lane c emits when its position is above the row's.  Users are distinct inside an
//               item, so the keys of one wave step are distinct: no wave merge.  T = 64 because the kernel is bound by its
//               five 64-bit atomics per pair (one key probe, four adds = 40 B of atomic traffic against 8 B read): one
//               rater per lane needs no LDS and a dozen registers, so every wave slot is filled to hide atomic latency.
//   similarity  finalize compacts the occupied slots, orders them by key with esr_segment_sort_ids (two stable passes, as
//               esr_cooccur_finalize), then sim = float(double(P) / (sqrt(double(Qa)) * sqrt(double(Qb)))) -- fp64, every
//               operation rounded once, no contraction -- filters, and an ordered compaction of the kept rows.
//   predict     one wave per (user, item) query: lane j looks the item up in the row of neighbour j (binary search); the
//               counted columns are accumulated in ascending column order by knn_accumulate.
//   recommend   one workgroup per query user: the rated items of all neighbours gathered into LDS keyed (item, column),
//               sorted, every run of one item accumulated in key order by the SAME knn_accumulate -- recommend's score is
//               predict's, bit for bit -- then dropped / ranked / selected as esr_itemknn_recommend does.
// No kernel waits on another workgroup; every loop is bounded by a size checked on the host, by the table's capacity or by
// a value validated in the kernel before it is used as a bound.
#include "esr_rank_keys.h"
#include "esr_wide_table.h"

namespace esr {

constexpr int kUsTile = kWave;              // T: raters per chunk, one per lane
constexpr int kUserKnnMaxEntries = 2048;    // ratings of all neighbours of one query: what the workgroup sorts
constexpr int kUserKnnMaxWidth = 1024;
constexpr int kUsFlagKeep = 0, kUsFlagDrop = 1;

// ---- table --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void usersim_init_kernel(WideTable t) {
  const int64_t cap = (int64_t)t.mask + 1;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < cap; i += (int64_t)gridDim.x * kBlock) {
    t.keys[i] = kEmptyKey;
#pragma unroll
    for (int s = 0; s < kWideSums; ++s) t.sums[s * cap + i] = 0ull;
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) t.used[threadIdx.x] = 0ull;  // used, fail
}

__global__ __launch_bounds__(kBlock) void usersim_rehash_kernel(WideTable src, WideTable dst) {
  const int64_t cap = (int64_t)src.mask + 1;
  carry_fail(header_of(src), header_of(dst));
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < cap; i += (int64_t)gridDim.x * kBlock) {
    const unsigned long long k = src.keys[i];
    if (k != kEmptyKey) wide_add(dst, k, src.sums[i], src.sums[cap + i], src.sums[2 * cap + i], src.sums[3 * cap + i]);
  }
}

// ---- accumulate ---------------------------------------------------------------------------------------------------------
// tile x of an item's triangle, column by column: x = cq (cq + 1) / 2 + cp with cp <= cq.  x < 2^49: 8 x + 1 is exact in a
// double; the two corrections are a safety net.
__device__ __forceinline__ void tile_decode(int64_t x, int64_t& cp, int64_t& cq) {
  int64_t c = (int64_t)((sqrt(8.0 * (double)x + 1.0) - 1.0) * 0.5);
  if (c * (c + 1) / 2 > x) --c;
  if ((c + 1) * (c + 2) / 2 <= x) ++c;
  cq = c;
  cp = x - c * (c + 1) / 2;
}

__global__ __launch_bounds__(kBlock) void usersim_accumulate_kernel(
    const int32_t* __restrict__ users, const int32_t* __restrict__ dev, int64_t N, const int64_t* __restrict__ item_offsets,
    const int32_t* __restrict__ item_ids, const int64_t* __restrict__ tile_prefix, int64_t item_begin, int64_t item_end,
    int64_t ntiles, WideTable t) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
  const int64_t nwaves = (int64_t)gridDim.x * (kBlock / kWave);
  const int64_t first = tile_prefix[item_begin];
  if (tile_prefix[item_end] - first != ntiles) {  // the device's prefix is not the host's plan: nothing is walked
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(t.fail, kFailBadOffsets);
    return;
  }
  for (int64_t x = wave; x < ntiles; x += nwaves) {  // (x and everything up to the column load: the same in all lanes)
    const int64_t it = doc_of(tile_prefix, item_begin + 1, item_end, first + x) - 1;
    const int64_t a = item_offsets[it], b = item_offsets[it + 1];
    const int64_t n = b - a, C = n < 2 ? 0 : (n + kUsTile - 1) / kUsTile;  // fewer than two raters: no pair, no tile
    const int64_t local = first + x - tile_prefix[it];
    if (a < 0 || b > N || a > b || local < 0 || local >= C * (C + 1) / 2) {
      if (lane == 0) atomicOr(t.fail, kFailBadOffsets);
      continue;
    }
    if (item_ids[it] < 0) {
      if (lane == 0) atomicOr(t.fail, kFailNegativeId);
      continue;
    }
    int64_t cp, cq;
    tile_decode(local, cp, cq);
    const int64_t q = cq * kUsTile + lane, p0 = cp * kUsTile;
    bool live = q < n;
    int32_t uq = 0, dq = 0;
    if (live) {
      uq = users[a + q];
      dq = dev[a + q];
      if (uq < 0) {
        atomicOr(t.fail, kFailNegativeId);
        live = false;
      }
    }
    const int rows = (int)(n - p0 < kUsTile ? n - p0 : kUsTile);
    for (int r = 0; r < rows; ++r) {
      const int64_t p = p0 + r;
      const int32_t up = users[a + p], dp = dev[a + p];
      if (up < 0) {
        if (lane == 0) atomicOr(t.fail, kFailNegativeId);
        continue;
      }
      if (!live || q <= p) continue;
      if (uq <= up) {  // a (user, item) given twice shows as adjacent equal users; any other disorder as a descent
        atomicOr(t.fail, kFailNotAscending);
        continue;
      }
      wide_add(t, ((unsigned long long)(uint32_t)up << 32) | (uint32_t)uq, 1ull,
               (unsigned long long)((long long)dp * (long long)dq), (unsigned long long)((long long)dp * (long long)dp),
               (unsigned long long)((long long)dq * (long long)dq));
    }
  }
}

// ---- finalize -----------------------------------------------------------------------------------------------------------
struct UsFinalizeWs {
  unsigned long long* counter;  // word 0: compaction rows, word 1: flat entries
  unsigned long long* tile;     // kept rows per tile of kBlock sorted rows, then their exclusive sums
  int32_t *index, *other, *slot, *sorted_other, *perm1, *index1, *sorted_index, *perm2, *overlap;
  float* sim;
  uint8_t* flag;
  void* sort_ws;
  size_t sort_ws_bytes;
  int64_t ntiles;
};
static size_t us_finalize_layout(int64_t nnz, char* base, UsFinalizeWs* ws) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return p;
  };
  UsFinalizeWs w;
  const size_t n = (size_t)std::max<int64_t>(nnz, 1);
  w.ntiles = cdiv((int64_t)n, kBlock);
  w.counter = (unsigned long long*)take(256);
  w.tile = (unsigned long long*)take(8 * (size_t)w.ntiles);
  w.index = (int32_t*)take(4 * n);
  w.other = (int32_t*)take(4 * n);
  w.slot = (int32_t*)take(4 * n);
  w.sorted_other = (int32_t*)take(4 * n);
  w.perm1 = (int32_t*)take(4 * n);
  w.index1 = (int32_t*)take(4 * n);
  w.sorted_index = (int32_t*)take(4 * n);
  w.perm2 = (int32_t*)take(4 * n);
  w.overlap = (int32_t*)take(4 * n);
  w.sim = (float*)take(4 * n);
  w.flag = (uint8_t*)take(n);
  w.sort_ws_bytes = esr_segment_sort_workspace_bytes(nnz);
  w.sort_ws = take(w.sort_ws_bytes);
  if (ws) *ws = w;
  return off;
}

__global__ __launch_bounds__(kBlock) void usersim_compact_kernel(WideTable t, int64_t nnz, UsFinalizeWs ws) {
  const int64_t cap = (int64_t)t.mask + 1;
  const CooccurTable head = header_of(t);
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < cap; i += (int64_t)gridDim.x * kBlock) {
    const unsigned long long k = t.keys[i];
    if (k == kEmptyKey) continue;
    unsigned long long pos;
    if (!compact_claim(head, ws.counter, nnz, pos)) continue;
    ws.index[pos] = (int32_t)(k >> 32);
    ws.other[pos] = (int32_t)(uint32_t)k;
    ws.slot[pos] = (int32_t)i;
  }
}

__global__ __launch_bounds__(kBlock) void usersim_gather_kernel(const int32_t* __restrict__ src,
                                                               const int32_t* __restrict__ perm, int64_t n,
                                                               int32_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    out[i] = src[perm[i]];
}

// sorted row i = compacted entry perm1[perm2[i]]: its similarity, overlap and fate; kept rows counted per tile
__global__ __launch_bounds__(kBlock) void usersim_score_kernel(WideTable t, int64_t nnz, int min_overlap, int has_min,
                                                              float min_similarity, UsFinalizeWs ws) {
#pragma clang fp contract(off)  // every fp64 operation rounds once, as the NumPy restatement's do
  __shared__ unsigned long long s_w[kBlock / kWave];
  const int64_t cap = (int64_t)t.mask + 1;
  for (int64_t tile = blockIdx.x; tile < ws.ntiles; tile += gridDim.x) {
    const int64_t i = tile * kBlock + threadIdx.x;
    unsigned long long keep = 0;
    if (i < nnz) {
      const int32_t c = ws.perm1[ws.perm2[i]];
      const int64_t slot = ws.slot[c];
      const unsigned long long n = t.sums[slot], P = t.sums[cap + slot], Qa = t.sums[2 * cap + slot],
                               Qb = t.sums[3 * cap + slot];
      const bool flat = Qa == 0 || Qb == 0;
      float sim = 0.f;
      if (flat) atomicAdd(ws.counter + 1, 1ull);
      else sim = (float)((double)(long long)P / (sqrt((double)Qa) * sqrt((double)Qb)));
      const bool drop = flat || n < (unsigned long long)min_overlap || (has_min && sim <= min_similarity);
      ws.sim[i] = sim;
      ws.overlap[i] = (int32_t)n;
      ws.flag[i] = drop ? kUsFlagDrop : kUsFlagKeep;
      keep = drop ? 0 : 1;
    }
    unsigned long long total;
    block_scan_excl(keep, s_w, total);
    if (threadIdx.x == 0) ws.tile[tile] = total;
  }
}

__global__ __launch_bounds__(kBlock) void usersim_tile_scan_kernel(UsFinalizeWs ws, int64_t* __restrict__ counts) {  // one workgroup
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
  if (threadIdx.x == 0) {
    counts[0] = (int64_t)carry;
    counts[1] = (int64_t)ws.counter[1];
  }
}

__global__ __launch_bounds__(kBlock) void usersim_emit_kernel(int64_t nnz, UsFinalizeWs ws, int32_t* __restrict__ index,
                                                             int32_t* __restrict__ other, float* __restrict__ sim,
                                                             int32_t* __restrict__ overlap) {
  __shared__ unsigned long long s_w[kBlock / kWave];
  for (int64_t tile = blockIdx.x; tile < ws.ntiles; tile += gridDim.x) {
    const int64_t i = tile * kBlock + threadIdx.x;
    const bool keep = i < nnz && ws.flag[i] == kUsFlagKeep;
    unsigned long long total;
    const unsigned long long o = ws.tile[tile] + block_scan_excl(keep ? 1ull : 0ull, s_w, total);
    if (keep && o < (unsigned long long)nnz) {  // (kept rows never outnumber the rows)
      index[o] = ws.sorted_index[i];
      other[o] = ws.sorted_other[ws.perm2[i]];
      sim[o] = ws.sim[i];
      overlap[o] = ws.overlap[i];
    }
  }
}

// ---- user-kNN -----------------------------------------------------------------------------------------------------------
struct UserKnn {
  const int32_t *t_ids, *t_nb;   // the neighbour table: ids [u], neighbours [u, W]
  const float* t_sc;             // similarities [u, W]
  const int32_t* t_len;          // [u]
  int64_t u;
  int W;
  const int32_t* users;          // [nu] ascending: the rows of the ratings CSR
  int64_t nu;
  const int64_t* row_off;        // [nu + 1]
  const int32_t* items;          // [R] ascending inside a row
  const float* ratings;          // [R]
  int64_t R;
  const double* mean;            // [nu]
  int center_neighbour, den_all;
};
struct KnnAcc {
  double num, den;
  int support;
};
// THE accumulation of both kernels: one counted column -- similarity s, the neighbour's rating r of the item, centre c
__device__ __forceinline__ void knn_accumulate(KnnAcc& a, double s, double r, double c, int den_all) {
#pragma clang fp contract(off)  // the product and the sum round separately
  a.num = a.num + s * (r - c);
  if (!den_all) a.den = a.den + fabs(s);
  a.support += 1;
}
// denominator "all": the similarities of the whole row, in column order
__device__ __forceinline__ double knn_den_all(const float* __restrict__ sc, int len) {
  double den = 0.0;
  for (int j = 0; j < len; ++j) den = den + (double)sc[j];
  return den;
}
__device__ __forceinline__ float knn_affinity(double mean_a, const KnnAcc& a) {
#pragma clang fp contract(off)
  const float f = (float)((a.support == 0 || a.den == 0.0) ? mean_a : mean_a + a.num / a.den);
  return f == 0.f ? 0.f : f;  // -0 counts as +0, as in the order key
}
// the ratings row [a, b) of users[pu], empty when the offsets cannot be used
__device__ __forceinline__ void knn_row(const UserKnn& m, int32_t pu, int64_t& a, int64_t& b) {
  a = b = 0;
  if (pu < 0) return;
  const int64_t x = m.row_off[pu], y = m.row_off[pu + 1];
  if (x >= 0 && x <= y && y <= m.R) a = x, b = y;
}
// the position of item x in items[a, b) (ascending), or -1
__device__ __forceinline__ int64_t knn_find_item(const int32_t* __restrict__ items, int64_t a, int64_t b, int32_t x) {
  int64_t lo = a, hi = b;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (items[mid] < x) lo = mid + 1; else hi = mid;
  }
  return (lo < b && items[lo] == x) ? lo : -1;
}

__global__ __launch_bounds__(kBlock) void userknn_predict_kernel(UserKnn m, const int32_t* __restrict__ q_users,
                                                                const int32_t* __restrict__ q_items, int64_t nq,
                                                                float* __restrict__ out_aff,
                                                                int32_t* __restrict__ out_support) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave;
  const int64_t nwaves = (int64_t)gridDim.x * (kBlock / kWave);
  for (int64_t q = wave; q < nq; q += nwaves) {  // (q, row, pa, len: the same in every lane of a wave)
    const int32_t A = q_users[q], it = q_items[q];
    const int32_t row = find_id(m.t_ids, m.u, A), pa = find_id(m.users, m.nu, A);
    if (row < 0 || pa < 0) {
      if (lane == 0) out_aff[q] = __uint_as_float(0x7FC00000u), out_support[q] = 0;
      continue;
    }
    int len = m.t_len[row];
    len = len < 0 ? 0 : (len > m.W ? m.W : len);
    const double mean_a = m.mean[pa];
    const float* sc = m.t_sc + (int64_t)row * m.W;
    KnnAcc acc{0.0, m.den_all ? knn_den_all(sc, len) : 0.0, 0};
    for (int j0 = 0; j0 < len; j0 += kWave) {  // whole waves stay in the loop: the ballot needs them
      const int j = j0 + lane;
      bool found = false;
      double s = 0.0, r = 0.0, c = 0.0;
      if (j < len) {
        const int32_t U = m.t_nb[(int64_t)row * m.W + j];
        const int32_t pu = U >= 0 ? find_id(m.users, m.nu, U) : -1;
        int64_t a, b;
        knn_row(m, pu, a, b);
        const int64_t pos = knn_find_item(m.items, a, b, it);
        if (pos >= 0) {
          found = true;
          s = (double)sc[j];
          r = (double)m.ratings[pos];
          c = m.center_neighbour ? m.mean[pu] : mean_a;
        }
      }
      for (unsigned long long mask = __ballot(found); mask; mask &= mask - 1) {  // ascending column order
        const int l = __ffsll((long long)mask) - 1;
        knn_accumulate(acc, __shfl(s, l, kWave), __shfl(r, l, kWave), __shfl(c, l, kWave), m.den_all);
      }
    }
    if (lane == 0) out_aff[q] = knn_affinity(mean_a, acc), out_support[q] = acc.support;
  }
}

__global__ __launch_bounds__(kBlock) void userknn_recommend_kernel(UserKnn m, const int32_t* __restrict__ q_users,
                                                                  int64_t nq, int k, int exclude, int min_support,
                                                                  int32_t* __restrict__ out_ids,
                                                                  float* __restrict__ out_sc,
                                                                  int32_t* __restrict__ out_len) {
  constexpr int kPer = kUserKnnMaxEntries / kBlock;
  __shared__ unsigned long long s_key[kUserKnnMaxEntries];
  __shared__ float s_val[kUserKnnMaxEntries];
  __shared__ int32_t s_pu[kUserKnnMaxWidth];
  __shared__ int32_t s_start[kUserKnnMaxWidth + 1];
  __shared__ double s_den;
  __shared__ int s_cnt;
  const int tid = threadIdx.x;
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {  // (q, row, pa, len, n, m2: the same in all threads)
    __syncthreads();  // the previous query's readers are done with the LDS
    const int32_t A = q_users[q];
    const int32_t row = find_id(m.t_ids, m.u, A), pa = find_id(m.users, m.nu, A);
    int len = row >= 0 ? m.t_len[row] : 0;
    len = len < 0 ? 0 : (len > m.W ? m.W : len);
    const float* sc = m.t_sc + (int64_t)(row < 0 ? 0 : row) * m.W;
    for (int j = tid; j < len; j += kBlock) {
      const int32_t U = m.t_nb[(int64_t)row * m.W + j];
      const int32_t pu = U >= 0 ? find_id(m.users, m.nu, U) : -1;
      int64_t a, b;
      knn_row(m, pu, a, b);
      s_pu[j] = pu;
      s_start[j + 1] = (int32_t)(b - a < kUserKnnMaxEntries + 1 ? b - a : kUserKnnMaxEntries + 1);
    }
    __syncthreads();
    if (tid == 0) {
      int at = 0;
      s_start[0] = 0;
      for (int j = 0; j < len; ++j) {  // len <= 1024; clamped: a query above the cap is refused below
        at += s_start[j + 1];
        at = at < kUserKnnMaxEntries + 1 ? at : kUserKnnMaxEntries + 1;
        s_start[j + 1] = at;
      }
      s_den = m.den_all ? knn_den_all(sc, len) : 0.0;
      s_cnt = 0;
    }
    __syncthreads();
    const int n = s_start[len];
    if (row < 0 || pa < 0 || n > kUserKnnMaxEntries) {  // a user the table lacks: an empty list; above the cap: refused
      for (int j = tid; j < k; j += kBlock) out_ids[q * k + j] = -1, out_sc[q * k + j] = 0.f;
      if (tid == 0) out_len[q] = (row < 0 || pa < 0) ? 0 : -1;
      continue;
    }
    const int m2 = pow2_at_least(n);
    const double mean_a = m.mean[pa];
    int64_t own_a, own_b;
    knn_row(m, pa, own_a, own_b);
    for (int e = tid; e < m2; e += kBlock) {
      unsigned long long key = kPadKey;
      float val = 0.f;
      if (e < n) {
        int lo = 0, hi = len;  // the column j with s_start[j] <= e < s_start[j + 1]
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_start[mid + 1] <= e) lo = mid + 1; else hi = mid;
        }
        const int j = lo;
        const int64_t pos = m.row_off[s_pu[j]] + (e - s_start[j]);  // inside the row knn_row accepted
        const int32_t item = m.items[pos];
        if (item >= 0) {
          key = ((unsigned long long)(uint32_t)item << 32) | (uint32_t)j;  // an item occurs once per row: keys distinct
          val = m.ratings[pos];
        }
      }
      s_key[e] = key;
      s_val[e] = val;
    }
    lds_sort(s_key, s_val, m2);
    // the head of every run of one item accumulates the run in key order = column order
    unsigned long long nk[kPer];
    int kept = 0;
#pragma unroll
    for (int c = 0; c < kPer; ++c) {
      const int i = c * kBlock + tid;
      nk[c] = kPadKey;
      if (i < m2) {
        const unsigned long long key = s_key[i];
        const uint32_t cand = (uint32_t)(key >> 32);
        if (key != kPadKey && (i == 0 || (uint32_t)(s_key[i - 1] >> 32) != cand)) {
          KnnAcc acc{0.0, s_den, 0};
          for (int x = i; x < m2 && s_key[x] != kPadKey && (uint32_t)(s_key[x] >> 32) == cand; ++x) {
            const int j = (int)(uint32_t)s_key[x];
            knn_accumulate(acc, (double)sc[j], (double)s_val[x], m.center_neighbour ? m.mean[s_pu[j]] : mean_a,
                           m.den_all);
          }
          bool drop = acc.support < min_support;
          if (!drop && exclude) drop = knn_find_item(m.items, own_a, own_b, (int32_t)cand) >= 0;
          if (!drop) {
            nk[c] = nb_key(knn_affinity(mean_a, acc), (int32_t)cand);
            ++kept;
          }
        }
      }
    }
    __syncthreads();  // every run is accumulated: the keys may be overwritten
    if (kept) atomicAdd(&s_cnt, kept);
#pragma unroll
    for (int c = 0; c < kPer; ++c) {
      const int i = c * kBlock + tid;
      if (i < m2) s_key[i] = nk[c];
    }
    lds_sort(s_key, (float*)nullptr, m2);
    const int kk = s_cnt < k ? s_cnt : k;
    for (int j = tid; j < k; j += kBlock) {
      const unsigned long long key = s_key[j < m2 ? j : 0];
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

int esr_usersim_tile(void) { return kUsTile; }

size_t esr_usersim_table_bytes(int64_t capacity) { return wide_table_bytes(capacity); }

int esr_usersim_table_init(void* table, int64_t capacity, esr_stream_t stream) {
  ESR_REQUIRE_TABLE("esr_usersim_table_init", "capacity", capacity);
  ESR_REQUIRE(table && ((uintptr_t)table & 15) == 0, "esr_usersim_table_init: null (or misaligned) table");
  hipStream_t st = as_stream(stream);
  ESR_KT("usersim_init", st,
         hipLaunchKernelGGL(usersim_init_kernel, dim3(grid_for(capacity)), dim3(kBlock), 0, st,
                            wide_view(table, capacity)));
  return check_launch("esr_usersim_table_init");
}

int esr_usersim_rehash(const void* table, int64_t capacity, void* new_table, int64_t new_capacity,
                       esr_stream_t stream) {
  TraceScope trace_scope_("esr_usersim_rehash");
  ESR_REQUIRE(table_capacity_ok(capacity) && table_capacity_ok(new_capacity) && new_capacity >= capacity,
              "esr_usersim_rehash: capacities %lld -> %lld must be powers of two >= 2 that do not shrink",
              (long long)capacity, (long long)new_capacity);
  ESR_REQUIRE(table && new_table && table != new_table && ((uintptr_t)new_table & 15) == 0,
              "esr_usersim_rehash: null, misaligned or aliased table");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(usersim_init_kernel, dim3(grid_for(new_capacity)), dim3(kBlock), 0, st,
                     wide_view(new_table, new_capacity));
  ESR_KT("usersim_rehash", st,
         hipLaunchKernelGGL(usersim_rehash_kernel, dim3(grid_for(capacity)), dim3(kBlock), 0, st,
                            wide_view(const_cast<void*>(table), capacity), wide_view(new_table, new_capacity)));
  return check_launch("esr_usersim_rehash");
}

int esr_usersim_accumulate(const int32_t* users, const int32_t* dev, int64_t N, const int64_t* item_offsets,
                           const int32_t* item_ids, const int64_t* tile_prefix, int64_t nitems, int64_t item_begin,
                           int64_t item_end, int64_t ntiles, void* table, int64_t capacity, esr_stream_t stream) {
  TraceScope trace_scope_("esr_usersim_accumulate");
  ESR_REQUIRE_TABLE("esr_usersim_accumulate", "capacity", capacity);
  ESR_REQUIRE(N >= 0 && nitems >= 0 && ntiles >= 0, "esr_usersim_accumulate: negative size N=%lld nitems=%lld ntiles=%lld",
              (long long)N, (long long)nitems, (long long)ntiles);
  ESR_REQUIRE(0 <= item_begin && item_begin <= item_end && item_end <= nitems,
              "esr_usersim_accumulate: item range [%lld, %lld) not inside [0, nitems=%lld)", (long long)item_begin,
              (long long)item_end, (long long)nitems);
  ESR_REQUIRE(table && item_offsets && tile_prefix, "esr_usersim_accumulate: null pointer");
  if (item_begin == item_end || N == 0 || ntiles == 0) return ESR_OK;
  ESR_REQUIRE(users && dev && item_ids, "esr_usersim_accumulate: null pointer (ratings)");
  hipStream_t st = as_stream(stream);
  const int grid = (int)std::min<int64_t>(kMaxGrid, cdiv(ntiles, kBlock / kWave));
  ESR_KT("usersim_accumulate", st,
         hipLaunchKernelGGL(usersim_accumulate_kernel, dim3(grid), dim3(kBlock), 0, st, users, dev, N, item_offsets,
                            item_ids, tile_prefix, item_begin, item_end, ntiles, wide_view(table, capacity)));
  return check_launch("esr_usersim_accumulate");
}

size_t esr_usersim_finalize_workspace_bytes(int64_t nnz) { return us_finalize_layout(nnz, nullptr, nullptr); }

int esr_usersim_finalize(void* table, int64_t capacity, int64_t nnz, int64_t num_ids, int min_overlap,
                         int has_min_similarity, float min_similarity, int32_t* index, int32_t* other, float* sim,
                         int32_t* overlap, int64_t* counts, void* workspace, size_t workspace_bytes,
                         esr_stream_t stream) {
  TraceScope trace_scope_("esr_usersim_finalize");
  ESR_REQUIRE_TABLE("esr_usersim_finalize", "capacity", capacity);
  ESR_REQUIRE(capacity <= ((int64_t)1 << 31), "esr_usersim_finalize: capacity=%lld above 2^31 slots", (long long)capacity);
  ESR_REQUIRE(nnz >= 0 && nnz <= capacity && nnz < ((int64_t)1 << 30) && num_ids > 0 &&
                  num_ids <= ((int64_t)1 << 31),
              "esr_usersim_finalize: bad sizes nnz=%lld (capacity %lld) num_ids=%lld", (long long)nnz,
              (long long)capacity, (long long)num_ids);
  ESR_REQUIRE(min_overlap >= 1, "esr_usersim_finalize: min_overlap=%d below 1", min_overlap);
  ESR_REQUIRE((has_min_similarity == 0 || has_min_similarity == 1) && !(min_similarity != min_similarity),
              "esr_usersim_finalize: has_min_similarity=%d is not 0 or 1 (or min_similarity is NaN)", has_min_similarity);
  ESR_REQUIRE(table && counts, "esr_usersim_finalize: null pointer");
  hipStream_t st = as_stream(stream);
  if (nnz == 0) {
    if (hipMemsetAsync(counts, 0, 16, st) != hipSuccess) return check_launch("esr_usersim_finalize");
    return ESR_OK;
  }
  ESR_REQUIRE(index && other && sim && overlap && workspace, "esr_usersim_finalize: null pointer (outputs)");
  if (workspace_bytes < us_finalize_layout(nnz, nullptr, nullptr) || ((uintptr_t)workspace & 15)) {
    set_error("esr_usersim_finalize: workspace %zu bytes < %zu required (or misaligned)", workspace_bytes,
              us_finalize_layout(nnz, nullptr, nullptr));
    return ESR_EWORKSPACE;
  }
  UsFinalizeWs ws;
  us_finalize_layout(nnz, (char*)workspace, &ws);
  // (index, other and slot are zeroed: with an nnz above the table's occupied count the rows past it stay valid to sort
  // and to read)
  if (hipMemsetAsync(ws.counter, 0, 256, st) != hipSuccess || hipMemsetAsync(ws.index, 0, 4 * (size_t)nnz, st) != hipSuccess ||
      hipMemsetAsync(ws.other, 0, 4 * (size_t)nnz, st) != hipSuccess || hipMemsetAsync(ws.slot, 0, 4 * (size_t)nnz, st) != hipSuccess)
    return check_launch("esr_usersim_finalize");
  const WideTable t = wide_view(table, capacity);
  const int g = grid_for(nnz);
  ESR_KT("usersim_compact", st,
         hipLaunchKernelGGL(usersim_compact_kernel, dim3(grid_for(capacity)), dim3(kBlock), 0, st, t, nnz, ws));
  // ascending (index, other): stable by `other`, then stable by `index` of that order
  if (int rc = esr_segment_sort_ids(ws.other, nnz, num_ids, ws.sorted_other, ws.perm1, ws.sort_ws, ws.sort_ws_bytes,
                                    stream))
    return rc;
  hipLaunchKernelGGL(usersim_gather_kernel, dim3(g), dim3(kBlock), 0, st, (const int32_t*)ws.index,
                     (const int32_t*)ws.perm1, nnz, ws.index1);
  if (int rc = esr_segment_sort_ids(ws.index1, nnz, num_ids, ws.sorted_index, ws.perm2, ws.sort_ws, ws.sort_ws_bytes,
                                    stream))
    return rc;
  const int tile_grid = (int)std::min<int64_t>(kMaxGrid, ws.ntiles);
  ESR_KT("usersim_score", st,
         hipLaunchKernelGGL(usersim_score_kernel, dim3(tile_grid), dim3(kBlock), 0, st, t, nnz, min_overlap,
                            has_min_similarity, min_similarity, ws));
  hipLaunchKernelGGL(usersim_tile_scan_kernel, dim3(1), dim3(kBlock), 0, st, ws, counts);
  ESR_KT("usersim_emit", st,
         hipLaunchKernelGGL(usersim_emit_kernel, dim3(tile_grid), dim3(kBlock), 0, st, nnz, ws, index, other, sim,
                            overlap));
  return check_launch("esr_usersim_finalize");
}

int esr_userknn_max_entries(void) { return kUserKnnMaxEntries; }

// the argument checks that predict and recommend share; `fn` is a string literal
#define ESR_REQUIRE_USERKNN(fn)                                                                                           \
  do {                                                                                                                    \
    ESR_REQUIRE(width >= 1 && width <= kUserKnnMaxWidth, fn ": table width=%d not in [1, %d]", width, kUserKnnMaxWidth);  \
    ESR_REQUIRE(u >= 0 && u <= (int64_t)INT32_MAX && nu >= 0 && nu <= (int64_t)INT32_MAX && R >= 0 &&                     \
                    R <= (int64_t)INT32_MAX && nq >= 0 && nq <= (int64_t)INT32_MAX,                                       \
                fn ": bad sizes u=%lld nu=%lld R=%lld nq=%lld", (long long)u, (long long)nu, (long long)R, (long long)nq); \
    ESR_REQUIRE((center == 0 || center == 1) && (denominator == 0 || denominator == 1),                                   \
                fn ": center=%d (0 query, 1 neighbour) or denominator=%d (0 rated, 1 all) unknown", center, denominator); \
  } while (0)

static UserKnn userknn_view(const int32_t* table_ids, const int32_t* table_neighbours, const float* table_scores,
                            const int32_t* table_lengths, int64_t u, int width, const int32_t* users, int64_t nu,
                            const int64_t* row_offsets, const int32_t* items, const float* ratings, int64_t R,
                            const double* mean, int center, int denominator) {
  UserKnn m;
  m.t_ids = table_ids, m.t_nb = table_neighbours, m.t_sc = table_scores, m.t_len = table_lengths, m.u = u, m.W = width;
  m.users = users, m.nu = nu, m.row_off = row_offsets, m.items = items, m.ratings = ratings, m.R = R, m.mean = mean;
  m.center_neighbour = center, m.den_all = denominator;
  return m;
}

int esr_userknn_predict(const int32_t* table_ids, const int32_t* table_neighbours, const float* table_scores,
                        const int32_t* table_lengths, int64_t u, int width, const int32_t* users, int64_t nu,
                        const int64_t* row_offsets, const int32_t* items, const float* ratings, int64_t R,
                        const double* mean, const int32_t* query_users, const int32_t* query_items, int64_t nq,
                        int center, int denominator, float* out_affinity, int32_t* out_support, esr_stream_t stream) {
  TraceScope trace_scope_("esr_userknn_predict");
  ESR_REQUIRE_USERKNN("esr_userknn_predict");
  if (nq == 0) return ESR_OK;
  ESR_REQUIRE(query_users && query_items && out_affinity && out_support, "esr_userknn_predict: null pointer");
  ESR_REQUIRE(u == 0 || (table_ids && table_neighbours && table_scores && table_lengths),
              "esr_userknn_predict: null pointer (table)");
  ESR_REQUIRE(row_offsets && (nu == 0 || (users && mean)) && (R == 0 || (items && ratings)),
              "esr_userknn_predict: null pointer (ratings)");
  hipStream_t st = as_stream(stream);
  const int grid = (int)std::min<int64_t>(kMaxGrid, cdiv(nq, kBlock / kWave));
  ESR_KT("userknn_predict", st,
         hipLaunchKernelGGL(userknn_predict_kernel, dim3(grid), dim3(kBlock), 0, st,
                            userknn_view(table_ids, table_neighbours, table_scores, table_lengths, u, width, users, nu,
                                         row_offsets, items, ratings, R, mean, center, denominator),
                            query_users, query_items, nq, out_affinity, out_support));
  return check_launch("esr_userknn_predict");
}

int esr_userknn_recommend(const int32_t* table_ids, const int32_t* table_neighbours, const float* table_scores,
                          const int32_t* table_lengths, int64_t u, int width, const int32_t* users, int64_t nu,
                          const int64_t* row_offsets, const int32_t* items, const float* ratings, int64_t R,
                          const double* mean, const int32_t* query_users, int64_t nq, int k, int exclude_rated,
                          int min_support, int center, int denominator, int32_t* out_ids, float* out_scores,
                          int32_t* out_lengths, esr_stream_t stream) {
  TraceScope trace_scope_("esr_userknn_recommend");
  ESR_REQUIRE(k >= 1 && k <= kSelectMaxK, "esr_userknn_recommend: k=%d not in [1, %d]", k, kSelectMaxK);
  ESR_REQUIRE_USERKNN("esr_userknn_recommend");
  ESR_REQUIRE((exclude_rated == 0 || exclude_rated == 1) && min_support >= 0,
              "esr_userknn_recommend: exclude_rated=%d is not 0 or 1 (or min_support=%d is negative)", exclude_rated,
              min_support);
  if (nq == 0) return ESR_OK;
  ESR_REQUIRE(query_users && out_ids && out_scores && out_lengths, "esr_userknn_recommend: null pointer");
  ESR_REQUIRE(u == 0 || (table_ids && table_neighbours && table_scores && table_lengths),
              "esr_userknn_recommend: null pointer (table)");
  ESR_REQUIRE(row_offsets && (nu == 0 || (users && mean)) && (R == 0 || (items && ratings)),
              "esr_userknn_recommend: null pointer (ratings)");
  hipStream_t st = as_stream(stream);
  ESR_KT("userknn_recommend", st,
         hipLaunchKernelGGL(userknn_recommend_kernel, dim3((int)std::min<int64_t>(kMaxGrid, nq)), dim3(kBlock), 0, st,
                            userknn_view(table_ids, table_neighbours, table_scores, table_lengths, u, width, users, nu,
                                         row_offsets, items, ratings, R, mean, center, denominator),
                            query_users, nq, k, exclude_rated, min_support, out_ids, out_scores, out_lengths));
  return check_launch("esr_userknn_recommend");
}

}  // extern "C"
