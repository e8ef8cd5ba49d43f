// What the kNN recommenders share (esr_neighbours.hip: item-kNN; esr_ratings.hip: user-kNN): the order key of a scored id,
// the lookup of an id in an ascending list, the workgroup's bitonic sort in LDS and its exclusive scan.
//   order       score descending, then id ascending: ONE uint64 per entry, (inverted order-preserving score bits) << 32 | id,
//               ascending.  The score key is total over signed floats; -0 counts as +0.
#pragma once
#include "esr_common.h"

namespace esr {

constexpr unsigned long long kPadKey = ~0ull;  // sorts behind every entry (no id is -1)

#ifdef __HIPCC__
// f32 -> uint32 whose ASCENDING order is the score's DESCENDING order (-0 counts as +0), and back
__device__ __forceinline__ uint32_t score_desc_bits(float s) {
  uint32_t b = __float_as_uint(s);
  if ((b << 1) == 0) b = 0;
  return ~((b & 0x80000000u) ? ~b : (b | 0x80000000u));
}
__device__ __forceinline__ float score_of_bits(uint32_t d) {
  const uint32_t asc = ~d;
  return __uint_as_float((asc & 0x80000000u) ? (asc & 0x7FFFFFFFu) : ~asc);
}
__device__ __forceinline__ unsigned long long nb_key(float score, int32_t partner) {
  return ((unsigned long long)score_desc_bits(score) << 32) | (uint32_t)partner;
}

// the position of x in the ascending ids[0, u), or -1
__device__ __forceinline__ int32_t find_id(const int32_t* __restrict__ ids, int64_t u, int32_t x) {
  int64_t lo = 0, hi = u;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ids[mid] < x) lo = mid + 1; else hi = mid;
  }
  return (lo < u && ids[lo] == x) ? (int32_t)lo : -1;
}

// key[0, m) ascending in LDS with its payload (pay may be null), m a power of two >= 2; all threads of the workgroup.
// Exchange x pairs positions lo (bit j clear) and lo + j: consecutive x are consecutive words of both.
template <class K, class P>
__device__ __forceinline__ void lds_sort(K* key, P* pay, int m) {
  __syncthreads();
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int x = threadIdx.x; x < m / 2; x += kBlock) {
        const int lo = 2 * x - (x & (j - 1)), hi = lo + j;
        const K p = key[lo], q = key[hi];
        if ((p > q) == ((lo & k) == 0)) {
          key[lo] = q;
          key[hi] = p;
          if (pay) {
            const P t = pay[lo];
            pay[lo] = pay[hi];
            pay[hi] = t;
          }
        }
      }
      __syncthreads();
    }
  }
}
__device__ __forceinline__ int pow2_at_least(int n) {
  int m = 2;
  while (m < n) m <<= 1;
  return m;
}

// the workgroup's exclusive scan of one value per thread; `total` in every thread.  s_w: 4 words of LDS.
__device__ __forceinline__ unsigned long long block_scan_excl(unsigned long long v, unsigned long long* s_w,
                                                              unsigned long long& total) {
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  unsigned long long incl = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const unsigned long long up = __shfl_up(incl, off, kWave);
    if (lane >= off) incl += up;
  }
  __syncthreads();  // s_w of the previous call is no longer read
  if (lane == kWave - 1) s_w[wid] = incl;
  __syncthreads();
  unsigned long long before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kBlock / kWave; ++w) {
    if (w < wid) before += s_w[w];
    total += s_w[w];
  }
  return before + incl - v;
}
#endif

}  // namespace esr
