// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) and what
// the Spotify negative sampler and its group call derive from it.  Plain integer C++ with no HIP dependency of its own:
// the kernels of esr_spotify.hip, the host side of the library and a stand-alone host program include the same text.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ESR_HD __host__ __device__
#else
#define ESR_HD
#endif

namespace esr {

// out = philox4x32-10(counter, key): ten rounds of two 32 x 32 -> 64 multiplies, the key raised by the Weyl constants
// between rounds.
ESR_HD inline void philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3], k0 = key[0], k1 = key[1];
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Negative i of global step s under `seed`: counter (i >> 2, s, 0, 0), key (seed low, seed high), word i & 3, mapped to
// [0, tm1) by multiply-high (tm1 = T - 1 <= 2^31 - 1: the last track is never drawn, train_spotify.py:146).  The relative
// bias of multiply-high is at most tm1 / 2^32.
ESR_HD inline uint32_t sp_negative_index(uint64_t seed, uint32_t step, uint32_t i, uint32_t tm1) {
  const uint32_t counter[4] = {i >> 2, step, 0u, 0u}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t w[4];
  philox4x32_10(counter, key, w);
  return (uint32_t)(((uint64_t)w[i & 3] * tm1) >> 32);
}

// Where step j's id lists start inside the group call's list region, in int32 units: [album ids R_j][artist ids R_j] with
// R_j = n + m_j + o.  A closed form of (j, next_offsets[j]) -- no prefix sum over the ragged lengths -- that is 256-byte
// aligned and leaves every block at least one int clear of the next: the unaligned running start u_j = 2 (j (n + o) +
// next_offsets[j]) rounded up to 64 ints, plus 64 j.
ESR_HD inline int64_t sp_list_start(int64_t j, int n, int o, int64_t next_offset_j) {
  const int64_t u = 2 * (j * ((int64_t)n + o) + next_offset_j);
  return (u + 63) / 64 * 64 + 64 * j;
}
// ints of the whole region for K steps whose next lists hold total_next ids
ESR_HD inline int64_t sp_list_region(int64_t K, int n, int o, int64_t total_next) { return sp_list_start(K, n, o, total_next); }

// The host offsets of a group: next_offsets[0] = 0, every list non-empty (strictly increasing).  Returns 0 and the longest
// list in *max_m, or 1 + the index of the first offending entry.
inline int64_t sp_check_offsets(const int64_t* next_offsets, int64_t K, int64_t* max_m) {
  if (next_offsets[0] != 0) return 1;
  int64_t mm = 0;
  for (int64_t j = 0; j < K; ++j) {
    if (next_offsets[j + 1] <= next_offsets[j]) return j + 2;
    const int64_t m = next_offsets[j + 1] - next_offsets[j];  // (both >= 0 here: no overflow)
    if (m > mm) mm = m;
  }
  *max_m = mm;
  return 0;
}

}  // namespace esr
