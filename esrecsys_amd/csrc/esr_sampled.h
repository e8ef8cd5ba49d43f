// What the units trained by sampled SGD (esr_bpr.hip, esr_warp.hip, esr_fpmc.hip, esr_sgns.hip) share beside the row layer
// of esr_row4.h: the failure bit and the grid cap, the argument checks every launcher repeats, and the shell of a sampler
// kernel -- one lane per slot, a workgroup on 256 consecutive slots of ONE step, the invalid slots of a wave counted with a
// ballot and added to dropped[k] by one integer atomic per wave.  The rule of a slot is the caller's (esr_*_sample.h).
#pragma once
#include <float.h>
#include <stdio.h>

#include <algorithm>
#include <initializer_list>

#include "esr_common.h"
#include "esr_row4.h"

namespace esr {

constexpr int kFailBadPosition = 1 << 30;                      // as FAIL_BAD_POSITION of esr_als.hip
constexpr int64_t kSampledMaxBlocks = (int64_t)kMaxGrid * 16;  // workgroups of a sampler or of warp_step: a stride beyond

// ---- the launchers' checks: ESR_OK, or ESR_EINVAL with the message set ----
inline int check_rank(const char* who, int D) {
  ESR_REQUIRE(D >= kRow4RankMultiple && D <= kRow4MaxRank && D % kRow4RankMultiple == 0,
              "%s: D=%d is not a multiple of %d in [%d, %d]", who, D, kRow4RankMultiple, kRow4RankMultiple, kRow4MaxRank);
  return ESR_OK;
}

inline int check_reg(const char* who, float reg) {
  ESR_REQUIRE(reg >= 0.f && reg <= FLT_MAX, "%s: reg=%g must be finite and not negative", who, (double)reg);
  return ESR_OK;
}

struct NamedSize {
  const char* name;
  int64_t value;
};
// every size in [1, 2^31 - 1]; `note` ends the parenthesis of the message
inline int check_sizes(const char* who, std::initializer_list<NamedSize> sizes, const char* note = "") {
  bool ok = true;
  char text[256] = "";
  size_t at = 0;
  for (const NamedSize& s : sizes) {
    ok = ok && s.value >= 1 && s.value <= (int64_t)INT32_MAX;
    if (at < sizeof text) at += (size_t)snprintf(text + at, sizeof text - at, " %s=%lld", s.name, (long long)s.value);
  }
  ESR_REQUIRE(ok, "%s: bad sizes%s (each in [1, 2^31 - 1]%s)", who, text, note);
  return ESR_OK;
}

// The launch of a sampler over K steps of B slots: K and B checked, dropped[K] zeroed on the stream, then `grid`
// workgroups over K * blocks_per_step (< 2^31 * 2^23: no overflow) blocks of kBlock slots.
inline int sample_plan(const char* who, int64_t K, int64_t B, int32_t* dropped, hipStream_t st, int& grid,
                       int64_t& blocks_per_step) {
  if (int rc = check_sizes(who, {{"K", K}, {"B", B}})) return rc;
  if (hipMemsetAsync(dropped, 0, (size_t)K * sizeof(int32_t), st) != hipSuccess) return check_launch(who);
  blocks_per_step = cdiv(B, kBlock);
  grid = (int)std::min<int64_t>(K * blocks_per_step, kSampledMaxBlocks);
  return ESR_OK;
}

// The body of a sampler kernel: draw(k, t, at) draws slot t of step k, writes its words at k * B + t and returns whether
// it is valid.  Integer arithmetic only; no workgroup waits on another and nothing is polled.
template <class Draw>
__device__ __forceinline__ void sample_slots(int64_t K, int64_t B, int64_t blocks_per_step, int32_t* __restrict__ dropped,
                                             Draw draw) {
  const int64_t nblocks = K * blocks_per_step;
  for (int64_t w = blockIdx.x; w < nblocks; w += gridDim.x) {  // (uniform per workgroup)
    const int64_t k = w / blocks_per_step, t = (w % blocks_per_step) * kBlock + threadIdx.x;
    const bool bad = t < B && !draw(k, t, k * B + t);
    const unsigned long long mask = __ballot(bad);
    if ((threadIdx.x & (kWave - 1)) == 0 && mask) atomicAdd(dropped + k, (int32_t)__popcll(mask));
  }
}

}  // namespace esr
