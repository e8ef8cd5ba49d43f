// Diversity re-ranking on the device: Maximal Marginal Relevance over a query's candidate list and the intra-list
// similarity of a list.  The rule of both is esr_rerank_rule.h's; rerank.py and _Factorization.diversify drive them.
//
// Launch.  One workgroup of kBlock threads per query, grid-stride past kMaxGrid.  The query's candidates are dealt to the
// kBlock / G lane groups of the float4 row-group layout (esr_row4.h): group g owns candidates g, g + kBlock / G, ...
//
// LDS.  Per candidate 16 bytes of state (MMR: m, rel, position, flags; ILS: the fp64 row sum and the position), owned by
// the candidate's group.  When width * D * 4 <= kRerankStageBytes the candidates' rows are copied into LDS once per query
// (STAGED) and every later read of a row is an LDS read; otherwise the rows are read from global memory each round.  The
// form is chosen by (width, D) alone and both forms run the same sim expression (warp_lane_dot + group_sum): the same bits.
//
// MMR round.  Every group folds the values of its candidates into one (v, c) pair while it updates them (one pass per
// round: the update after pick t computes the values of round t + 1); the pairs meet in a wave reduction (DPP / ds_swizzle,
// as group_sum) and a four-wave exchange through LDS, double-buffered so that a round costs one barrier.  (v, c) is a total
// order, so the partition does not enter.  The picked row is read once per round into registers.
//
// ILS.  A group owns position i, keeps row i in registers and walks j < i in ascending order (an fp64 chain); thread 0
// forms the prefix over i (<= 1024 fp64 additions).  Positions are dealt round-robin, so the groups' loads differ by at most
// one position's walk; the imbalance inside a round is accepted.
//
// Only bounded loops (n_out rounds, width / groups candidates); no workgroup waits on another, nothing is polled, no float
// atomic; the failure bits are one integer atomicOr per thread that met one.  Registers and LDS: DESIGN.md section 4m.
#include "esr_common.h"
#include "esr_rerank_rule.h"
#include "esr_row4.h"

namespace esr {

__device__ __forceinline__ float rerank_group_sim(const float4& x, const float4& y, int G) {
  return group_sum(warp_lane_dot(x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w), G);
}

// The best (v, c) of the wave in every lane.  The lanes of a group hold one pair: the exchange starts at stride G.
template <int G>
__device__ __forceinline__ void rerank_wave_best(float& v, int& c) {
#define ESR_RERANK_STEP(S)                                                  \
  if (G <= S) {                                                             \
    const float ov = __uint_as_float(xor_lane(__float_as_uint(v), S));      \
    const int oc = (int)xor_lane((uint32_t)c, S);                           \
    if (rerank_better(ov, oc, v, c)) v = ov, c = oc;                        \
  }
  ESR_RERANK_STEP(1) ESR_RERANK_STEP(2) ESR_RERANK_STEP(4) ESR_RERANK_STEP(8) ESR_RERANK_STEP(16) ESR_RERANK_STEP(32)
#undef ESR_RERANK_STEP
}

template <int G, bool STAGED>
__global__ __launch_bounds__(kBlock) void rerank_mmr_kernel(const float* __restrict__ rows, int64_t ni, int D,
                                                            const int32_t* __restrict__ cand, const float* __restrict__ rel,
                                                            const int32_t* __restrict__ lengths, int64_t nq, int width,
                                                            int n_out, float lam, int32_t* __restrict__ out_pos,
                                                            int32_t* __restrict__ out_item, float* __restrict__ out_rel,
                                                            float* __restrict__ out_value, int32_t* __restrict__ out_length,
                                                            int32_t* __restrict__ failed) {
  extern __shared__ __attribute__((aligned(16))) char rerank_lds[];
  __shared__ float ex_v[2][kBlock / kWave];
  __shared__ int ex_c[2][kBlock / kWave];
  float* m_s = reinterpret_cast<float*>(rerank_lds);
  float* rel_s = m_s + width;
  int32_t* pos_s = reinterpret_cast<int32_t*>(rel_s + width);
  int32_t* st_s = pos_s + width;
  float* rows_s = reinterpret_cast<float*>(st_s + width);  // (16 width bytes in: float4-aligned)
  constexpr int NG = kBlock / G;
  const int lig = row4_lig<G>(), grp = threadIdx.x / G, lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const bool holds = row4_holds(lig, D);
  const float oml = 1.0f - lam;
  int fail = 0;
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const int L = rerank_length(lengths, q, width);
    const int32_t* cq = cand + q * width;
    const float* rq = rel + q * width;
    __syncthreads();  // (the query before this one is done with the state)
    for (int c = threadIdx.x; c < L; c += kBlock) {
      const int32_t p = cq[c];
      const float r = rq[c];
      const int bits = rerank_absent_bits(p, r, ni);
      fail |= bits;
      pos_s[c] = p, rel_s[c] = r, st_s[c] = bits ? 0 : kRerankPresent, m_s[c] = 0.0f;
    }
    __syncthreads();
    float bv = -INFINITY;
    int bc = kRerankNone;
    for (int c = grp; c < L; c += NG) {  // stage the rows; the values of round 0
      if (st_s[c] != kRerankPresent) continue;
      if (STAGED && holds) *reinterpret_cast<float4*>(rows_s + c * D + 4 * lig) = *row4_ptr(rows, pos_s[c], D, lig);
      const float v = rerank_value(lam, oml, rel_s[c], 0.0f);
      if (rerank_better(v, c, bv, bc)) bv = v, bc = c;
    }
    int t = 0;
    for (; t < n_out; ++t) {
      rerank_wave_best<G>(bv, bc);
      if (lane == 0) ex_v[t & 1][wid] = bv, ex_c[t & 1][wid] = bc;
      __syncthreads();  // (also: round 0's staged rows, the round before's m and flags)
      bv = ex_v[t & 1][0], bc = ex_c[t & 1][0];
#pragma unroll
      for (int w = 1; w < kBlock / kWave; ++w) {
        const float ov = ex_v[t & 1][w];
        const int oc = ex_c[t & 1][w];
        if (rerank_better(ov, oc, bv, bc)) bv = ov, bc = oc;
      }
      if (bc == kRerankNone) break;  // (uniform over the workgroup: the list ends here)
      const int s = bc;
      if (threadIdx.x == 0) {
        const int64_t o = q * n_out + t;
        out_pos[o] = s, out_item[o] = pos_s[s], out_rel[o] = rel_s[s], out_value[o] = bv;
      }
      float4 ps = row4_zero();  // the picked row: once per round, in registers
      if (holds) ps = STAGED ? *reinterpret_cast<const float4*>(rows_s + s * D + 4 * lig) : *row4_ptr(rows, pos_s[s], D, lig);
      bv = -INFINITY, bc = kRerankNone;
      for (int c = grp; c < L; c += NG) {
        const int st = st_s[c];
        if (c == s) {
          if (lig == 0) st_s[c] = st | kRerankPicked;
          continue;
        }
        if (st != kRerankPresent) continue;
        float4 y = row4_zero();
        if (holds) y = STAGED ? *reinterpret_cast<const float4*>(rows_s + c * D + 4 * lig) : *row4_ptr(rows, pos_s[c], D, lig);
        const float sim = rerank_group_sim(y, ps, G);
        const float mc = t == 0 ? sim : fmaxf(m_s[c], sim);
        if (lig == 0) m_s[c] = mc;
        const float v = rerank_value(lam, oml, rel_s[c], mc);
        if (rerank_better(v, c, bv, bc)) bv = v, bc = c;
      }
    }
    for (int i = t + threadIdx.x; i < n_out; i += kBlock) {
      const int64_t o = q * n_out + i;
      out_pos[o] = -1, out_item[o] = -1, out_rel[o] = 0.0f, out_value[o] = 0.0f;
    }
    if (threadIdx.x == 0) out_length[q] = t;
  }
  if (fail) atomicOr(failed, fail);
}

struct RerankCutoffs {
  int32_t k[kRerankMaxCutoffs];
  int nk;
};

template <int G, bool STAGED>
__global__ __launch_bounds__(kBlock) void rerank_ils_kernel(const float* __restrict__ rows, int64_t ni, int D,
                                                            const int32_t* __restrict__ cand,
                                                            const int32_t* __restrict__ lengths, int64_t nq, int width,
                                                            RerankCutoffs ks, float* __restrict__ ils,
                                                            int32_t* __restrict__ valid, int32_t* __restrict__ failed) {
  extern __shared__ __attribute__((aligned(16))) char rerank_lds[];
  double* r_s = reinterpret_cast<double*>(rerank_lds);
  int32_t* pos_s = reinterpret_cast<int32_t*>(r_s + width);  // (-1: absent)
  float* rows_s = reinterpret_cast<float*>(rerank_lds + (size_t)width * kRerankStateBytes);
  constexpr int NG = kBlock / G;
  const int lig = row4_lig<G>(), grp = threadIdx.x / G;
  const bool holds = row4_holds(lig, D);
  int fail = 0;
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const int L = rerank_length(lengths, q, width);
    const int kmax = ks.k[ks.nk - 1] < L ? ks.k[ks.nk - 1] : L;
    const int32_t* cq = cand + q * width;
    __syncthreads();
    for (int c = threadIdx.x; c < kmax; c += kBlock) {
      const int32_t p = cq[c];
      const bool ok = p >= 0 && (int64_t)p < ni;
      if (!ok) fail |= kRerankFailPos;
      pos_s[c] = ok ? p : -1, r_s[c] = 0.0;
    }
    __syncthreads();
    if (STAGED) {
      for (int c = grp; c < kmax; c += NG)
        if (pos_s[c] >= 0 && holds) *reinterpret_cast<float4*>(rows_s + c * D + 4 * lig) = *row4_ptr(rows, pos_s[c], D, lig);
      __syncthreads();
    }
    for (int i = grp; i < kmax; i += NG) {
      if (pos_s[i] < 0) continue;
      float4 x = row4_zero();
      if (holds) x = STAGED ? *reinterpret_cast<const float4*>(rows_s + i * D + 4 * lig) : *row4_ptr(rows, pos_s[i], D, lig);
      double r = 0.0;
      for (int j = 0; j < i; ++j) {
        if (pos_s[j] < 0) continue;
        float4 y = row4_zero();
        if (holds) y = STAGED ? *reinterpret_cast<const float4*>(rows_s + j * D + 4 * lig) : *row4_ptr(rows, pos_s[j], D, lig);
        r += (double)rerank_group_sim(x, y, G);
      }
      if (lig == 0) r_s[i] = r;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // the prefix over positions and the cutoffs it closes, as rerank_ils_query
      double P = 0.0;
      int n = 0, j = 0;
      for (int i = 0; i <= kmax; ++i) {
        for (; j < ks.nk && (ks.k[j] < L ? ks.k[j] : L) == i; ++j) {
          const bool ok = n >= 2;
          ils[q * ks.nk + j] = ok ? (float)(P / ((double)n * (double)(n - 1) * 0.5)) : 0.0f;
          valid[q * ks.nk + j] = ok;
        }
        if (i == kmax || pos_s[i] < 0) continue;
        P += r_s[i];
        n += 1;
      }
    }
  }
  if (fail) atomicOr(failed, fail);
}

// what the entry points check alike; 0 when the arguments stand
static int rerank_args(const char* who, const float* rows, int64_t ni, int D, const int32_t* cand, const int32_t* lengths,
                       int64_t nq, int width, int32_t* failed) {
  ESR_REQUIRE(D >= kRerankRankMultiple && D <= kRerankMaxRank && D % kRerankRankMultiple == 0,
              "%s: D=%d is not a multiple of %d in [%d, %d]", who, D, kRerankRankMultiple, kRerankRankMultiple, kRerankMaxRank);
  ESR_REQUIRE(width >= 1 && width <= kRerankMaxWidth, "%s: list width=%d not in [1, %d]", who, width, kRerankMaxWidth);
  ESR_REQUIRE(ni >= 1 && ni <= (int64_t)INT32_MAX && nq >= 0 && nq <= (int64_t)INT32_MAX,
              "%s: bad sizes ni=%lld nq=%lld (ni in [1, 2^31 - 1], nq in [0, 2^31 - 1])", who, (long long)ni, (long long)nq);
  ESR_REQUIRE(rows && cand && failed, "%s: null pointer", who);
  ESR_REQUIRE(((uintptr_t)rows & 15) == 0 && (((uintptr_t)cand | (uintptr_t)lengths | (uintptr_t)failed) & 3) == 0,
              "%s: misaligned pointer (rows: 16 bytes, the other arrays: 4)", who);
  return ESR_OK;
}

// a kernel instance that stages rows needs more dynamic LDS than the 64 KiB a kernel gets unasked
static int rerank_raise_lds(const char* who, const void* kernel, bool* done) {
  if (*done) return ESR_OK;
  const int most = kRerankStageBytes + kRerankMaxWidth * kRerankStateBytes;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess) {
    set_error("%s: cannot raise the LDS limit", who);
    return ESR_ELAUNCH;
  }
  *done = true;
  return ESR_OK;
}

template <int G, bool STAGED>
static int launch_mmr(const char* who, hipStream_t st, int grid, int lds, const float* rows, int64_t ni, int D,
                      const int32_t* cand, const float* rel, const int32_t* lengths, int64_t nq, int width, int n_out,
                      float lam, int32_t* out_pos, int32_t* out_item, float* out_rel, float* out_value, int32_t* out_length,
                      int32_t* failed) {
  static bool raised = false;
  if (STAGED)
    if (int rc = rerank_raise_lds(who, (const void*)rerank_mmr_kernel<G, STAGED>, &raised)) return rc;
  ESR_KT("rerank_mmr", st,
         hipLaunchKernelGGL((rerank_mmr_kernel<G, STAGED>), dim3(grid), dim3(kBlock), lds, st, rows, ni, D, cand, rel, lengths,
                            nq, width, n_out, lam, out_pos, out_item, out_rel, out_value, out_length, failed));
  return check_launch(who);
}

template <int G, bool STAGED>
static int launch_ils(const char* who, hipStream_t st, int grid, int lds, const float* rows, int64_t ni, int D,
                      const int32_t* cand, const int32_t* lengths, int64_t nq, int width, const RerankCutoffs& ks, float* ils,
                      int32_t* valid, int32_t* failed) {
  static bool raised = false;
  if (STAGED)
    if (int rc = rerank_raise_lds(who, (const void*)rerank_ils_kernel<G, STAGED>, &raised)) return rc;
  ESR_KT("rerank_ils", st,
         hipLaunchKernelGGL((rerank_ils_kernel<G, STAGED>), dim3(grid), dim3(kBlock), lds, st, rows, ni, D, cand, lengths, nq,
                            width, ks, ils, valid, failed));
  return check_launch(who);
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_rerank_geometry(int D, int width, int* max_rank, int* rank_multiple, int* max_width, int* max_cutoffs,
                        int* stage_bytes, int* grid_cap, int* staged, int* lds_bytes) {
  const char* who = "esr_rerank_geometry";
  ESR_REQUIRE(max_rank && rank_multiple && max_width && max_cutoffs && stage_bytes && grid_cap && staged && lds_bytes,
              "%s: null pointer", who);
  ESR_REQUIRE(D >= kRerankRankMultiple && D <= kRerankMaxRank && D % kRerankRankMultiple == 0,
              "%s: D=%d is not a multiple of %d in [%d, %d]", who, D, kRerankRankMultiple, kRerankRankMultiple, kRerankMaxRank);
  ESR_REQUIRE(width >= 1 && width <= kRerankMaxWidth, "%s: list width=%d not in [1, %d]", who, width, kRerankMaxWidth);
  *max_rank = kRerankMaxRank, *rank_multiple = kRerankRankMultiple, *max_width = kRerankMaxWidth;
  *max_cutoffs = kRerankMaxCutoffs, *stage_bytes = kRerankStageBytes, *grid_cap = kMaxGrid;
  *staged = rerank_staged(width, D), *lds_bytes = rerank_lds_bytes(width, D);
  return ESR_OK;
}

int esr_rerank_mmr(const float* rows, int64_t ni, int D, const int32_t* cand, const float* rel, const int32_t* lengths,
                   int64_t nq, int width, int n_out, float lam, int32_t* out_pos, int32_t* out_item, float* out_rel,
                   float* out_value, int32_t* out_length, int32_t* failed, esr_stream_t stream) {
  TraceScope trace_scope_("esr_rerank_mmr");
  const char* who = "esr_rerank_mmr";
  if (int rc = rerank_args(who, rows, ni, D, cand, lengths, nq, width, failed)) return rc;
  ESR_REQUIRE(n_out >= 1 && n_out <= width, "%s: n_out=%d not in [1, width=%d]", who, n_out, width);
  ESR_REQUIRE(lam >= 0.0f && lam <= 1.0f, "%s: lam=%g not in [0, 1]", who, (double)lam);
  ESR_REQUIRE(rel && out_pos && out_item && out_rel && out_value && out_length, "%s: null pointer", who);
  ESR_REQUIRE((((uintptr_t)rel | (uintptr_t)out_pos | (uintptr_t)out_item | (uintptr_t)out_rel | (uintptr_t)out_value |
                (uintptr_t)out_length) & 3) == 0,
              "%s: misaligned pointer (rows: 16 bytes, the other arrays: 4)", who);
  if (nq == 0) return ESR_OK;
  hipStream_t st = as_stream(stream);
  const int G = row4_lanes(D), grid = (int)std::min<int64_t>(kMaxGrid, nq), lds = rerank_lds_bytes(width, D);
  int rc = ESR_OK;
  if (rerank_staged(width, D)) {
    ESR_DISPATCH_G(G, rc = launch_mmr<GG, true>(who, st, grid, lds, rows, ni, D, cand, rel, lengths, nq, width, n_out, lam,
                                                out_pos, out_item, out_rel, out_value, out_length, failed));
  } else {
    ESR_DISPATCH_G(G, rc = launch_mmr<GG, false>(who, st, grid, lds, rows, ni, D, cand, rel, lengths, nq, width, n_out, lam,
                                                 out_pos, out_item, out_rel, out_value, out_length, failed));
  }
  return rc;
}

int esr_rerank_ils(const float* rows, int64_t ni, int D, const int32_t* cand, const int32_t* lengths, int64_t nq, int width,
                   const int32_t* ks, int nk, float* ils, int32_t* valid, int32_t* failed, esr_stream_t stream) {
  TraceScope trace_scope_("esr_rerank_ils");
  const char* who = "esr_rerank_ils";
  if (int rc = rerank_args(who, rows, ni, D, cand, lengths, nq, width, failed)) return rc;
  ESR_REQUIRE(ks && nk >= 1 && nk <= kRerankMaxCutoffs, "%s: nk=%d cutoffs not in [1, %d] (or null ks)", who, nk,
              kRerankMaxCutoffs);
  RerankCutoffs cut;
  cut.nk = nk;
  for (int j = 0; j < kRerankMaxCutoffs; ++j) cut.k[j] = j < nk ? ks[j] : INT32_MAX;
  for (int j = 0; j < nk; ++j)
    ESR_REQUIRE(ks[j] >= 1 && (j == 0 || ks[j] > ks[j - 1]), "%s: ks must be strictly ascending and >= 1 (ks[%d]=%d)", who, j,
                ks[j]);
  ESR_REQUIRE(ils && valid, "%s: null pointer", who);
  ESR_REQUIRE((((uintptr_t)ils | (uintptr_t)valid) & 3) == 0, "%s: misaligned pointer (rows: 16 bytes, the other arrays: 4)",
              who);
  if (nq == 0) return ESR_OK;
  hipStream_t st = as_stream(stream);
  const int G = row4_lanes(D), grid = (int)std::min<int64_t>(kMaxGrid, nq), lds = rerank_lds_bytes(width, D);
  int rc = ESR_OK;
  if (rerank_staged(width, D)) {
    ESR_DISPATCH_G(G, rc = launch_ils<GG, true>(who, st, grid, lds, rows, ni, D, cand, lengths, nq, width, cut, ils, valid,
                                                failed));
  } else {
    ESR_DISPATCH_G(G, rc = launch_ils<GG, false>(who, st, grid, lds, rows, ni, D, cand, lengths, nq, width, cut, ils, valid,
                                                 failed));
  }
  return rc;
}

}  // extern "C"
