// The row-sparse update engine (esr_optim.hip) as other translation units see it: the fused-table argument of its kernels
// and the internal entry points the in-batch step (esr_inbatch2h.hip) and the Spotify step (esr_spotify.hip) call.
#pragma once
#include "esr_common.h"

namespace esr {

// Several tables may be updated by ONE sorted occurrence list: occurrence ids are then "virtual rows"
// vid = row_offset[t] + id of a concatenation of up to kMaxFusedTables tables with the same D (the two towers of one
// step), so a step needs one sort and one update instead of one per table -- at the reference's batch sizes the step
// is bound by the number of dependent launches, not by bytes.  A single table is the n = 1 case.
constexpr int kMaxFusedTables = 4;
struct FusedTables {
  void* table[kMaxFusedTables];
  float* accum[kMaxFusedTables];                // the tables' one state plane (accumulator, trace, mu); null where an op has none
  int64_t row_offset[kMaxFusedTables + 1];      // slots past n repeat row_offset[n], the end of the last table
  int n;
};

// a run of equal ids longer than this is summed chunk-wise (segment_update_kernel in esr_optim.hip)
constexpr int kSegChunk = 32;

struct InbatchMergeArgs;  // esr_inbatch_mfma.h

// esr_sparse_adagrad_scatter_multi over a SUB-RANGE of a sorted occurrence list
int sparse_adagrad_range(void* const* tables, float* const* accums, const int64_t* row_offsets, int ntables, int dtype,
                         int D, const int32_t* sorted_vids, const int32_t* perm, int64_t n, float* grad_rows, float lr,
                         float eps, bool skip_long, hipStream_t st);
// the in-batch step's merge launches and its sparse Adagrad update of both towers in one kernel
int inbatch_merge_update(void* const* tables, float* const* accums, const int64_t* row_offsets, int dtype,
                         const int32_t* sorted_vids, const int32_t* perm, const InbatchMergeArgs& a, float lr, float eps,
                         hipStream_t st);
// esr_sparse_momentum_step_multi for one or two tables whose rows may be behind: catch-up + step + mark
int sparse_momentum_step_lazy2(float* const* tables, float* const* traces, int32_t* const* lasts, const int64_t* row_offsets,
                               int ntables, int D, const int32_t* sorted_vids, const int32_t* perm, int64_t n, float* grad_rows,
                               float lr, float momentum, int now, hipStream_t st);

#ifdef __HIPCC__
// ---- the long runs, written once ---------------------------------------------------------------------------------------
// A run of equal sorted ids that outgrows its head chunk is cut at the multiples of CHUNK: partial 0 = the head chunk
// [h, nxt), h the run's head and nxt the first chunk boundary at least CHUNK positions later; partial i >= 1 = the CHUNK
// positions from nxt + (i - 1) CHUNK; K = the number of continuation chunks.  The update kernels (segment_update_kernel,
// glove_step_kernel, triplet_step_kernel) leave one partial sum per chunk; what follows combines them, for the segment
// engine (esr_optim.hip) and the one-pass steps (esr_glove.hip, esr_triplet_step.hip) alike: row group gi of the workgroup
// adds partials gi, gi + NG, ... in order, the groups' sums are added in group order.  Fixed association: a hot row gets
// the same bits from every one of them, whatever the scheduling.

// position of the first occurrence of partial i
__device__ __forceinline__ int64_t long_part_pos(int64_t h, int64_t nxt, int64_t i, int chunk) {
  return i == 0 ? h : nxt + (i - 1) * chunk;
}
struct BarrierOnly {
  template <class... A>
  __device__ __forceinline__ void operator()(A...) const { __syncthreads(); }
};
// The groups' sums `acc` of a run of K + 1 partials -> their sum in group order, in group 0's registers (true there).
// `publish` runs on all threads between the spill and the fold and must contain a barrier: by default it is one.
template <int VEC, int NCH, class Publish = BarrierOnly>
__device__ __forceinline__ bool combine_groups(RowRegs<VEC, NCH>& acc, int64_t K, int G, Publish publish = {}) {
  __shared__ float red[kBlock * VEC * NCH];  // [groups][lanes][NCH][VEC]
  const int tid = threadIdx.x, lig = tid & (G - 1), gidx = tid / G, NG = kBlock / G;
#pragma unroll
  for (int k = 0; k < NCH; ++k)
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[((gidx * G + lig) * NCH + k) * VEC + e] = acc.v[k][e];
  publish();
  if (gidx != 0) return false;
  const int used = (int)min<int64_t>(NG, K + 1);
  for (int gg = 1; gg < used; ++gg)
#pragma unroll
    for (int k = 0; k < NCH; ++k)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc.v[k][e] += red[((gg * G + lig) * NCH + k) * VEC + e];
  return true;
}

// The whole combining kernel but its prologue.  The first continuation chunk of every long run is found by screening the
// chunk boundaries (three loads per boundary; in a batch without hot rows that is all this does); the workgroup then
// combines one run at a time.
//   part(h, nxt, i)            -> the f32 row that holds partial i
//   done(id, h, nxt, K, acc)   row group 0 only: the finished sum
//   fold(h, nxt, K)            optional; all threads, between the spill of the group sums and their combination, IN PLACE
//                              of the barrier there (so it must contain one: GloVe's bias sums, through block_sum_d)
template <int VEC, int NCH, int CHUNK, class Part, class Done, class Fold = BarrierOnly>
__device__ __forceinline__ void combine_long_runs(const int32_t* __restrict__ sorted_ids, int64_t n, int D, int G, Part part,
                                                  Done done, Fold fold = {}) {
  constexpr int kPass = 4;             // chunk boundaries screened per workgroup pass (long runs are then spread over
                                       // many workgroups instead of queueing in a few)
  __shared__ long long s_long[kPass];  // chunk boundaries at which a long run leaves its first chunk
  __shared__ int s_nlong, s_hoff;
  const int tid = threadIdx.x, lig = tid & (G - 1), gidx = tid / G, NG = kBlock / G;
  const int nvec = D / VEC;
  const int64_t nbound = (n - 1) / CHUNK;  // boundaries CHUNK, 2 CHUNK, ... < n
  for (int64_t b0 = (int64_t)blockIdx.x * kPass; b0 < nbound; b0 += (int64_t)gridDim.x * kPass) {
    __syncthreads();  // red / s_* of the previous pass are no longer read
    if (tid == 0) s_nlong = 0;
    __syncthreads();
    // screening, one thread per chunk boundary B: B is the FIRST continuation chunk of a long run iff the whole
    // block before it belongs to the run (ids at B - CHUNK and B equal) and the block before that does not
    {
      const int64_t B = (b0 + tid + 1) * CHUNK;
      if (tid < kPass && b0 + tid < nbound) {
        const int32_t id_b = sorted_ids[B];
        const bool first = B < 2 * CHUNK || sorted_ids[B - 2 * CHUNK] != id_b;
        if (sorted_ids[B - CHUNK] == id_b && first) s_long[atomicAdd(&s_nlong, 1)] = B;
      }
    }
    __syncthreads();
    const int nlong = s_nlong;
    for (int li = 0; li < nlong; ++li) {  // rare: the whole workgroup combines one long run at a time
      // (the order of the list is arbitrary; it affects no result: every run is combined independently)
      const int64_t nxt = s_long[li];
      const int32_t id = sorted_ids[nxt];
      const int64_t win = max<int64_t>(nxt - 2 * CHUNK + 1, 0);  // the head lies in [nxt - 2 CHUNK + 1, nxt - CHUNK]
      if (tid < 64) {
        const int64_t pos = win + tid;
        const bool is_head = pos <= nxt - CHUNK && sorted_ids[pos] == id && (pos == 0 || sorted_ids[pos - 1] != id);
        const unsigned long long m = __ballot(is_head);
        if (tid == 0) s_hoff = __ffsll((long long)m) - 1;
      }
      __syncthreads();
      const int64_t h = win + s_hoff;
      // K = number of continuation chunks (chunk starts nxt, nxt + CHUNK, ... that still carry this id)
      int64_t K = 0;
      for (int64_t k0 = 0;; k0 += kBlock) {
        const int64_t pos = nxt + (k0 + tid) * CHUNK;
        const int cnt = __syncthreads_count(pos < n && sorted_ids[pos] == id);
        K += cnt;
        if (cnt < kBlock) break;
      }
      RowRegs<VEC, NCH> acc;
      row_zero(acc);
      int64_t i = gidx;
      for (; i + 3 * NG <= K; i += 4 * NG) {  // four partials in flight, added in order
        RowRegs<VEC, NCH> t0, t1, t2, t3;
        row_load(t0, part(h, nxt, i), lig, G, nvec);
        row_load(t1, part(h, nxt, i + NG), lig, G, nvec);
        row_load(t2, part(h, nxt, i + 2 * NG), lig, G, nvec);
        row_load(t3, part(h, nxt, i + 3 * NG), lig, G, nvec);
        row_add4(acc, t0, t1, t2, t3);
      }
      for (; i <= K; i += NG) {
        RowRegs<VEC, NCH> t;
        row_load(t, part(h, nxt, i), lig, G, nvec);
        row_add(acc, t);
      }
      if (combine_groups(acc, K, G, [&]() { fold(h, nxt, K); })) done(id, h, nxt, K, acc);
      __syncthreads();  // red is rewritten by the next long run
    }
  }
}
#endif

}  // namespace esr
