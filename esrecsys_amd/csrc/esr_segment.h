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

}  // namespace esr
