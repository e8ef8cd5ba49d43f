// Matrix factorisation of explicit ratings by alternating least squares: esr_als_*.  One half-sweep solves, for every row
// u of one side (n ratings, columns c_k into the OTHER side's factor table Y [n_other, rank], targets d_k),
//     (sum_k y_k y_k^T + lam I) x_u = sum_k d_k y_k,      lam = reg * (weighted ? n : 1),     y_k = Y[c_k].
//   gram        on v_mfma_f32_32x32x2_f32: the A operand of a diagonal 32 x 32 tile of Y^T Y and its B operand are the SAME
//               register -- lane l holds y_{k0 + (l >> 5)}[l & 31], so a rating's factor row is one coalesced gather
//               straight into VGPRs (no LDS staging) and an instruction consumes two ratings.  rank > 32: a second register
//               (dims 32..63) feeds the tiles (hi, lo) and (hi, hi); the tile (lo, hi) is the transpose of (hi, lo) bit for
//               bit and is never computed -- the Cholesky reads the lower triangle only.  Lanes at or above rank and the odd
//               rating at a chunk's tail supply 0.  The right-hand side runs on the VALU beside it: lane l sums d_k y_k[l & 31]
//               over the ratings of its parity, the two parities are added at the chunk's end (even + odd).
//   order       a row's ratings are taken in CSR order and cut into chunks of kAlsChunk; a chunk's Gram entries are the
//               k-ordered f32 fmaf chain from 0 that the MFMA gives, the chunk partials (Gram and right-hand side) are added
//               in ascending chunk order in f32, then lam is added on the diagonal, then an f32 Cholesky (left-looking,
//               column j: s = a_ij; s = fmaf(-l_ik, l_jk, s) for k ascending; l_jj = sqrt(s_j), l_ij = s / l_jj) and the
//               two triangular solves (column-oriented, fmaf(-l, z, b)) by ONE wave on the matrix in LDS.  The output row
//               is a function of that row's ratings, Y, reg and weighted alone: not of the grid, of the cut into launches or
//               of the other rows.  No atomics on floating-point data.
//   rows        three classes by length, each with its own fixed schedule (the HOST sorts the rows into them: it holds the
//               row offsets):  <= kAlsChunk ratings: a wave per row;  <= kAlsChunk * kAlsChunksPerWg: a workgroup per row,
//               wave w takes chunk w, the partials are summed in LDS in chunk order;  longer: a wave per chunk writes its
//               partial to the workspace, a second launch (a workgroup per row) sums them in chunk order and solves.
//   failures    a column outside [0, n_other) is never dereferenced: its rating counts as absent and bit 30 of *failed is
//               set; a pivot that is not finite and positive (or a solution that is not finite) leaves the output row as it
//               was and adds 1 to *failed.
//
// Implicit feedback (Hu, Koren, Volinsky 2008): esr_als_gram and esr_als_solve_rows_implicit.  Every cell of the matrix is
// fitted, preference 1 on a row's entries and 0 elsewhere, confidence 1 + w_k on the entries (w_k: a float per entry) and 1
// elsewhere, so a row solves
//     (G + sum_k w_k y_k y_k^T + lam I) x = sum_k c_k y_k,     G = Y^T Y,   c_k = fl32(1 + w_k),   lam = reg * (weighted ? n : 1).
//   whole gram  esr_als_gram: the table is cut into segments of kAlsGramSegment consecutive rows; ONE wave owns a segment and
//               accumulates its lower block triangle as one k-ordered f32 fmaf chain from 0 on the same MFMA scheme (both
//               operands the same register, rows gathered straight into VGPRs, lanes at or above rank and an odd tail supply
//               0) and writes it to the workspace; a second launch adds the segment partials per entry in fp64 in ascending
//               segment order, rounds once to f32 and writes the entry and its mirror.  G is a function of the table alone:
//               not of the grid, and a trailing all-zero row adds fma(0, 0, acc) = acc or a partial of zeros.
//   order       (1) a row's entries in CSR order, cut into chunks of kAlsChunk as above; (2) within a chunk the lower-triangle
//               entry (i, j), i >= j, is the k-ordered chain acc = fmaf(fl32(w_k * y_k[i]), y_k[j], acc) from 0 -- one VALU
//               multiply per MFMA step scales the A operand, which indexes the row; (3) the right-hand side is
//               fmaf(c_k, y_k[d], acc) over the chunk's even entries plus the same chain over its odd ones; (4) chunk partials
//               are added in ascending order in f32; (5) then G[i][j] is added; (6) then lam on the diagonal; (7) then the
//               Cholesky and the two solves above.  The same three row classes, the same workspace layout.
//   failures    as above, and a weight that is negative or not finite counts as absent and sets bit 29 of *failed.
// No kernel waits on another workgroup; every loop is bounded by a length the host wrote into the unit lists.
#include <math.h>

#include <vector>

#include "esr_common.h"
#include "esr_row4.h"

namespace esr {

typedef float als_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kAlsMaxRank = 64;                 // the solves and the Gram: one wave holds a rank x rank f32 matrix in LDS
constexpr int kAlsPredictMaxRank = kRow4MaxRank;  // predict is a per-pair loop over the row: the widest row-group table
constexpr int kAlsChunk = 256;                  // ratings per chunk (even: an MFMA step takes two)
constexpr int kAlsWaves = kBlock / kWave;
constexpr int kAlsChunksPerWg = kAlsWaves;      // one chunk per wave of the workgroup
constexpr int kAlsFinishBlock = 1024;           // the long rows' second launch: more threads, fewer partial loads each
constexpr int kAlsFailBadPosition = 1 << 30;
constexpr int kAlsFailBadWeight = 1 << 29;      // (implicit) a weight that is negative or not finite
constexpr int kAlsGramSegment = 512;            // table rows per segment of esr_als_gram (even), one wave each
constexpr int64_t kAlsMaxRows = (int64_t)1 << 30;

struct AlsUnit {       // a row of class 1 or 2
  long long begin;     // its first rating
  int32_t row, len;
};
struct AlsLongRow {    // a row of class 3
  long long begin, first;  // first: its first partial in the workspace
  int32_t row, len;
};
struct AlsChunkUnit {  // a chunk of a class-3 row
  long long begin, slot;
  int32_t len, pad;
};
struct AlsIn {
  const float* other;
  int64_t n_other;
  int rank;
  const int32_t* cols;
  const float* targets;
  float reg;
  int weighted;
  float* out;
  int32_t* failed;
  const float* gram;   // (implicit) Y^T Y [rank, rank]; `targets` holds the weights w_k
};
template <bool HI>
struct AlsAcc {
  als_f32x16 ll, hl, hh;
  float rlo, rhi;
};

__host__ __device__ inline int als_stride(int rank) { return rank | 1; }   // odd: a column of the matrix spans all banks
__host__ __device__ inline int als_slot_floats(int rank) { return rank * als_stride(rank) + kAlsMaxRank; }
static size_t als_lds_bytes(int rank, int slots) { return sizeof(float) * (size_t)slots * als_slot_floats(rank); }

// LDS ops of one wave complete in order; this only stops the compiler moving reads above writes.
__device__ __forceinline__ void als_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the partial of the ratings [begin, begin + len) (len >= 1, at most kAlsChunk), from zero
// IMP: targets are the weights w_k -- the A operand (the row index) is fl32(w_k * y_k), the right-hand side takes fl32(1 + w_k)
template <bool HI, bool IMP>
__device__ __forceinline__ void als_chunk(const AlsIn& in, int64_t begin, int len, AlsAcc<HI>& a, int lane) {
#pragma unroll
  for (int r = 0; r < 16; ++r) a.ll[r] = 0.f, a.hl[r] = 0.f, a.hh[r] = 0.f;
  a.rlo = a.rhi = 0.f;
  const int dim = lane & 31, half = lane >> 5;
  const bool lo_live = dim < in.rank, hi_live = HI && dim + 32 < in.rank;
  const int dlo = lo_live ? dim : 0, dhi = hi_live ? dim + 32 : 0;   // a dead lane reads element 0 and drops it
  bool bad = false, bad_weight = false;
  for (int b0 = 0; b0 < len; b0 += kWave) {
    const int k = b0 + lane;
    int32_t c = -1;
    float d = 0.f;
    if (k < len) {
      c = in.cols[begin + k];
      d = in.targets[begin + k];
      const bool off = c < 0 || (int64_t)c >= in.n_other;
      if (IMP && (!(d >= 0.f) || !(d < INFINITY))) bad_weight = true, c = -1, d = 0.f;
      if (off) bad = true, c = -1, d = 0.f;
    }
    const int left = len - b0;
    const int steps = ((left < kWave ? left : kWave) + 1) >> 1;
    // eight steps at a time, so that their gathers are in flight together; a step past the last rating reads c = -1
    // from a lane at or above len and adds fma(0, 0, acc) = acc
    for (int s0 = 0; s0 < steps; s0 += 8)
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int src = 2 * (s0 + t) + half;   // <= 63: steps <= 32
      const int32_t cs = __shfl(c, src, kWave);
      const float ds = __shfl(d, src, kWave);
      const float* y = in.other + (int64_t)(cs < 0 ? 0 : cs) * in.rank;   // (row 0 exists: n_other >= 1 where a rating does)
      const float vlo = y[dlo];
      const float ylo = (cs >= 0 && lo_live) ? vlo : 0.f;
      const float rs = IMP ? __fadd_rn(1.f, ds) : ds;
      a.ll = __builtin_amdgcn_mfma_f32_32x32x2f32(IMP ? __fmul_rn(ds, ylo) : ylo, ylo, a.ll, 0, 0, 0);
      a.rlo = fmaf(rs, ylo, a.rlo);
      if (HI) {
        const float vhi = y[dhi];
        const float yhi = (cs >= 0 && hi_live) ? vhi : 0.f;
        const float ahi = IMP ? __fmul_rn(ds, yhi) : yhi;
        a.hl = __builtin_amdgcn_mfma_f32_32x32x2f32(ahi, ylo, a.hl, 0, 0, 0);
        a.hh = __builtin_amdgcn_mfma_f32_32x32x2f32(ahi, yhi, a.hh, 0, 0, 0);
        a.rhi = fmaf(rs, yhi, a.rhi);
      }
    }
  }
  if (__any(bad) && lane == 0) atomicOr(in.failed, kAlsFailBadPosition);
  if (IMP && __any(bad_weight) && lane == 0) atomicOr(in.failed, kAlsFailBadWeight);
}

// the partial as a matrix [rank][S] (lower block triangle: rows >= 32 x columns < 32 included, the transposed block not)
// and a right-hand side [rank]
template <bool HI>
__device__ __forceinline__ void als_store_matrix(const AlsAcc<HI>& a, float* __restrict__ A, int S, int n, int lane) {
  const int col = lane & 31, half = lane >> 5;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
    if (row < n && col < n) A[row * S + col] = a.ll[r];
    if (HI) {
      if (row + 32 < n) A[(row + 32) * S + col] = a.hl[r];
      if (row + 32 < n && col + 32 < n) A[(row + 32) * S + col + 32] = a.hh[r];
    }
  }
}

template <bool HI>
__device__ __forceinline__ void als_store_partial(const AlsAcc<HI>& a, float* __restrict__ A, int S, float* __restrict__ rhs,
                                                  int n, int lane) {
  const int col = lane & 31, half = lane >> 5;
  als_store_matrix<HI>(a, A, S, n, lane);
  const float lo = a.rlo + __shfl_xor(a.rlo, 32, kWave);   // even ratings + odd ratings (the same bits in both halves)
  if (half == 0 && col < n) rhs[col] = lo;
  if (HI) {
    const float hi = a.rhi + __shfl_xor(a.rhi, 32, kWave);
    if (half == 0 && col + 32 < n) rhs[col + 32] = hi;
  }
}

// whether als_store_partial writes cell (row, col) of a partial laid out as rows of a matrix followed by the right-hand side
// (row >= n: the right-hand side): everything but the padding column and the block (rows < 32, columns >= 32), which is the
// transpose of the block below the diagonal and is never computed -- the sums of the partials skip what nobody wrote
__device__ __forceinline__ bool als_cell_written(int row, int col, int n) {
  return row >= n || (col < n && !(row < 32 && col >= 32));
}

// ONE wave: (IMP: G on the lower triangle, then) lam on the diagonal, Cholesky, both solves; writes the row or counts the
// failure
template <bool IMP>
__device__ __forceinline__ void als_finish_row(const AlsIn& in, float* __restrict__ A, const float* __restrict__ rhs, int n,
                                               int S, int len, float* __restrict__ out, int lane) {
  const float lam = in.weighted ? in.reg * (float)len : in.reg;
  const bool live = lane < n;
  if (IMP) {   // the Cholesky reads the lower triangle only
    for (int e = lane; e < n * n; e += kWave) {
      const int row = e / n, col = e - row * n;
      if (col <= row) A[row * S + col] = A[row * S + col] + in.gram[e];
    }
    als_wave_sync();
  }
  if (live) A[lane * S + lane] = A[lane * S + lane] + lam;
  als_wave_sync();
  bool ok = true;
  for (int j = 0; j < n; ++j) {   // (j and ok: the same in every lane)
    float s = 0.f;
    if (live && lane >= j) {
      s = A[lane * S + j];
      for (int k = 0; k < j; ++k) s = fmaf(-A[lane * S + k], A[j * S + k], s);
    }
    const float piv = __shfl(s, j, kWave);
    if (!(piv > 0.f) || !(piv < INFINITY)) {
      ok = false;
      break;
    }
    // the correctly rounded square root: sqrtf is (v_sqrt_f32 and a correction); __fsqrt_rn is the bare 1-ulp v_sqrt_f32
    // here, which test_gpu_als_exact.py::test_exact_rows_bit_for_bit tells apart
    const float dj = sqrtf(piv);
    if (lane == j) A[j * S + j] = dj;
    else if (live && lane > j) A[lane * S + j] = __fdiv_rn(s, dj);
    als_wave_sync();
  }
  float b = live ? rhs[lane] : 0.f;
  if (ok) {
    for (int j = 0; j < n; ++j) {           // L z = b
      const float z = __fdiv_rn(__shfl(b, j, kWave), A[j * S + j]);
      if (lane == j) b = z;
      else if (live && lane > j) b = fmaf(-A[lane * S + j], z, b);
    }
    for (int j = n - 1; j >= 0; --j) {      // L^T x = z
      const float x = __fdiv_rn(__shfl(b, j, kWave), A[j * S + j]);
      if (lane == j) b = x;
      else if (lane < j) b = fmaf(-A[j * S + lane], x, b);
    }
    ok = !__any(live && !(fabsf(b) < INFINITY));
  }
  if (ok) {
    if (live) out[lane] = b;
  } else if (lane == 0) {
    atomicAdd(in.failed, 1);
  }
}

// ---- class 1: a wave per row ----------------------------------------------------------------------------------------------
template <bool HI, bool IMP>
__global__ __launch_bounds__(kBlock) void als_wave_rows_kernel(AlsIn in, const AlsUnit* __restrict__ units, int64_t n_units) {
  extern __shared__ __attribute__((aligned(16))) float als_lds[];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const int n = in.rank, S = als_stride(n);
  float* A = als_lds + w * als_slot_floats(n);
  float* rhs = A + n * S;
  for (int64_t u = (int64_t)blockIdx.x * kAlsWaves + w; u < n_units; u += (int64_t)gridDim.x * kAlsWaves) {
    const AlsUnit un = units[u];
    float* out = in.out + (int64_t)un.row * n;
    if (un.len <= 0) {   // a row without ratings: the zero vector
      if (lane < n) out[lane] = 0.f;
      continue;
    }
    AlsAcc<HI> a;
    als_chunk<HI, IMP>(in, un.begin, un.len < kAlsChunk ? un.len : kAlsChunk, a, lane);
    als_wave_sync();
    als_store_partial<HI>(a, A, S, rhs, n, lane);
    als_wave_sync();
    als_finish_row<IMP>(in, A, rhs, n, S, un.len, out, lane);
  }
}

// ---- class 2: a workgroup per row, a chunk per wave -------------------------------------------------------------------------
template <bool HI, bool IMP>
__global__ __launch_bounds__(kBlock) void als_group_rows_kernel(AlsIn in, const AlsUnit* __restrict__ units, int64_t n_units) {
  extern __shared__ __attribute__((aligned(16))) float als_lds[];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const int n = in.rank, S = als_stride(n), slot = als_slot_floats(n), used = n * S + n;
  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {   // (u, un, nch: the same in all threads)
    const AlsUnit un = units[u];
    int nch = (un.len + kAlsChunk - 1) / kAlsChunk;
    nch = nch < 1 ? 1 : (nch > kAlsChunksPerWg ? kAlsChunksPerWg : nch);
    __syncthreads();   // the previous row's solve is done with slot 0
    if (w < nch) {
      const int off = w * kAlsChunk, left = un.len - off;
      AlsAcc<HI> a;
      als_chunk<HI, IMP>(in, un.begin + off, left < kAlsChunk ? left : kAlsChunk, a, lane);
      als_store_partial<HI>(a, als_lds + w * slot, S, als_lds + w * slot + n * S, n, lane);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < used; e += kBlock) {   // ascending chunk order
      if (!als_cell_written(e / S, e % S, n)) continue;
      float s = als_lds[e];
      for (int c = 1; c < nch; ++c) s = s + als_lds[c * slot + e];
      als_lds[e] = s;
    }
    __syncthreads();
    if (w == 0) als_finish_row<IMP>(in, als_lds, als_lds + n * S, n, S, un.len, in.out + (int64_t)un.row * n, lane);
  }
}

// ---- class 3: a wave per chunk into the workspace, then a workgroup per row ---------------------------------------------------
template <bool HI, bool IMP>
__global__ __launch_bounds__(kBlock) void als_chunk_partials_kernel(AlsIn in, const AlsChunkUnit* __restrict__ units,
                                                                    int64_t n_units, float* __restrict__ partials) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const int n = in.rank, P = n * n + n;
  for (int64_t u = (int64_t)blockIdx.x * kAlsWaves + w; u < n_units; u += (int64_t)gridDim.x * kAlsWaves) {
    const AlsChunkUnit un = units[u];
    if (un.len <= 0) continue;
    AlsAcc<HI> a;
    als_chunk<HI, IMP>(in, un.begin, un.len < kAlsChunk ? un.len : kAlsChunk, a, lane);
    float* dst = partials + un.slot * P;
    als_store_partial<HI>(a, dst, n, dst + n * n, n, lane);
  }
}

template <bool IMP>
__global__ __launch_bounds__(kAlsFinishBlock) void als_long_rows_kernel(AlsIn in, const AlsLongRow* __restrict__ rows,
                                                                        int64_t n_rows, const float* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float als_lds[];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const int n = in.rank, S = als_stride(n), P = n * n + n;
  for (int64_t u = blockIdx.x; u < n_rows; u += gridDim.x) {
    const AlsLongRow un = rows[u];
    const int64_t nch = ((int64_t)un.len + kAlsChunk - 1) / kAlsChunk;
    const float* base = partials + un.first * P;
    __syncthreads();
    for (int e = threadIdx.x; e < P; e += kAlsFinishBlock) {
      if (!als_cell_written(e / n, e % n, n)) continue;
      float s = base[e];
      int64_t c = 1;
      for (; c + 4 <= nch; c += 4) {   // four loads in flight, added strictly in order
        const float t0 = base[c * P + e], t1 = base[(c + 1) * P + e], t2 = base[(c + 2) * P + e], t3 = base[(c + 3) * P + e];
        s = (((s + t0) + t1) + t2) + t3;
      }
      for (; c < nch; ++c) s = s + base[c * P + e];
      if (e < n * n) als_lds[(e / n) * S + e % n] = s;
      else als_lds[n * S + (e - n * n)] = s;
    }
    __syncthreads();
    if (w == 0) als_finish_row<IMP>(in, als_lds, als_lds + n * S, n, S, un.len, in.out + (int64_t)un.row * n, lane);
  }
}

// ---- the whole table's Gram matrix: a wave per segment into the workspace, then an fp64 sum per entry ------------------------------
template <bool HI>
__global__ __launch_bounds__(kBlock) void als_gram_segments_kernel(const float* __restrict__ table, int64_t n, int rank,
                                                                   int64_t n_seg, float* __restrict__ partials) {
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const int dim = lane & 31, half = lane >> 5;
  const bool lo_live = dim < rank, hi_live = HI && dim + 32 < rank;
  const int dlo = lo_live ? dim : 0, dhi = hi_live ? dim + 32 : 0;   // a dead lane reads element 0 and drops it
  for (int64_t s = (int64_t)blockIdx.x * kAlsWaves + w; s < n_seg; s += (int64_t)gridDim.x * kAlsWaves) {
    const int64_t r0 = s * kAlsGramSegment;   // (< n: n_seg = ceil(n / kAlsGramSegment))
    const int64_t left = n - r0;
    const int len = (int)(left < kAlsGramSegment ? left : kAlsGramSegment);
    AlsAcc<HI> a;
#pragma unroll
    for (int r = 0; r < 16; ++r) a.ll[r] = 0.f, a.hl[r] = 0.f, a.hh[r] = 0.f;
    const int steps = (len + 1) >> 1;
    // eight steps at a time, as als_chunk; a row at or above len is read as row r0 and dropped: fma(0, 0, acc) = acc
    for (int s0 = 0; s0 < steps; s0 += 8)
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int k = 2 * (s0 + t) + half;
      const bool in_seg = k < len;
      const float* y = table + (r0 + (in_seg ? k : 0)) * rank;
      const float vlo = y[dlo];
      const float ylo = (in_seg && lo_live) ? vlo : 0.f;
      a.ll = __builtin_amdgcn_mfma_f32_32x32x2f32(ylo, ylo, a.ll, 0, 0, 0);
      if (HI) {
        const float vhi = y[dhi];
        const float yhi = (in_seg && hi_live) ? vhi : 0.f;
        a.hl = __builtin_amdgcn_mfma_f32_32x32x2f32(yhi, ylo, a.hl, 0, 0, 0);
        a.hh = __builtin_amdgcn_mfma_f32_32x32x2f32(yhi, yhi, a.hh, 0, 0, 0);
      }
    }
    als_store_matrix<HI>(a, partials + s * rank * rank, rank, rank, lane);
  }
}

// entry (i, j), i >= j: the segment partials in ascending order in fp64, rounded once; the mirror gets the same bits
__global__ __launch_bounds__(kBlock) void als_gram_sum_kernel(const float* __restrict__ partials, int64_t n_seg, int rank,
                                                              float* __restrict__ out) {
  const int P = rank * rank;
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < P; e += gridDim.x * kBlock) {
    const int i = e / rank, j = e - i * rank;
    if (j > i) continue;
    double acc = 0.0;
    int64_t s = 0;
    for (; s + 8 <= n_seg; s += 8) {   // eight loads in flight, added strictly in order
      float t[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) t[q] = partials[(s + q) * P + e];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc = acc + (double)t[q];
    }
    for (; s < n_seg; ++s) acc = acc + (double)partials[s * P + e];
    const float g = (float)acc;
    out[e] = g;
    out[j * rank + i] = g;
  }
}

// ---- predict ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void als_predict_kernel(const float* __restrict__ uf, int64_t nu, const float* __restrict__ vf,
                                                            int64_t ni, int rank, const int32_t* __restrict__ upos,
                                                            const int32_t* __restrict__ ipos, const double* __restrict__ offset,
                                                            const float* __restrict__ targets, int64_t nq,
                                                            float* __restrict__ out) {
  for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (int64_t)gridDim.x * kBlock) {
    const int32_t u = upos[q], i = ipos[q];
    if (u < 0 || (int64_t)u >= nu || i < 0 || (int64_t)i >= ni) {
      out[q] = __uint_as_float(0x7FC00000u);
      continue;
    }
    const float* x = uf + (int64_t)u * rank;
    const float* y = vf + (int64_t)i * rank;
    double acc = 0.0;
    for (int d = 0; d < rank; ++d) acc = acc + (double)x[d] * (double)y[d];   // every product exact in a double
    const double v = offset ? offset[u] + acc : acc;
    out[q] = targets ? (float)((double)targets[q] - v) : (float)v;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct AlsWs {
  AlsUnit* units;
  AlsLongRow* long_rows;
  AlsChunkUnit* chunks;
  float* partials;
  int64_t max_long, max_chunks;
};
static size_t als_layout(int64_t n_rows, int64_t nnz, int rank, char* base, AlsWs* ws) {
  n_rows = std::max<int64_t>(n_rows, 0);
  nnz = std::max<int64_t>(nnz, 0);
  rank = std::min(std::max(rank, 1), kAlsMaxRank);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align_up(bytes, 256);
    return p;
  };
  AlsWs w;
  // a long row has more than kAlsChunk * kAlsChunksPerWg ratings; its chunks: ceil(len / kAlsChunk) <= len / kAlsChunk + 1
  w.max_long = std::min<int64_t>(n_rows, nnz / ((int64_t)kAlsChunk * kAlsChunksPerWg + 1));
  w.max_chunks = w.max_long ? nnz / kAlsChunk + w.max_long : 0;
  w.units = (AlsUnit*)take(sizeof(AlsUnit) * (size_t)n_rows);
  w.long_rows = (AlsLongRow*)take(sizeof(AlsLongRow) * (size_t)w.max_long);
  w.chunks = (AlsChunkUnit*)take(sizeof(AlsChunkUnit) * (size_t)w.max_chunks);
  w.partials = (float*)take(sizeof(float) * (size_t)w.max_chunks * (size_t)(rank * rank + rank));
  if (ws) *ws = w;
  return off + 256;
}

static int als_raise_lds(const char* who, const void* fn, size_t bytes) {
  if (bytes <= 65536) return ESR_OK;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
    set_error("%s: cannot raise the LDS limit to %zu bytes", who, bytes);
    return ESR_ELAUNCH;
  }
  return ESR_OK;
}

static bool als_finite(float x) { return x == x && x - x == 0.f; }

static int64_t als_gram_segments(int64_t n) { return n > 0 ? cdiv(n, kAlsGramSegment) : 0; }
static size_t als_gram_layout(int64_t n, int rank) {
  rank = std::min(std::max(rank, 1), kAlsMaxRank);
  return align_up(sizeof(float) * (size_t)als_gram_segments(n) * (size_t)(rank * rank), 256) + 256;
}

// the half-sweep of esr_als_solve_rows (targets) and of esr_als_solve_rows_implicit (IMP: `targets` are the weights, gram is
// Y^T Y): one argument check, one row plan, one launch sequence
template <bool IMP>
static int als_solve_rows_impl(const char* fn, const float* other_factors, int64_t n_other, int rank, const int64_t* row_offsets,
                               const int32_t* cols, const float* targets, const float* gram, int64_t row_begin, int64_t row_end,
                               float reg, int weighted, float* out_factors, int32_t* failed, void* workspace,
                               size_t workspace_bytes, esr_stream_t stream) {
  TraceScope trace_scope_(fn);
  ESR_REQUIRE(rank >= 1 && rank <= kAlsMaxRank, "%s: rank=%d not in [1, %d]", fn, rank, kAlsMaxRank);
  ESR_REQUIRE(n_other >= 0 && n_other <= (int64_t)INT32_MAX, "%s: bad size n_other=%lld", fn, (long long)n_other);
  ESR_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end - row_begin <= kAlsMaxRows && row_end <= (int64_t)INT32_MAX,
              "%s: row range [%lld, %lld) out of order (or longer than 2^30 rows)", fn, (long long)row_begin,
              (long long)row_end);
  ESR_REQUIRE(als_finite(reg) && reg > 0.f, "%s: reg=%g must be finite and positive", fn, (double)reg);
  ESR_REQUIRE(weighted == 0 || weighted == 1, "%s: weighted=%d is not 0 or 1", fn, weighted);
  ESR_REQUIRE(row_offsets && out_factors && failed && (!IMP || gram), "%s: null pointer", fn);
  ESR_REQUIRE(((uintptr_t)row_offsets & 7) == 0 && ((uintptr_t)out_factors & 3) == 0 && ((uintptr_t)failed & 3) == 0 &&
                  ((uintptr_t)other_factors & 3) == 0 && ((uintptr_t)cols & 3) == 0 && ((uintptr_t)targets & 3) == 0,
              "%s: misaligned pointer", fn);
  ESR_REQUIRE(((uintptr_t)gram & 3) == 0, "%s: misaligned pointer (gram)", fn);
  {  // the rows written against the table read
    const uintptr_t o0 = (uintptr_t)(out_factors + row_begin * rank), o1 = (uintptr_t)(out_factors + row_end * rank);
    const uintptr_t y0 = (uintptr_t)other_factors, y1 = (uintptr_t)(other_factors + n_other * rank);
    ESR_REQUIRE(out_factors != other_factors && !(other_factors && o0 < y1 && y0 < o1),
                "%s: out_factors aliases other_factors", fn);
    const uintptr_t g0 = (uintptr_t)gram, g1 = g0 + sizeof(float) * (size_t)(rank * rank);
    ESR_REQUIRE(!IMP || (out_factors != gram && !(o0 < g1 && g0 < o1)), "%s: out_factors aliases gram", fn);
  }
  const int64_t n_rows = row_end - row_begin;
  if (n_rows == 0) return ESR_OK;
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < als_layout(n_rows, 0, rank, nullptr, nullptr)) {
    set_error("%s: workspace %zu bytes < %zu required (or null, or misaligned)", fn, workspace_bytes,
              als_layout(n_rows, 0, rank, nullptr, nullptr));
    return ESR_EWORKSPACE;
  }
  // the row offsets are HOST memory: the class lists are made here
  const int64_t first = row_offsets[row_begin], last = row_offsets[row_end];
  ESR_REQUIRE(first >= 0 && last >= first, "%s: row offsets %lld .. %lld are not ascending from >= 0", fn,
              (long long)first, (long long)last);
  const int64_t nnz = last - first;
  for (int64_t r = row_begin; r < row_end; ++r) {
    const int64_t len = row_offsets[r + 1] - row_offsets[r];
    ESR_REQUIRE(len >= 0 && len <= (int64_t)INT32_MAX && row_offsets[r + 1] <= last,
                "%s: row offsets are not ascending at row %lld (or a row above 2^31 - 1 ratings)", fn, (long long)r);
  }
  ESR_REQUIRE(nnz == 0 || (other_factors && cols && targets && n_other >= 1),
              "%s: null pointer (ratings or other_factors; or n_other=0 with ratings)", fn);
  const size_t need = als_layout(n_rows, nnz, rank, nullptr, nullptr);
  if (workspace_bytes < need) {
    set_error("%s: workspace %zu bytes < %zu required", fn, workspace_bytes, need);
    return ESR_EWORKSPACE;
  }
  AlsWs ws;
  als_layout(n_rows, nnz, rank, (char*)workspace, &ws);
  std::vector<AlsUnit> wave_rows, group_rows;
  std::vector<AlsLongRow> long_rows;
  std::vector<AlsChunkUnit> chunks;
  for (int64_t r = row_begin; r < row_end; ++r) {
    const int64_t a = row_offsets[r], len = row_offsets[r + 1] - a;
    if (len <= kAlsChunk) wave_rows.push_back(AlsUnit{a, (int32_t)r, (int32_t)len});
    else if (len <= (int64_t)kAlsChunk * kAlsChunksPerWg) group_rows.push_back(AlsUnit{a, (int32_t)r, (int32_t)len});
    else {
      long_rows.push_back(AlsLongRow{a, (long long)chunks.size(), (int32_t)r, (int32_t)len});
      for (int64_t o = 0; o < len; o += kAlsChunk)
        chunks.push_back(AlsChunkUnit{a + o, (long long)chunks.size(), (int32_t)std::min<int64_t>(kAlsChunk, len - o), 0});
    }
  }
  if ((int64_t)long_rows.size() > ws.max_long || (int64_t)chunks.size() > ws.max_chunks) {  // (the layout's bound: never)
    set_error("%s: internal: the long-row plan exceeds its bound", fn);
    return ESR_EINVAL;
  }
  hipStream_t st = as_stream(stream);
  const size_t n1 = wave_rows.size(), n2 = group_rows.size(), n3 = long_rows.size(), nc = chunks.size();
  bool copied = true;
  if (n1) copied &= hipMemcpyAsync(ws.units, wave_rows.data(), sizeof(AlsUnit) * n1, hipMemcpyHostToDevice, st) == hipSuccess;
  if (n2) copied &= hipMemcpyAsync(ws.units + n1, group_rows.data(), sizeof(AlsUnit) * n2, hipMemcpyHostToDevice, st) == hipSuccess;
  if (n3) copied &= hipMemcpyAsync(ws.long_rows, long_rows.data(), sizeof(AlsLongRow) * n3, hipMemcpyHostToDevice, st) == hipSuccess;
  if (nc) copied &= hipMemcpyAsync(ws.chunks, chunks.data(), sizeof(AlsChunkUnit) * nc, hipMemcpyHostToDevice, st) == hipSuccess;
  // the lists are pageable host memory that dies with this call: the copies are complete before it goes on
  if (!copied || hipStreamSynchronize(st) != hipSuccess) {
    if (check_launch(fn) == ESR_OK) set_error("%s: the copy of the row lists failed", fn);
    return ESR_ELAUNCH;
  }
  const bool hi = rank > 32;
  const size_t lds4 = als_lds_bytes(rank, kAlsWaves), lds1 = als_lds_bytes(rank, 1);
  const auto wave_rows_kernel = hi ? als_wave_rows_kernel<true, IMP> : als_wave_rows_kernel<false, IMP>;
  const auto group_rows_kernel = hi ? als_group_rows_kernel<true, IMP> : als_group_rows_kernel<false, IMP>;
  const auto chunk_partials_kernel = hi ? als_chunk_partials_kernel<true, IMP> : als_chunk_partials_kernel<false, IMP>;
  // above the 64 KiB a kernel gets unasked (rank 64): raised on every such call, for the device the call runs on -- no flag
  // that another device or another thread could find set
  if (n1 && als_raise_lds(fn, (const void*)wave_rows_kernel, lds4)) return ESR_ELAUNCH;
  if (n2 && als_raise_lds(fn, (const void*)group_rows_kernel, lds4)) return ESR_ELAUNCH;
  const AlsIn in{other_factors, n_other, rank, cols, targets, reg, weighted, out_factors, failed, gram};
  if (n1) {
    const int grid = (int)std::min<int64_t>(kMaxGrid, cdiv((int64_t)n1, kAlsWaves));
    ESR_KT(IMP ? "als_wave_rows_implicit" : "als_wave_rows", st,
           hipLaunchKernelGGL(wave_rows_kernel, dim3(grid), dim3(kBlock), lds4, st, in, (const AlsUnit*)ws.units, (int64_t)n1));
  }
  if (n2) {
    const int grid = (int)std::min<int64_t>(kMaxGrid, (int64_t)n2);
    ESR_KT(IMP ? "als_group_rows_implicit" : "als_group_rows", st,
           hipLaunchKernelGGL(group_rows_kernel, dim3(grid), dim3(kBlock), lds4, st, in, (const AlsUnit*)(ws.units + n1),
                              (int64_t)n2));
  }
  if (n3) {
    const int grid = (int)std::min<int64_t>(4 * kMaxGrid, cdiv((int64_t)nc, kAlsWaves));
    ESR_KT(IMP ? "als_chunk_partials_implicit" : "als_chunk_partials", st,
           hipLaunchKernelGGL(chunk_partials_kernel, dim3(grid), dim3(kBlock), 0, st, in, (const AlsChunkUnit*)ws.chunks,
                              (int64_t)nc, ws.partials));
    ESR_KT(IMP ? "als_long_rows_implicit" : "als_long_rows", st,
           hipLaunchKernelGGL(als_long_rows_kernel<IMP>, dim3((int)std::min<int64_t>(kMaxGrid, (int64_t)n3)),
                              dim3(kAlsFinishBlock), lds1, st, in, (const AlsLongRow*)ws.long_rows, (int64_t)n3,
                              (const float*)ws.partials));
  }
  return check_launch(fn);
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_als_max_rank(void) { return kAlsMaxRank; }

int esr_als_predict_max_rank(void) { return kAlsPredictMaxRank; }

int esr_als_geometry(int* chunk, int* chunks_per_workgroup) {
  ESR_REQUIRE(chunk && chunks_per_workgroup, "esr_als_geometry: null pointer");
  *chunk = kAlsChunk;
  *chunks_per_workgroup = kAlsChunksPerWg;
  return ESR_OK;
}

size_t esr_als_solve_workspace_bytes(int64_t n_rows, int64_t nnz, int rank) {
  return als_layout(n_rows, nnz, rank, nullptr, nullptr);
}

int esr_als_solve_rows(const float* other_factors, int64_t n_other, int rank, const int64_t* row_offsets, const int32_t* cols,
                       const float* targets, int64_t row_begin, int64_t row_end, float reg, int weighted, float* out_factors,
                       int32_t* failed, void* workspace, size_t workspace_bytes, esr_stream_t stream) {
  return als_solve_rows_impl<false>("esr_als_solve_rows", other_factors, n_other, rank, row_offsets, cols, targets, nullptr,
                                    row_begin, row_end, reg, weighted, out_factors, failed, workspace, workspace_bytes, stream);
}

int esr_als_solve_rows_implicit(const float* other_factors, int64_t n_other, int rank, const float* gram,
                                const int64_t* row_offsets, const int32_t* cols, const float* weights, int64_t row_begin,
                                int64_t row_end, float reg, int weighted, float* out_factors, int32_t* failed, void* workspace,
                                size_t workspace_bytes, esr_stream_t stream) {
  return als_solve_rows_impl<true>("esr_als_solve_rows_implicit", other_factors, n_other, rank, row_offsets, cols, weights, gram,
                                   row_begin, row_end, reg, weighted, out_factors, failed, workspace, workspace_bytes, stream);
}

int esr_als_gram_geometry(int* segment) {
  ESR_REQUIRE(segment, "esr_als_gram_geometry: null pointer");
  *segment = kAlsGramSegment;
  return ESR_OK;
}

size_t esr_als_gram_workspace_bytes(int64_t n, int rank) { return als_gram_layout(n, rank); }

int esr_als_gram(const float* factors, int64_t n, int rank, float* out_gram, void* workspace, size_t workspace_bytes,
                 esr_stream_t stream) {
  TraceScope trace_scope_("esr_als_gram");
  ESR_REQUIRE(rank >= 1 && rank <= kAlsMaxRank, "esr_als_gram: rank=%d not in [1, %d]", rank, kAlsMaxRank);
  ESR_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, "esr_als_gram: bad size n=%lld", (long long)n);
  ESR_REQUIRE(out_gram && (n == 0 || factors), "esr_als_gram: null pointer");
  ESR_REQUIRE(((uintptr_t)factors & 3) == 0 && ((uintptr_t)out_gram & 3) == 0, "esr_als_gram: misaligned pointer");
  {
    const uintptr_t o0 = (uintptr_t)out_gram, o1 = (uintptr_t)(out_gram + rank * rank);
    const uintptr_t y0 = (uintptr_t)factors, y1 = (uintptr_t)(factors + n * rank);
    ESR_REQUIRE(out_gram != factors && !(factors && o0 < y1 && y0 < o1), "esr_als_gram: out_gram aliases factors");
  }
  const size_t need = als_gram_layout(n, rank);
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < need) {
    set_error("esr_als_gram: workspace %zu bytes < %zu required (or null, or misaligned)", workspace_bytes, need);
    return ESR_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  const int64_t n_seg = als_gram_segments(n);
  float* partials = (float*)workspace;
  if (n_seg) {
    const int grid = (int)std::min<int64_t>(4 * kMaxGrid, cdiv(n_seg, kAlsWaves));
    const auto segments_kernel = rank > 32 ? als_gram_segments_kernel<true> : als_gram_segments_kernel<false>;
    ESR_KT("als_gram_segments", st,
           hipLaunchKernelGGL(segments_kernel, dim3(grid), dim3(kBlock), 0, st, factors, n, rank, n_seg, partials));
  }
  ESR_KT("als_gram_sum", st,
         hipLaunchKernelGGL(als_gram_sum_kernel, dim3((int)cdiv(rank * rank, kBlock)), dim3(kBlock), 0, st,
                            (const float*)partials, n_seg, rank, out_gram));
  return check_launch("esr_als_gram");
}

int esr_als_predict(const float* user_factors, int64_t nu, const float* item_factors, int64_t ni, int rank,
                    const int32_t* user_pos, const int32_t* item_pos, const double* offset, const float* targets, int64_t nq,
                    float* out, esr_stream_t stream) {
  TraceScope trace_scope_("esr_als_predict");
  ESR_REQUIRE(rank >= 1 && rank <= kAlsPredictMaxRank, "esr_als_predict: rank=%d not in [1, %d]", rank, kAlsPredictMaxRank);
  ESR_REQUIRE(nu >= 0 && nu <= (int64_t)INT32_MAX && ni >= 0 && ni <= (int64_t)INT32_MAX && nq >= 0,
              "esr_als_predict: bad sizes nu=%lld ni=%lld nq=%lld", (long long)nu, (long long)ni, (long long)nq);
  if (nq == 0) return ESR_OK;
  ESR_REQUIRE(user_pos && item_pos && out, "esr_als_predict: null pointer");
  ESR_REQUIRE((nu == 0 || user_factors) && (ni == 0 || item_factors), "esr_als_predict: null pointer (factors)");
  ESR_REQUIRE(((uintptr_t)user_factors & 3) == 0 && ((uintptr_t)item_factors & 3) == 0 && ((uintptr_t)user_pos & 3) == 0 &&
                  ((uintptr_t)item_pos & 3) == 0 && ((uintptr_t)offset & 7) == 0 && ((uintptr_t)targets & 3) == 0 &&
                  ((uintptr_t)out & 3) == 0,
              "esr_als_predict: misaligned pointer");
  hipStream_t st = as_stream(stream);
  ESR_KT("als_predict", st,
         hipLaunchKernelGGL(als_predict_kernel, dim3(grid_for_groups(nq, 1)), dim3(kBlock), 0, st, user_factors, nu, item_factors,
                            ni, rank, user_pos, item_pos, offset, targets, nq, out));
  return check_launch("esr_als_predict");
}

}  // extern "C"
