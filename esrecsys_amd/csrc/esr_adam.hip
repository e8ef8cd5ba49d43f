// Lazy optax.adam: the catch-up of the rows a step is about to read (alone, or fused with the owner-side gather of a
// row-sharded lookup) and the flush of every row (esr_adam.h has the arithmetic and the exactness contract; the step
// itself is esr_optim.hip's kAdamStepLazy segment update).
#include "esr_adam.h"

#include <algorithm>

namespace esr {

struct AdamCatchupTables {  // up to two tables, caught up by one launch (blockIdx.y = the table), each with its own width
  float* table[2];
  float* mu[2];
  float* nu[2];
  int32_t* last[2];
  const int32_t* ids[2];
  int64_t V[2];
  int64_t n[2];
  int D[2];
  int G[2];
  int modulus[2];
};

// bring the rows ids[i] % modulus (modulus 0: ids[i]) up to step ax.now - 1 and stamp them so: the group whose atomicMax on
// last[row] returns an older step owns the row, every other occurrence of it skips.  Ids outside [0, V) are skipped.
template <int VEC, int NCH>
__global__ __launch_bounds__(kBlock) void adam_catchup_kernel(AdamCatchupTables ct, AdamLazyArgs ax) {
  const int y = blockIdx.y;
  float* __restrict__ table = y ? ct.table[1] : ct.table[0];
  float* __restrict__ mu = y ? ct.mu[1] : ct.mu[0];
  float* __restrict__ nu = y ? ct.nu[1] : ct.nu[0];
  int32_t* __restrict__ last = y ? ct.last[1] : ct.last[0];
  const int32_t* __restrict__ ids = y ? ct.ids[1] : ct.ids[0];
  const int64_t V = y ? ct.V[1] : ct.V[0];
  const int64_t n = y ? ct.n[1] : ct.n[0];
  const int D = y ? ct.D[1] : ct.D[0];
  const int G = y ? ct.G[1] : ct.G[0];
  const int modulus = y ? ct.modulus[1] : ct.modulus[0];
  const int lig = threadIdx.x & (G - 1);
  const int64_t gpb = kBlock / G;
  const int nvec = D / VEC;
  const int target = ax.now - 1;
  for (int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x / G; i < n; i += (int64_t)gridDim.x * gpb) {
    const int64_t row = modulus > 0 ? (int64_t)ids[i] % modulus : (int64_t)ids[i];
    if (row < 0 || row >= V) continue;
    int old = 0;
    if (lig == 0) old = atomicMax(&last[row], target);
    old = __shfl(old, (threadIdx.x & 63) & ~(G - 1), kWave);
    if (old >= target) continue;
    RowRegs<VEC, NCH> w, a, b;
    row_load(w, table + row * D, lig, G, nvec);
    row_load(a, mu + row * D, lig, G, nvec);
    row_load(b, nu + row * D, lig, G, nvec);
    adam_catchup(w, a, b, old, target, ax, lig, G);
    row_store(w, table + row * D, lig, G, nvec);
    row_store(a, mu + row * D, lig, G, nvec);
    row_store(b, nu + row * D, lig, G, nvec);
  }
}

// every row up to step ax.now (before an eval, a checkpoint, a dense step, or anybody reading the plain tables)
template <int VEC, int NCH>
__global__ __launch_bounds__(kBlock) void adam_flush_kernel(float* __restrict__ table, float* __restrict__ mu,
                                                           float* __restrict__ nu, int32_t* __restrict__ last, int64_t V,
                                                           int D, int G, AdamLazyArgs ax) {
  const int lig = threadIdx.x & (G - 1);
  const int64_t gpb = kBlock / G;
  const int nvec = D / VEC;
  for (int64_t row = (int64_t)blockIdx.x * gpb + threadIdx.x / G; row < V; row += (int64_t)gridDim.x * gpb) {
    const int t0 = last[row];
    if (t0 >= ax.now) continue;
    RowRegs<VEC, NCH> w, a, b;
    row_load(w, table + row * D, lig, G, nvec);
    row_load(a, mu + row * D, lig, G, nvec);
    row_load(b, nu + row * D, lig, G, nvec);
    adam_catchup(w, a, b, t0, ax.now, ax, lig, G);
    row_store(w, table + row * D, lig, G, nvec);
    row_store(a, mu + row * D, lig, G, nvec);
    row_store(b, nu + row * D, lig, G, nvec);
    if (lig == 0) last[row] = ax.now;
  }
}

// The owner side of a row-sharded lookup under lazy Adam: the sorted rows asked of this rank (virtual local rows of up to
// two same-width tables at offsets off[]), each brought up to step ax.now - 1 and served.  One row group per RUN of equal
// rows (the group at the run's first position owns it; runs are distinct, so no atomics): a row with last < now - 1 is
// caught up and stored back (p, mu, nu, last), then written to served[perm[j]] for the first G positions j of the run (their
// perm entries loaded by the group at once).  A longer run's other positions -- a Zipf batch asks for its top rows thousands
// of times, which one group would walk serially -- are served by adam_serve_tail_kernel, launched behind this kernel: a
// copy of the caught-up row.  served == nullptr: catch up only (the replicated steps).  Rows outside [0, off[nt]) are
// skipped.
struct AdamServeTables {
  float* table[2];
  float* mu[2];
  float* nu[2];
  int32_t* last[2];
  int64_t off[3];
  int nt;
};

template <int VEC, int NCH>
__global__ __launch_bounds__(kBlock) void adam_catchup_gather_kernel(AdamServeTables at, const int32_t* __restrict__ sorted,
                                                                    const int32_t* __restrict__ perm, int64_t n,
                                                                    float* __restrict__ served, int D, int G,
                                                                    AdamLazyArgs ax) {
  const int lig = threadIdx.x & (G - 1);
  const int64_t gpb = kBlock / G;
  const int nvec = D / VEC;
  const int target = ax.now - 1;
  const int64_t end = at.off[at.nt];
  for (int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x / G; i < n; i += (int64_t)gridDim.x * gpb) {
    const int64_t vid = sorted[i];
    if (i > 0 && sorted[i - 1] == vid) continue;  // not the head of its run
    if (vid < 0 || vid >= end) continue;
    const int t = (at.nt > 1 && vid >= at.off[1]) ? 1 : 0;
    float* __restrict__ table = t ? at.table[1] : at.table[0];
    const int64_t row = vid - (t ? at.off[1] : at.off[0]);
    RowRegs<VEC, NCH> w;
    row_load(w, table + row * D, lig, G, nvec);
    int32_t* __restrict__ last = t ? at.last[1] : at.last[0];
    const int t0 = last[row];
    if (t0 < target) {  // (the same row for every lane of the group: adam_catchup's group sums see every lane)
      float* __restrict__ mu = t ? at.mu[1] : at.mu[0];
      float* __restrict__ nu = t ? at.nu[1] : at.nu[0];
      RowRegs<VEC, NCH> a, b;
      row_load(a, mu + row * D, lig, G, nvec);
      row_load(b, nu + row * D, lig, G, nvec);
      adam_catchup(w, a, b, t0, target, ax, lig, G);
      row_store(w, table + row * D, lig, G, nvec);
      row_store(a, mu + row * D, lig, G, nvec);
      row_store(b, nu + row * D, lig, G, nvec);
      if (lig == 0) last[row] = target;
    }
    if (served == nullptr) continue;
    const int64_t j = i + lig;
    const int pj = (j < n && sorted[j] == vid) ? perm[j] : -1;  // (sorted: the run's positions come first)
    const int base = (threadIdx.x & (kWave - 1)) & ~(G - 1);
    for (int c = 0; c < G; ++c) {
      const int pc = __shfl(pj, base + c, kWave);
      if (pc < 0) break;
      row_store(w, served + (int64_t)pc * D, lig, G, nvec);
    }
  }
}

// the positions of a run beyond its first G (i >= G with sorted[i - G] == sorted[i]): the row, caught up by
// adam_catchup_gather_kernel, copied to served[perm[i]]
template <int VEC, int NCH>
__global__ __launch_bounds__(kBlock) void adam_serve_tail_kernel(AdamServeTables at, const int32_t* __restrict__ sorted,
                                                                const int32_t* __restrict__ perm, int64_t n,
                                                                float* __restrict__ served, int D, int G) {
  const int lig = threadIdx.x & (G - 1);
  const int64_t gpb = kBlock / G;
  const int nvec = D / VEC;
  const int64_t end = at.off[at.nt];
  for (int64_t i = (int64_t)blockIdx.x * gpb + threadIdx.x / G + G; i < n; i += (int64_t)gridDim.x * gpb) {
    const int64_t vid = sorted[i];
    if (sorted[i - G] != vid || vid < 0 || vid >= end) continue;
    const int t = (at.nt > 1 && vid >= at.off[1]) ? 1 : 0;
    const float* __restrict__ table = t ? at.table[1] : at.table[0];
    RowRegs<VEC, NCH> w;
    row_load(w, table + (vid - (t ? at.off[1] : at.off[0])) * D, lig, G, nvec);
    row_store(w, served + (int64_t)perm[i] * D, lig, G, nvec);
  }
}

// the geometry of a row of D scalars (one element per chunk): lets a table of any width share a launch with a D = 1 table
static RowGeom scalar_geom(int D) {
  RowGeom g;
  g.vec = 1;
  g.nvec = D;
  int G = 1;
  while (G < D && G < kWave) G <<= 1;
  g.G = G;
  g.nch = (D + G - 1) / G;
  return g;
}

// at least 16 lanes per row: the long-gap coefficients of a row are summed by its group, and a narrow row (GloVe's
// [V, 1] bias: one lane) would walk all ~210 terms on one lane -- tens of microseconds of fp64 latency per launch
static RowGeom wide(RowGeom g) {
  g.G = std::max(g.G, 16);
  g.nch = (g.nvec + g.G - 1) / g.G;
  return g;
}

// one launch for tables [first, first + count) of ct whose geometries share the chunk width
static int launch_catchup(AdamCatchupTables ct, int first, int count, const RowGeom* geo, const AdamLazyArgs& ax,
                          hipStream_t st) {
  AdamCatchupTables c = ct;
  RowGeom g = geo[first];
  int64_t blocks = 1;
  for (int y = 0; y < count; ++y) {
    const int t = first + y;
    c.table[y] = ct.table[t];
    c.mu[y] = ct.mu[t];
    c.nu[y] = ct.nu[t];
    c.last[y] = ct.last[t];
    c.ids[y] = ct.ids[t];
    c.V[y] = ct.V[t];
    c.n[y] = ct.n[t];
    c.D[y] = ct.D[t];
    c.modulus[y] = ct.modulus[t];
    c.G[y] = geo[t].G;
    g.nch = std::max(g.nch, geo[t].nch);
    blocks = std::max<int64_t>(blocks, grid_for_groups(ct.n[t], geo[t].G));
  }
  ESR_DISPATCH_ROW(g, ESR_KT("adam_catchup_kernel", st,
                             hipLaunchKernelGGL((adam_catchup_kernel<VEC, NCH>), dim3((int)blocks, count), dim3(kBlock), 0,
                                                st, c, ax)));
  return check_launch("esr_adam_catchup_rows2");
}

static bool adam_ptrs_ok(const float* table, const float* mu, const float* nu, const int32_t* last, const int32_t* ids) {
  return ((((uintptr_t)table | (uintptr_t)mu | (uintptr_t)nu) & 15) == 0) &&
         ((((uintptr_t)last | (uintptr_t)ids) & 3) == 0);
}

}  // namespace esr

using namespace esr;

extern "C" {

int esr_adam_catchup_rows2(float* table0, float* mu0, float* nu0, int32_t* last0, int64_t V0, int D0, const int32_t* ids0,
                           int64_t n0, int modulus0, float* table1, float* mu1, float* nu1, int32_t* last1, int64_t V1,
                           int D1, const int32_t* ids1, int64_t n1, int modulus1, int step, float lr, float b1, float b2,
                           float eps, esr_stream_t stream) {
  const bool two = table1 != nullptr;
  ESR_REQUIRE(V0 > 0 && D0 > 0 && n0 >= 0 && modulus0 >= 0 && step >= 1 && V0 < ((int64_t)1 << 31),
              "esr_adam_catchup_rows2: bad arguments for table 0 (V=%lld D=%d n=%lld modulus=%d step=%d)", (long long)V0, D0,
              (long long)n0, modulus0, step);
  ESR_REQUIRE(!two || (V1 > 0 && D1 > 0 && n1 >= 0 && modulus1 >= 0 && V1 < ((int64_t)1 << 31)),
              "esr_adam_catchup_rows2: bad arguments for table 1 (V=%lld D=%d n=%lld modulus=%d)", (long long)V1, D1,
              (long long)n1, modulus1);
  ESR_REQUIRE(table0 && mu0 && nu0 && last0 && ids0, "esr_adam_catchup_rows2: null pointer (table 0)");
  ESR_REQUIRE(!two || (mu1 && nu1 && last1 && ids1), "esr_adam_catchup_rows2: null pointer (table 1)");
  ESR_REQUIRE(adam_ptrs_ok(table0, mu0, nu0, last0, ids0) && (!two || adam_ptrs_ok(table1, mu1, nu1, last1, ids1)),
              "esr_adam_catchup_rows2: table / mu / nu must be 16-byte aligned, last / ids 4-byte aligned");
  RowGeom geo[2] = {row_geom(D0), row_geom(two ? D1 : D0)};
  ESR_REQUIRE(geo[0].nch <= kMaxChunksPerLane && geo[1].nch <= kMaxChunksPerLane,
              "esr_adam_catchup_rows2: D=%d / %d not supported", D0, two ? D1 : D0);
  AdamCatchupTables ct{{table0, table1}, {mu0, mu1}, {nu0, nu1}, {last0, last1}, {ids0, ids1}, {V0, two ? V1 : 0},
                       {n0, two ? n1 : 0}, {D0, two ? D1 : 1}, {1, 1}, {modulus0, two ? modulus1 : 0}};
  AdamLazyArgs ax;
  adam_lazy_args(ax, lr, b1, b2, eps, step);
  if (n0 == 0 && (!two || n1 == 0)) return ESR_OK;
  hipStream_t st = as_stream(stream);
  if (!two) {
    geo[0] = wide(geo[0]);
    return launch_catchup(ct, 0, 1, geo, ax, st);
  }
  if (geo[0].vec != geo[1].vec) {  // one float4 table, one scalar one (GloVe: the embedding and its [V, 1] bias)
    const RowGeom s0 = scalar_geom(D0), s1 = scalar_geom(D1);
    if (s0.nch <= kMaxChunksPerLane && s1.nch <= kMaxChunksPerLane) {
      geo[0] = s0;
      geo[1] = s1;
    } else {  // (a float4 table too wide to be walked as scalars: two launches)
      geo[0] = wide(geo[0]);
      geo[1] = wide(geo[1]);
      const int rc = launch_catchup(ct, 0, 1, geo, ax, st);
      return rc != ESR_OK ? rc : launch_catchup(ct, 1, 1, geo, ax, st);
    }
  }
  geo[0] = wide(geo[0]);
  geo[1] = wide(geo[1]);
  return launch_catchup(ct, 0, 2, geo, ax, st);
}

int esr_adam_catchup_gather(float* const* tables, float* const* mus, float* const* nus, int32_t* const* lasts,
                            const int64_t* row_offsets, int ntables, int D, const int32_t* sorted_rows, const int32_t* perm,
                            int64_t n, float* served, int step, float lr, float b1, float b2, float eps,
                            esr_stream_t stream) {
  ESR_REQUIRE(ntables >= 1 && ntables <= 2 && D > 0 && n >= 0 && step >= 1,
              "esr_adam_catchup_gather: ntables=%d not in [1, 2] or bad D=%d n=%lld step=%d", ntables, D, (long long)n,
              step);
  const RowGeom g = wide(row_geom(D));  // the geometry esr_adam_catchup_rows2 gives a table of this width (same sums)
  ESR_REQUIRE(g.nch <= kMaxChunksPerLane, "esr_adam_catchup_gather: D=%d not supported", D);
  ESR_REQUIRE(tables && mus && nus && lasts && row_offsets && (n == 0 || (sorted_rows && (served == nullptr || perm))),
              "esr_adam_catchup_gather: null pointer");  // (an empty list may come with null ids: torch's empty tensors)
  ESR_REQUIRE((((uintptr_t)sorted_rows | (uintptr_t)perm) & 3) == 0 && ((uintptr_t)served & (D % 4 ? 3 : 15)) == 0,
              "esr_adam_catchup_gather: misaligned ids or served rows");
  ESR_REQUIRE(row_offsets[0] == 0, "esr_adam_catchup_gather: row_offsets[0] must be 0");
  AdamServeTables at{};
  at.nt = ntables;
  for (int i = 0; i < ntables; ++i) {
    ESR_REQUIRE(tables[i] && mus[i] && nus[i] && lasts[i] && row_offsets[i + 1] > row_offsets[i],
                "esr_adam_catchup_gather: bad table %d", i);
    ESR_REQUIRE(adam_ptrs_ok(tables[i], mus[i], nus[i], lasts[i], sorted_rows),
                "esr_adam_catchup_gather: table %d: table / mu / nu must be 16-byte aligned, last 4-byte aligned", i);
    at.table[i] = tables[i];
    at.mu[i] = mus[i];
    at.nu[i] = nus[i];
    at.last[i] = lasts[i];
  }
  for (int i = 0; i <= 2; ++i) at.off[i] = row_offsets[std::min(i, ntables)];
  ESR_REQUIRE(row_offsets[ntables] < ((int64_t)1 << 31), "esr_adam_catchup_gather: %lld virtual rows >= 2^31",
              (long long)row_offsets[ntables]);
  if (n == 0) return ESR_OK;
  AdamLazyArgs ax;
  adam_lazy_args(ax, lr, b1, b2, eps, step);
  const int grid = grid_for_groups(n, g.G);
  hipStream_t st = as_stream(stream);
  ESR_DISPATCH_ROW(g, ESR_KT("adam_catchup_gather_kernel", st,
                             hipLaunchKernelGGL((adam_catchup_gather_kernel<VEC, NCH>), dim3(grid), dim3(kBlock), 0, st, at,
                                                sorted_rows, perm, n, served, D, g.G, ax)));
  if (served == nullptr || n <= g.G) return check_launch("esr_adam_catchup_gather");
  ESR_DISPATCH_ROW(g, ESR_KT("adam_serve_tail_kernel", st,
                             hipLaunchKernelGGL((adam_serve_tail_kernel<VEC, NCH>), dim3(grid_for_groups(n - g.G, g.G)),
                                                dim3(kBlock), 0, st, at, sorted_rows, perm, n, served, D, g.G)));
  return check_launch("esr_adam_catchup_gather");
}

int esr_adam_flush(float* table, float* mu, float* nu, int32_t* last, int64_t V, int D, int step, float lr, float b1, float b2,
                   float eps, esr_stream_t stream) {
  ESR_REQUIRE(V > 0 && D > 0 && step >= 0 && V < ((int64_t)1 << 31), "esr_adam_flush: bad arguments (V=%lld D=%d step=%d)",
              (long long)V, D, step);
  ESR_REQUIRE(table && mu && nu && last, "esr_adam_flush: null pointer");
  ESR_REQUIRE(((((uintptr_t)table | (uintptr_t)mu | (uintptr_t)nu) & 15) == 0) && ((uintptr_t)last & 3) == 0,
              "esr_adam_flush: table / mu / nu must be 16-byte aligned, last 4-byte aligned");
  const RowGeom g = wide(row_geom(D));
  ESR_REQUIRE(g.nch <= kMaxChunksPerLane, "esr_adam_flush: D=%d not supported", D);
  if (step == 0) return ESR_OK;  // nothing has happened yet
  AdamLazyArgs ax;
  adam_lazy_args(ax, lr, b1, b2, eps, step);
  const int grid = grid_for_groups(V, g.G);
  hipStream_t st = as_stream(stream);
  ESR_DISPATCH_ROW(g, ESR_KT("adam_flush_kernel", st,
                             hipLaunchKernelGGL((adam_flush_kernel<VEC, NCH>), dim3(grid), dim3(kBlock), 0, st, table, mu, nu,
                                                last, V, D, g.G, ax)));
  return check_launch("esr_adam_flush");
}

}  // extern "C"
