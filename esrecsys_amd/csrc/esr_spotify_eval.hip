// esr_spotify_eval.hip -- eval_step's top_k(500) over every track (spotify/train_spotify.py:113-131) for a BATCH of
// playlists: the reference evaluates eval_steps = 1000 playlists every eval_every_steps (:270-281).
//
// One call scores the T tracks of the corpus against the context rows of P playlists and keeps a running top-k per
// playlist; no [P, T] score matrix is ever written.  A workgroup gathers the rows of 512 / G tracks ONCE into registers
// and scores them against every playlist of its playlist group, whose context rows pass through LDS a sub-tile at a
// time.  The top-k is the list / threshold pipeline of esr_retrieve.hip (select_topk_head / _compact / _tail): the first
// chunk of tracks is scored densely and selected, every later chunk appends only the (score, index) records that reach
// the playlist's threshold.
//
// Scores are bit-identical to esr_spotify_affinity_all (esr_spotify.hip), whose 16 lanes per track are replayed here
// as 16 VIRTUAL lanes: virtual lane l chains, from +0, the elements it owns in increasing position -- float4 chunk q
// belongs to lane q % 16 when F % 4 == 0, element d to lane d % 16 otherwise -- and the 16 partials are combined by
// the xor tree o = 8, 4, 2, 1 of the __shfl_xor butterfly.  A real lane holds the virtual lanes l = g + G v
// (g < G, v < 16 / G): the tree's steps with o >= G are additions inside the lane, the others go across its G lanes.
// (Every lane of the butterfly ends with the same bits: IEEE addition commutes.)  G = 1 for 2F <= 64, 2 for <= 128,
// 4 for <= 256: 64 row elements per lane and track either way.
#include "esr_common.h"

#include <algorithm>
#include <cstdlib>

namespace esr {

constexpr int kEvMaxCtx = 32;      // context tracks per playlist (reference: 5)
constexpr int kEvMaxDim = 256;     // 2F
constexpr float kEvBoost = 0.1f;   // spotify/models.py:76-81, as in esr_spotify.hip
constexpr int kEvTracks = 2;       // tracks per lane group and workgroup pass
constexpr int kEvLdsFloats = 12288;  // context rows of one playlist sub-tile (48 KB)
constexpr int kEvLdsIds = 512;       // their raw ids
constexpr int kEvMaxSubtile = 64;
constexpr int kEvFirstChunk = 8192;

// element e of virtual lane l: its position in the 2F-row
template <bool VEC>
__device__ __forceinline__ int ev_pos(int l, int e) {
  return VEC ? 4 * (l + 16 * (e >> 2)) + (e & 3) : l + 16 * e;
}

// rows [P * n][2F] = concat(album_table[album mod A], artist_table[artist]) of every context track
__global__ __launch_bounds__(kBlock) void spotify_eval_ctx_kernel(const float* __restrict__ album_table, int64_t A,
                                                                 const float* __restrict__ artist_table, int F,
                                                                 const int32_t* __restrict__ ctx_album,
                                                                 const int32_t* __restrict__ ctx_artist, int64_t rows,
                                                                 float* __restrict__ out) {
  const int D2 = 2 * F;
  const int64_t total = rows * D2;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int64_t r = i / D2;
    const int d = (int)(i - r * D2);
    out[i] = d < F ? album_table[((int64_t)ctx_album[r] % A) * F + d] : artist_table[(int64_t)ctx_artist[r] * F + d - F];
  }
}

struct EvArgs {
  const float* album_table;
  int64_t A;
  const float* artist_table;
  int F, n, P;
  const float* ctx_rows;         // [P * n][2F]
  const int32_t* ctx_album;      // [P * n] raw ids
  const int32_t* ctx_artist;
  const int32_t* all_albums;     // [T]
  const int32_t* all_artists;
  int64_t t0;                    // this chunk: tracks [t0, t0 + nt)
  int nt;
  int pg, pt;                    // playlists per workgroup (blockIdx.y), per LDS sub-tile
  float* S;                      // dense chunk: S[p * ldS + (t - t0)], or null
  int64_t ldS;
  const float* tau;              // filtered chunk: append (score, t) to pairs[p * ppitch + ...] when score >= tau[p]
  int32_t* cnt;
  int2* pairs;
  int64_t ppitch;
};

// D2T: 2F known at compile time (0: a.F at run time, every element guarded)
template <int G, bool VEC, int D2T>
__global__ __launch_bounds__(kBlock) void spotify_eval_score_kernel(EvArgs a) {
  __shared__ __attribute__((aligned(16))) float s_ctx[kEvLdsFloats];
  __shared__ int32_t s_al[kEvLdsIds], s_ar[kEvLdsIds];
  constexpr int V = 16 / G;     // virtual lanes per lane
  constexpr int E = 4 * G;      // elements per virtual lane, at most
  constexpr int kGroups = kBlock / G;
  const int D2 = D2T ? D2T : 2 * a.F;
  const int F = D2 >> 1;
  const int n = a.n;
  const int g = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t tile0 = a.t0 + (int64_t)blockIdx.x * kGroups * kEvTracks;
  const int64_t tend = a.t0 + a.nt;
  const uint32_t A32 = a.A < ((int64_t)1 << 31) ? (uint32_t)a.A : 0u;

  float x[kEvTracks][V][E];
  int32_t al[kEvTracks], ar[kEvTracks];
  bool on[kEvTracks];
#pragma unroll
  for (int j = 0; j < kEvTracks; ++j) {
    const int64_t t = tile0 + grp + j * kGroups;
    on[j] = t < tend;
    al[j] = on[j] ? a.all_albums[t] : 0;
    ar[j] = on[j] ? a.all_artists[t] : 0;
  }
#pragma unroll
  for (int j = 0; j < kEvTracks; ++j) {
    const int64_t ha = A32 ? (int64_t)((uint32_t)al[j] % A32) : (int64_t)al[j] % a.A;
    const float* pa = a.album_table + ha * F;
    const float* pr = a.artist_table + (int64_t)ar[j] * F;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (VEC) {
#pragma unroll
        for (int e = 0; e < E; e += 4) {
          const int pos = ev_pos<VEC>(g + G * v, e);
          float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
          if (on[j] && pos < D2)
            r = pos < F ? *reinterpret_cast<const float4*>(pa + pos) : *reinterpret_cast<const float4*>(pr + pos - F);
          x[j][v][e] = r.x; x[j][v][e + 1] = r.y; x[j][v][e + 2] = r.z; x[j][v][e + 3] = r.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int pos = ev_pos<VEC>(g + G * v, e);
          x[j][v][e] = (on[j] && pos < D2) ? (pos < F ? pa[pos] : pr[pos - F]) : 0.f;
        }
      }
    }
  }

  const int p_begin = blockIdx.y * a.pg, p_end = min(a.P, p_begin + a.pg);
  for (int p0 = p_begin; p0 < p_end; p0 += a.pt) {
    const int np = min(a.pt, p_end - p0);
    __syncthreads();  // the previous sub-tile has been read
    {
      const int m = np * n * D2;
      const float* src = a.ctx_rows + (int64_t)p0 * n * D2;
      if (VEC) {
        for (int i = threadIdx.x; i < (m >> 2); i += kBlock)
          reinterpret_cast<float4*>(s_ctx)[i] = reinterpret_cast<const float4*>(src)[i];
      } else {
        for (int i = threadIdx.x; i < m; i += kBlock) s_ctx[i] = src[i];
      }
      for (int i = threadIdx.x; i < np * n; i += kBlock) {
        s_al[i] = a.ctx_album[(int64_t)p0 * n + i];
        s_ar[i] = a.ctx_artist[(int64_t)p0 * n + i];
      }
    }
    __syncthreads();
    for (int pp = 0; pp < np; ++pp) {
      const int p = p0 + pp;
      float best[kEvTracks];
#pragma unroll
      for (int j = 0; j < kEvTracks; ++j) best[j] = -INFINITY;
      for (int c = 0; c < n; ++c) {
        const float* cr = s_ctx + (pp * n + c) * D2;
        float s[kEvTracks][V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
#pragma unroll
          for (int j = 0; j < kEvTracks; ++j) s[j][v] = 0.f;
          if (VEC) {
#pragma unroll
            for (int e = 0; e < E; e += 4) {
              const int pos = ev_pos<VEC>(g + G * v, e);
              if (pos < D2) {
                const float4 y = *reinterpret_cast<const float4*>(cr + pos);
#pragma unroll
                for (int j = 0; j < kEvTracks; ++j)
                  s[j][v] = fmaf(x[j][v][e + 3], y.w,
                                 fmaf(x[j][v][e + 2], y.z, fmaf(x[j][v][e + 1], y.y, fmaf(x[j][v][e], y.x, s[j][v]))));
              }
            }
          } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const int pos = ev_pos<VEC>(g + G * v, e);
              if (pos < D2) {
                const float y = cr[pos];
#pragma unroll
                for (int j = 0; j < kEvTracks; ++j) s[j][v] = fmaf(x[j][v][e], y, s[j][v]);
              }
            }
          }
        }
        // the butterfly o = 8, 4, 2, 1: inside the lane while o >= G (virtual lane v ^ o / G), then across lanes
#pragma unroll
        for (int j = 0; j < kEvTracks; ++j) {
#pragma unroll
          for (int b = 3; b >= 0; --b) {
            const int o = 1 << b;
            if (o >= G) {
              const int step = o / G;
#pragma unroll
              for (int v = 0; v < V; ++v)
                if (!(v & step)) s[j][v] = s[j][v] + s[j][v ^ step];
            } else {
              s[j][0] += __shfl_xor(s[j][0], o, G);
            }
          }
          best[j] = fmaxf(best[j], s[j][0]);
        }
      }
#pragma unroll
      for (int j = 0; j < kEvTracks; ++j) {
        bool in_album = false, in_artist = false;
        for (int c = 0; c < n; ++c) {
          in_album |= al[j] == s_al[pp * n + c];
          in_artist |= ar[j] == s_ar[pp * n + c];
        }
        const float score = best[j] + (in_album ? kEvBoost : 0.f) + (in_artist ? kEvBoost : 0.f);
        const int64_t t = tile0 + grp + j * kGroups;
        const bool mine = on[j] && g == 0;
        if (a.S) {
          if (mine) a.S[(int64_t)p * a.ldS + (t - a.t0)] = score;
        } else {
          // !(score < tau): a NaN is kept too (the select ranks it by its bits, as the dense path does)
          const bool pass = mine && !(score < a.tau[p]);
          const unsigned long long mask = __ballot(pass);  // (p is uniform: one reservation per wave)
          if (mask) {
            const int lane = threadIdx.x & 63;
            const int lead = __ffsll((long long)mask) - 1;
            int base = 0;
            if (lane == lead) base = atomicAdd(a.cnt + p, __popcll(mask));
            base = __shfl(base, lead, 64);
            if (pass)
              a.pairs[(int64_t)p * a.ppitch + base + __popcll(mask & ((1ull << lane) - 1ull))] =
                  make_int2(__float_as_int(score), (int32_t)t);
          }
        }
      }
    }
  }
}

struct EvPlan {
  int64_t first, chunk, ppitch;
  int skip_upto;
  size_t off_ctx, off_S, off_pairs, off_cnt, off_tau, total;
};

static EvPlan ev_plan(int64_t P, int n, int64_t T, int F, int k) {
  EvPlan p;
  p.first = std::min<int64_t>(T, std::max<int64_t>(kEvFirstChunk, 16 * (int64_t)k));
  // lazy compaction as in esr_retrieve_topk: a list is cut back to its k best only once it holds more than skip_upto
  // records, so it must hold skip_upto plus a whole chunk (worst case: every track of the chunk reaches tau)
  p.skip_upto = (int)std::max<int64_t>(3 * (int64_t)k, 1536);
  p.chunk = 0;
  p.ppitch = 0;
  if (T > p.first) {
    // the lists of all P playlists together ~1 GiB
    const char* cc = getenv("ESR_SPOTIFY_EVAL_CHUNK");  // tracks per filtered chunk (tests / measuring hook)
    int64_t chunk = cc ? std::max<int64_t>(64, atoll(cc)) : std::max<int64_t>(4096, ((int64_t)1 << 27) / P - p.skip_upto);
    chunk = std::min<int64_t>(chunk, (int64_t)1 << 20);
    p.chunk = std::min<int64_t>(chunk, T - p.first);
    p.ppitch = p.skip_upto + p.chunk;
  }
  size_t o = 0;
  p.off_ctx = o; o += align_up((size_t)P * n * 2 * F * 4, 256);
  p.off_S = o; o += align_up((size_t)P * p.first * 4, 256);
  p.off_pairs = o; o += align_up((size_t)P * p.ppitch * 8, 256);
  p.off_cnt = o; o += align_up((size_t)P * 4, 256);
  p.off_tau = o; o += align_up((size_t)P * 4, 256);
  p.total = o;
  return p;
}

static void ev_score(EvArgs a, hipStream_t st) {
  const int D2 = 2 * a.F;
  const int G = D2 <= 64 ? 1 : (D2 <= 128 ? 2 : 4);
  const bool vec = (a.F & 3) == 0;
  a.pt = std::min(kEvMaxSubtile, std::min(kEvLdsFloats / (a.n * D2), kEvLdsIds / a.n));
  const int64_t gx = cdiv(a.nt, (int64_t)(kBlock / G) * kEvTracks);
  // enough workgroups to fill the chip (~2048), each reusing its gathered rows over as many playlists as that allows
  const int64_t ny = std::max<int64_t>(1, std::min<int64_t>(cdiv(2048, gx), cdiv(a.P, a.pt)));
  a.pg = (int)cdiv(a.P, ny);
  const dim3 grid((unsigned)gx, (unsigned)cdiv(a.P, a.pg));
#define ESR_EV_LAUNCH(G_, VEC_, D2T_) \
  ESR_KT("spotify_eval_score_kernel", st, hipLaunchKernelGGL((spotify_eval_score_kernel<G_, VEC_, D2T_>), grid, dim3(kBlock), 0, st, a))
  if (vec && D2 == 64) ESR_EV_LAUNCH(1, true, 64);
  else if (vec && G == 1) ESR_EV_LAUNCH(1, true, 0);
  else if (vec && G == 2) ESR_EV_LAUNCH(2, true, 0);
  else if (vec) ESR_EV_LAUNCH(4, true, 0);
  else if (G == 1) ESR_EV_LAUNCH(1, false, 0);
  else if (G == 2) ESR_EV_LAUNCH(2, false, 0);
  else ESR_EV_LAUNCH(4, false, 0);
#undef ESR_EV_LAUNCH
}

}  // namespace esr

using namespace esr;

extern "C" {

size_t esr_spotify_topk_batch_workspace_bytes(int64_t P, int n, int64_t T, int F, int k) {
  if (P <= 0 || n <= 0 || T <= 0 || F <= 0 || k <= 0) return 256;
  return ev_plan(P, n, T, F, k).total;
}

int esr_spotify_topk_batch(const float* album_table, int64_t n_album_rows, const float* artist_table, int64_t n_artists,
                           int F, const int32_t* ctx_album, const int32_t* ctx_artist, int64_t P, int n,
                           const int32_t* all_albums, const int32_t* all_artists, int64_t T, int k, float* out_scores,
                           int32_t* out_indices, void* workspace, size_t workspace_bytes, esr_stream_t stream) {
  TraceScope trace_scope_("esr_spotify_topk_batch");
  ESR_REQUIRE(n >= 1 && n <= kEvMaxCtx && F >= 1 && 2 * F <= kEvMaxDim && n_album_rows > 0 && n_artists > 0,
              "esr_spotify_topk_batch: bad sizes n=%d F=%d (1 <= n <= %d, 2F <= %d)", n, F, kEvMaxCtx, kEvMaxDim);
  ESR_REQUIRE(P >= 1 && P < ((int64_t)1 << 24) && T >= 1 && T < ((int64_t)1 << 31),
              "esr_spotify_topk_batch: bad sizes P=%lld T=%lld", (long long)P, (long long)T);
  ESR_REQUIRE(k >= 1 && k <= T && k <= kSelectMaxK, "esr_spotify_topk_batch: k=%d (1 <= k <= min(T, %d))", k, kSelectMaxK);
  ESR_REQUIRE(album_table && artist_table && ctx_album && ctx_artist && all_albums && all_artists && out_scores &&
                  out_indices && workspace,
              "esr_spotify_topk_batch: null pointer");
  const EvPlan pl = ev_plan(P, n, T, F, k);
  if (workspace_bytes < pl.total || ((uintptr_t)workspace & 15)) {
    set_error("esr_spotify_topk_batch: workspace %zu bytes < %zu required (or misaligned)", workspace_bytes, pl.total);
    return ESR_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  char* base = (char*)workspace;
  float* ctx_rows = (float*)(base + pl.off_ctx);
  float* S = (float*)(base + pl.off_S);
  int2* pairs = (int2*)(base + pl.off_pairs);
  int32_t* cnt = (int32_t*)(base + pl.off_cnt);
  float* tau = (float*)(base + pl.off_tau);
  const int64_t ctx_elems = P * n * 2 * F;
  ESR_KT("spotify_eval_ctx_kernel", st,
         hipLaunchKernelGGL(spotify_eval_ctx_kernel, dim3((int)std::min<int64_t>(cdiv(ctx_elems, kBlock), 4096)), dim3(kBlock),
                            0, st, album_table, n_album_rows, artist_table, F, ctx_album, ctx_artist, P * n, ctx_rows));
  EvArgs a;
  a.album_table = album_table; a.A = n_album_rows; a.artist_table = artist_table; a.F = F; a.n = n; a.P = (int)P;
  a.ctx_rows = ctx_rows; a.ctx_album = ctx_album; a.ctx_artist = ctx_artist;
  a.all_albums = all_albums; a.all_artists = all_artists;
  a.t0 = 0; a.nt = (int)pl.first; a.pg = 0; a.pt = 0;
  a.S = S; a.ldS = pl.first;
  a.tau = nullptr; a.cnt = nullptr; a.pairs = nullptr; a.ppitch = 0;
  ev_score(a, st);
  if (T == pl.first) {  // the whole corpus is one dense chunk
    int rc = ESR_OK;
    ESR_KT("topk_select_kernel", st, rc = select_topk_dense(S, pl.first, P, (int)T, k, out_scores, out_indices, st));
    return rc ? rc : check_launch("esr_spotify_topk_batch");
  }
  int rc = ESR_OK;
  ESR_KT("topk_select_kernel", st, rc = select_topk_head(S, pl.first, P, (int)pl.first, k, pairs, pl.ppitch, cnt, tau, st));
  if (rc) return rc;
  a.S = nullptr; a.ldS = 0;
  a.tau = tau; a.cnt = cnt; a.pairs = pairs; a.ppitch = pl.ppitch;
  for (int64_t c0 = pl.first; c0 < T; c0 += pl.chunk) {
    const int64_t nc = std::min<int64_t>(pl.chunk, T - c0);
    a.t0 = c0;
    a.nt = (int)nc;
    ev_score(a, st);
    if (c0 + nc < T) {
      ESR_KT("topk_select_kernel", st, rc = select_topk_compact(pairs, pl.ppitch, cnt, P, k, tau, st, pl.skip_upto));
      if (rc) return rc;
    }
  }
  ESR_KT("topk_select_kernel", st, rc = select_topk_tail(pairs, pl.ppitch, cnt, P, k, out_scores, out_indices, st));
  return rc ? rc : check_launch("esr_spotify_topk_batch");
}

}  // extern "C"
