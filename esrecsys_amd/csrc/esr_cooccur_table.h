// The pair table of the builders (esr_cooccur.hip: window pairs; esr_dice.hip: set pairs; esr_terms.hip: term statistics,
// the dictionary lookup, tf-idf scratch), and every idiom that belongs to the table and not to one builder.
//   table       open addressing, linear probing: [256-byte header | keys uint64[capacity] | sums uint64[capacity]],
//               key = index << 32 | other, all ones = empty (no int32 id >= 0 makes it).  A slot is claimed by a 64-bit
//               compare-and-swap and summed into by a 64-bit atomic add.  A probe sequence is bounded by the capacity: one
//               that wraps raises the header's failure word instead of spinning or dropping the increment silently.
//               The caller keeps capacity >= used + (pairs a call can emit), so that never happens in a sound builder
//               (wikipedia/pair_table.py: PairTable.reserve).
//   device      table_add / table_find; wave_merge_add (equal keys of a wave merged before the atomic); doc_of (the
//               document of a position); compact_claim (an output row of a compaction); carry_fail (the failure word
//               follows the entries from one table into another).
//   host        ESR_REQUIRE_TABLE: the capacity check of every entry point that takes a table.
#pragma once
#include "esr_common.h"

namespace esr {

constexpr unsigned long long kEmptyKey = ~0ull;
constexpr size_t kCooccurHeaderBytes = 256;
// failure word of the header (or-ed bits)
constexpr unsigned long long kFailProbeWrapped = 1, kFailNegativeId = 2, kFailBadOffsets = 4, kFailCompactOverflow = 8,
                             kFailDocTooLong = 16;

struct CooccurTable {
  unsigned long long* used;  // header word 0: occupied slots (= new-key insertions)
  unsigned long long* fail;  // header word 1
  unsigned long long* keys;
  unsigned long long* sums;
  unsigned long long mask;   // capacity - 1
};
static inline CooccurTable table_view(void* table, int64_t capacity) {
  char* base = (char*)table;
  CooccurTable t;
  t.used = (unsigned long long*)base;
  t.fail = t.used + 1;
  t.keys = (unsigned long long*)(base + kCooccurHeaderBytes);
  t.sums = t.keys + capacity;
  t.mask = (unsigned long long)capacity - 1;
  return t;
}

static inline int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(kMaxGrid, cdiv(n, kBlock))); }
static inline bool table_capacity_ok(int64_t c) { return c >= 2 && (c & (c - 1)) == 0; }  // mask = capacity - 1

// `fn` and `name` are string literals; returns ESR_EINVAL from the caller, as ESR_REQUIRE does
#define ESR_REQUIRE_TABLE(fn, name, capacity) \
  ESR_REQUIRE(esr::table_capacity_ok(capacity), fn ": " name "=%lld is not a power of two >= 2", (long long)(capacity))

#ifdef __HIPCC__
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {  // murmur3's finalizer
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// sums[slot of key] += w, claiming a slot for a new key.  At most capacity probes.
__device__ __forceinline__ void table_add(const CooccurTable& t, unsigned long long key, unsigned long long w) {
  unsigned long long slot = mix64(key) & t.mask;
  for (unsigned long long probes = 0; probes <= t.mask; ++probes, slot = (slot + 1) & t.mask) {
    unsigned long long k = __hip_atomic_load(&t.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == kEmptyKey) {
      k = atomicCAS(&t.keys[slot], kEmptyKey, key);
      if (k == kEmptyKey) {
        atomicAdd(t.used, 1ull);
        k = key;
      }
    }
    if (k == key) {
      atomicAdd(&t.sums[slot], w);
      return;
    }
  }
  atomicOr(t.fail, kFailProbeWrapped);
}

// the sum of `key`, or false when the table does not hold it.  Read-only: the table is complete when this runs.
__device__ __forceinline__ bool table_find(const CooccurTable& t, unsigned long long key, unsigned long long& sum) {
  unsigned long long slot = mix64(key) & t.mask;
  for (unsigned long long probes = 0; probes <= t.mask; ++probes, slot = (slot + 1) & t.mask) {
    const unsigned long long k = t.keys[slot];
    if (k == key) {
      sum = t.sums[slot];
      return true;
    }
    if (k == kEmptyKey) return false;
  }
  return false;
}

// sums[key] += w for every live lane of a wave, equal keys merged first: the lowest live lane broadcasts its key, the
// lanes that hold the same key are counted by a ballot and that lane makes ONE table access for all of them.  A few such
// rounds take the frequent keys (a frequent token repeats inside any window, a document may be one token repeated); what
// is left goes lane by lane.  `w` is the same in every lane.
// PRECONDITION: every lane of the wave calls this together, live or not -- the ballots need the whole wave, so the caller
// keeps whole waves in its loop.
constexpr int kMergeRounds = 4;
__device__ __forceinline__ void wave_merge_add(const CooccurTable& t, bool live, unsigned long long key,
                                               unsigned long long w, int lane) {
#pragma nounroll  // (a rolled loop at both call sites before it moved here; unrolled, each kernel grows by 300 instructions)
  for (int m = 0; m < kMergeRounds; ++m) {
    const unsigned long long alive = __ballot(live);
    if (!alive) break;
    const int leader = __ffsll((long long)alive) - 1;
    const unsigned long long lk = __shfl(key, leader, kWave);
    const bool same = live && key == lk;
    const int cnt = __popcll(__ballot(same));
    if (lane == leader) table_add(t, lk, w * (unsigned long long)cnt);
    if (same) live = false;
  }
  if (live) table_add(t, key, w);
}

// the document of position q: the first k in [lo, hi] with doc_offsets[k] > q, or hi (empty documents repeat an offset);
// the document is k - 1
__device__ __forceinline__ int64_t doc_of(const int64_t* __restrict__ doc_offsets, int64_t lo, int64_t hi, int64_t q) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (doc_offsets[mid] > q) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the output row of one occupied slot in a compaction into `rows` rows, or false (and the failure bit) when the caller's
// count is not the table's: nothing is written out of bounds
__device__ __forceinline__ bool compact_claim(const CooccurTable& t, unsigned long long* __restrict__ counter,
                                              int64_t rows, unsigned long long& pos) {
  pos = atomicAdd(counter, 1ull);
  if (pos < (unsigned long long)rows) return true;
  atomicOr(t.fail, kFailCompactOverflow);
  return false;
}

// what src's launches raised stays raised in the table its entries move into
__device__ __forceinline__ void carry_fail(const CooccurTable& src, const CooccurTable& dst) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && *src.fail) atomicOr(dst.fail, *src.fail);
}
#endif

}  // namespace esr
