// The pair table of the co-occurrence builders (esr_cooccur.hip: window pairs; esr_dice.hip: set pairs), shared by both.
//   table       open addressing, linear probing: [256-byte header | keys uint64[capacity] | sums uint64[capacity]],
//               key = index << 32 | other, all ones = empty (no int32 id >= 0 makes it).  A slot is claimed by a 64-bit
//               compare-and-swap and summed into by a 64-bit atomic add.  A probe sequence is bounded by the capacity: one
//               that wraps raises the header's failure word instead of spinning or dropping the increment silently.
//               The caller keeps capacity >= used + (pairs a call can emit), so that never happens in a sound builder.
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
static inline bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

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
#endif

}  // namespace esr
