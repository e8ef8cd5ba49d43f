// The pair table with FOUR sums per slot (esr_ratings.hip: the user-similarity job reduces n, P, Qa and Qb per user pair).
// The narrow table of esr_cooccur_table.h is left as it is; this is its wide form, built from the same pieces: mix64, the
// probe bounded by the capacity, the failure word of the 256-byte header, compact_claim.
//   table       [256-byte header | keys uint64[capacity] | sums uint64[4][capacity]], plane-major: plane s of slot i is
//               sums[s * capacity + i].  Header word 0: occupied slots, word 1: failure bits -- the narrow table's header,
//               so the host reads both the same way.
//   add         the key's slot is claimed ONCE by a 64-bit compare-and-swap; then four 64-bit atomic adds, one per plane.
//               Integer sums: the result does not depend on the order of the atomics.  No loop waits on another
//               workgroup; a probe sequence that wraps raises kFailProbeWrapped.
#pragma once
#include "esr_cooccur_table.h"

namespace esr {

constexpr int kWideSums = 4;
constexpr unsigned long long kFailNotAscending = 128;  // beside the narrow table's bits 1..16, the lookup's 32, the neighbours' 64

struct WideTable {
  unsigned long long* used;  // header word 0
  unsigned long long* fail;  // header word 1
  unsigned long long* keys;
  unsigned long long* sums;  // [kWideSums][capacity]
  unsigned long long mask;   // capacity - 1
};
static inline WideTable wide_view(void* table, int64_t capacity) {
  char* base = (char*)table;
  WideTable t;
  t.used = (unsigned long long*)base;
  t.fail = t.used + 1;
  t.keys = (unsigned long long*)(base + kCooccurHeaderBytes);
  t.sums = t.keys + capacity;
  t.mask = (unsigned long long)capacity - 1;
  return t;
}
static inline size_t wide_table_bytes(int64_t capacity) {
  return capacity <= 0 ? kCooccurHeaderBytes : kCooccurHeaderBytes + 8 * (size_t)(1 + kWideSums) * (size_t)capacity;
}
// compact_claim and carry_fail take the header alone
static inline __host__ __device__ CooccurTable header_of(const WideTable& w) {
  CooccurTable t;
  t.used = w.used, t.fail = w.fail, t.keys = w.keys, t.sums = w.sums, t.mask = w.mask;
  return t;
}

#ifdef __HIPCC__
// sums[s][slot of key] += w[s] for the four planes, claiming a slot for a new key.  At most capacity probes.
__device__ __forceinline__ void wide_add(const WideTable& t, unsigned long long key, unsigned long long w0,
                                         unsigned long long w1, unsigned long long w2, unsigned long long w3) {
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
      unsigned long long* s = t.sums + slot;
      atomicAdd(s, w0);
      atomicAdd(s + (t.mask + 1), w1);
      atomicAdd(s + 2 * (t.mask + 1), w2);
      atomicAdd(s + 3 * (t.mask + 1), w3);
      return;
    }
  }
  atomicOr(t.fail, kFailProbeWrapped);
}
#endif

}  // namespace esr
