// Stand-alone host program over esr_philox.h (no HIP, no library): prints the three Random123 known answers of
// Philox4x32-10, sampler indices for the (seed, step, count, T) quadruples given on the command line, and what the
// offsets validation and the list layout say for a few groups.  Meant to be built with -fsanitize=address,undefined:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/spotify_philox_host.cpp -o philox_host
//   ./philox_host 0x123456789abcdef 7 9 13
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../esrecsys_amd/csrc/esr_philox.h"

static void kat(const uint32_t c[4], const uint32_t k[2]) {
  uint32_t out[4];
  esr::philox4x32_10(c, k, out);
  printf("kat %08x %08x %08x %08x\n", out[0], out[1], out[2], out[3]);
}

int main(int argc, char** argv) {
  const uint32_t c0[4] = {0, 0, 0, 0}, k0[2] = {0, 0};
  const uint32_t c1[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, k1[2] = {0xffffffffu, 0xffffffffu};
  const uint32_t c2[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, k2[2] = {0xa4093822u, 0x299f31d0u};
  kat(c0, k0);
  kat(c1, k1);
  kat(c2, k2);
  for (int a = 1; a + 3 < argc; a += 4) {
    const uint64_t seed = strtoull(argv[a], nullptr, 0);
    const uint32_t step = (uint32_t)strtoul(argv[a + 1], nullptr, 0), count = (uint32_t)strtoul(argv[a + 2], nullptr, 0);
    const uint64_t T = strtoull(argv[a + 3], nullptr, 0);
    if (T < 2 || T - 1 > 0x7fffffffu) {
      fprintf(stderr, "T out of range\n");
      return 2;
    }
    printf("idx");
    for (uint32_t i = 0; i < count; ++i) printf(" %u", esr::sp_negative_index(seed, step, i, (uint32_t)(T - 1)));
    printf("\n");
  }
  // offsets validation: 0 = good (and the longest list), else 1 + the offending entry
  const std::vector<std::vector<int64_t>> groups = {
      {0, 3}, {0, 1, 4, 44}, {1, 3}, {0, 3, 3}, {0, 5, 4}, {0, 0}, {0, INT64_MAX}, {0, 2, INT64_MIN}, {INT64_MIN, 0}};
  for (const auto& g : groups) {
    int64_t max_m = -1;
    const int64_t rc = esr::sp_check_offsets(g.data(), (int64_t)g.size() - 1, &max_m);
    printf("offsets %" PRId64 " %" PRId64 "\n", rc, max_m);
  }
  // list layout for n = 5, o = 64 and the second group: starts are 64-int aligned and blocks do not overlap
  const std::vector<int64_t>& off = groups[1];
  const int n = 5, o = 64, K = (int)off.size() - 1;
  int64_t prev_end = 0;
  printf("starts");
  for (int j = 0; j < K; ++j) {
    const int64_t s = esr::sp_list_start(j, n, o, off[j]), R = n + (off[j + 1] - off[j]) + o;
    if (s % 64 != 0 || s < prev_end) {
      fprintf(stderr, "layout: block %d at %" PRId64 " overlaps or is misaligned\n", j, s);
      return 3;
    }
    prev_end = s + 2 * R;
    printf(" %" PRId64, s);
  }
  if (esr::sp_list_region(K, n, o, off[K]) < prev_end) return 4;
  printf(" region %" PRId64 "\n", esr::sp_list_region(K, n, o, off[K]));
  return 0;
}
