// Stand-alone host program over esr_bpr_sample.h (no HIP, no library): reads cases from the file named on the command
// line and prints every triple the header draws for them.  A case is the whitespace-separated integers
//   nu ni nnz seed step0 K B   row_offsets[nu + 1]   row_upos[nnz]   row_ipos[nnz]
// and is answered by one line "case K B" followed by K * B lines "u i j valid" (step-major, slot-minor).  The arrays are
// heap allocations of exactly the stated sizes.  Meant to be built with -fsanitize=address,undefined:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/bpr_sample_host.cpp -o bpr_host
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../esrecsys_amd/csrc/esr_bpr_sample.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  printf("max_tries %d\n", esr::kBprMaxTries);
  int64_t nu, ni, nnz, K, B;
  uint64_t seed, step0;
  while (fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNd64, &nu, &ni, &nnz, &seed,
                &step0, &K, &B) == 7) {
    if (nu < 1 || ni < 1 || ni > INT32_MAX || nnz < 1 || nnz > INT32_MAX || K < 1 || B < 1 || step0 > UINT32_MAX) {
      fprintf(stderr, "case out of range\n");
      return 3;
    }
    std::vector<int64_t> offsets((size_t)nu + 1);
    std::vector<int32_t> upos((size_t)nnz), ipos((size_t)nnz);
    for (auto& v : offsets)
      if (fscanf(f, "%" SCNd64, &v) != 1) return 4;
    for (auto& v : upos)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    for (auto& v : ipos)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    printf("case %" PRId64 " %" PRId64 "\n", K, B);
    for (int64_t k = 0; k < K; ++k)
      for (int64_t t = 0; t < B; ++t) {
        const esr::BprTriple r = esr::bpr_sample_triple(offsets.data(), upos.data(), ipos.data(), nu, (uint32_t)ni,
                                                        (uint32_t)nnz, seed, (uint32_t)step0 + (uint32_t)k, (uint32_t)t);
        printf("%d %d %d %d\n", r.u, r.i, r.j, r.valid);
      }
  }
  fclose(f);
  return 0;
}
