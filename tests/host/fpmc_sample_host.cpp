// Stand-alone host program over esr_fpmc_sample.h (no HIP, no library): reads cases from the file named on the command
// line and prints every slot the header draws for them.  A case is the whitespace-separated integers
//   nu ni nnz_seq nnz_seen window seed step0 K B   seq_offsets[nu + 1]   seq_upos[nnz_seq]   seq_ipos[nnz_seq]
//   row_offsets[nu + 1]   row_ipos[nnz_seen]
// and is answered by one line "case K B" followed by K * B lines "u e c i j valid" (step-major, slot-minor).  The arrays
// are heap allocations of exactly the stated sizes.  Meant to be built with -fsanitize=address,undefined:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/fpmc_sample_host.cpp -o fpmc_host
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../esrecsys_amd/csrc/esr_fpmc_sample.h"

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
  printf("max_window %d max_tries %d\n", esr::kFpmcMaxWindow, esr::kBprMaxTries);
  int64_t nu, ni, nnz_seq, nnz_seen, window, K, B;
  uint64_t seed, step0;
  while (fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNd64,
                &nu, &ni, &nnz_seq, &nnz_seen, &window, &seed, &step0, &K, &B) == 9) {
    if (nu < 1 || ni < 1 || ni > INT32_MAX || nnz_seq < 1 || nnz_seq > INT32_MAX || nnz_seen < 1 || nnz_seen > INT32_MAX ||
        window < 1 || window > esr::kFpmcMaxWindow || K < 1 || B < 1 || step0 > UINT32_MAX) {
      fprintf(stderr, "case out of range\n");
      return 3;
    }
    std::vector<int64_t> seq_offsets((size_t)nu + 1), row_offsets((size_t)nu + 1);
    std::vector<int32_t> seq_upos((size_t)nnz_seq), seq_ipos((size_t)nnz_seq), row_ipos((size_t)nnz_seen);
    for (auto& v : seq_offsets)
      if (fscanf(f, "%" SCNd64, &v) != 1) return 4;
    for (auto& v : seq_upos)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    for (auto& v : seq_ipos)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    for (auto& v : row_offsets)
      if (fscanf(f, "%" SCNd64, &v) != 1) return 4;
    for (auto& v : row_ipos)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    printf("case %" PRId64 " %" PRId64 "\n", K, B);
    for (int64_t k = 0; k < K; ++k)
      for (int64_t t = 0; t < B; ++t) {
        const esr::FpmcSlot r = esr::fpmc_sample_slot(seq_offsets.data(), seq_upos.data(), seq_ipos.data(), (uint32_t)nnz_seq,
                                                      row_offsets.data(), row_ipos.data(), nnz_seen, nu, (uint32_t)ni,
                                                      (int)window, seed, (uint32_t)step0 + (uint32_t)k, (uint32_t)t);
        printf("%d %d %d %d %d %d\n", r.u, r.e, r.c, r.i, r.j, r.valid);
      }
  }
  fclose(f);
  return 0;
}
