// Stand-alone host program over esr_sgns_sample.h (no HIP, no library): reads cases from the file named on the command
// line and prints every slot the header draws for them.  A case is the whitespace-separated integers
//   nd ni nnz_seq window negatives seed step0 K B   seq_offsets[nd + 1]   seq_upos[nnz_seq]   seq_ipos[nnz_seq]
//   noise_keep[ni]   noise_alias[ni]
// and is answered by one line "case K B" followed by K * B lines "c e o valid n_0 .. n_{negatives - 1}" (step-major,
// slot-minor).  The arrays are heap allocations of exactly the stated sizes.  Meant to be built with
// -fsanitize=address,undefined:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/sgns_sample_host.cpp -o sgns_host
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../esrecsys_amd/csrc/esr_sgns_sample.h"

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
  printf("max_window %d max_negatives %d\n", esr::kSgnsMaxWindow, esr::kSgnsMaxNegatives);
  int64_t nd, ni, nnz_seq, window, negatives, K, B;
  uint64_t seed, step0;
  while (fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNd64,
                &nd, &ni, &nnz_seq, &window, &negatives, &seed, &step0, &K, &B) == 9) {
    if (nd < 1 || ni < 1 || ni > INT32_MAX || nnz_seq < 1 || nnz_seq > INT32_MAX || window < 1 ||
        window > esr::kSgnsMaxWindow || negatives < 1 || negatives > esr::kSgnsMaxNegatives || K < 1 || B < 1 ||
        step0 > UINT32_MAX) {
      fprintf(stderr, "case out of range\n");
      return 3;
    }
    std::vector<int64_t> seq_offsets((size_t)nd + 1);
    std::vector<int32_t> seq_upos((size_t)nnz_seq), seq_ipos((size_t)nnz_seq), alias((size_t)ni), neg((size_t)negatives);
    std::vector<uint32_t> keep((size_t)ni);
    for (auto& v : seq_offsets)
      if (fscanf(f, "%" SCNd64, &v) != 1) return 4;
    for (auto& v : seq_upos)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    for (auto& v : seq_ipos)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    for (auto& v : keep)
      if (fscanf(f, "%" SCNu32, &v) != 1) return 4;
    for (auto& v : alias)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    printf("case %" PRId64 " %" PRId64 "\n", K, B);
    for (int64_t k = 0; k < K; ++k)
      for (int64_t t = 0; t < B; ++t) {
        const esr::SgnsSlot r = esr::sgns_sample_slot(seq_offsets.data(), seq_upos.data(), seq_ipos.data(), (uint32_t)nnz_seq,
                                                      nd, (uint32_t)ni, (int)window, (int)negatives, keep.data(), alias.data(),
                                                      seed, (uint32_t)step0 + (uint32_t)k, (uint32_t)t, neg.data());
        printf("%d %d %d %d", r.c, r.e, r.o, r.valid);
        for (int32_t v : neg) printf(" %d", v);
        printf("\n");
      }
  }
  fclose(f);
  return 0;
}
