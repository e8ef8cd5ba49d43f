// Stand-alone host program over esr_warp_sample.h (no HIP, no library): reads cases from the file named on the command
// line and prints what the header's warp_slot gives for every slot.  A case is the whitespace-separated integers
//   nu ni nnz D seed step B max_trials margin reg   row_offsets[nu + 1]   row_upos[nnz]   row_ipos[nnz]
//   rank_weight[ni + 1]   user_table[nu * D]   item_table[ni * D]
// with every float32 (margin, reg, rank_weight, the tables) given as the unsigned integer of its bits, and is answered by
// one line "case B" followed by B lines "u i j valid trials bits(s_i) bits(d)".  The arrays are heap allocations of
// exactly the stated sizes.  Meant to be built with -fsanitize=address,undefined:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/warp_sample_host.cpp -o warp_host
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../esrecsys_amd/csrc/esr_warp_sample.h"

static bool read_float(FILE* f, float* v) {
  uint32_t bits;
  if (fscanf(f, "%" SCNu32, &bits) != 1) return false;
  memcpy(v, &bits, 4);
  return true;
}

static uint32_t bits_of(float v) {
  uint32_t bits;
  memcpy(&bits, &v, 4);
  return bits;
}

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
  printf("max_trials %d\n", esr::kWarpMaxTrials);
  int64_t nu, ni, nnz, D, B, T;
  uint64_t seed, step;
  while (fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNd64, &nu, &ni, &nnz,
                &D, &seed, &step, &B, &T) == 8) {
    float margin, reg;
    if (!read_float(f, &margin) || !read_float(f, &reg)) return 4;
    if (nu < 1 || ni < 1 || ni > INT32_MAX || nnz < 1 || nnz > INT32_MAX || B < 1 || step > UINT32_MAX || D < 4 ||
        D > esr::kWarpMaxRank || D % esr::kWarpRankMultiple || T < 1 || T > esr::kWarpMaxTrials) {
      fprintf(stderr, "case out of range\n");
      return 3;
    }
    std::vector<int64_t> offsets((size_t)nu + 1);
    std::vector<int32_t> upos((size_t)nnz), ipos((size_t)nnz);
    std::vector<float> weight((size_t)ni + 1), user((size_t)(nu * D)), item((size_t)(ni * D)), grads((size_t)(3 * D));
    for (auto& v : offsets)
      if (fscanf(f, "%" SCNd64, &v) != 1) return 4;
    for (auto& v : upos)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    for (auto& v : ipos)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    for (auto* a : {&weight, &user, &item})
      for (auto& v : *a)
        if (!read_float(f, &v)) return 4;
    printf("case %" PRId64 "\n", B);
    for (int64_t t = 0; t < B; ++t) {
      const esr::WarpSlot r =
          esr::warp_slot(user.data(), nu, item.data(), (uint32_t)ni, (int)D, offsets.data(), upos.data(), ipos.data(),
                         (uint32_t)nnz, weight.data(), seed, (uint32_t)step, (uint32_t)t, (int)T, margin, reg, grads.data());
      printf("%d %d %d %d %d %" PRIu32 " %" PRIu32 "\n", r.u, r.i, r.j, r.valid, r.trials, bits_of(r.s_i), bits_of(r.d));
    }
  }
  fclose(f);
  return 0;
}
