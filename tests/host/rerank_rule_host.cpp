// Stand-alone host program over esr_rerank_rule.h (no HIP, no library): reads one-query cases from the file named on the
// command line and prints what the header computes for them.  Floats travel as their 32-bit patterns in hexadecimal, so
// nothing is rounded on the way.  A case is the whitespace-separated words
//   mmr ni D width n_out L lam          rows[ni * D] cand[width] rel[width]
//   ils ni D width L nk ks[nk]          rows[ni * D] cand[width]
// (L = the list's length, clamped by the header; -1 = no lengths).  It is answered by "mmr n_out length failed" and the four
// lines pos, item, rel, value, or by "ils nk failed" and the two lines ils, valid.  The arrays are heap allocations of
// exactly the stated sizes.  Meant to be built with -fsanitize=address,undefined:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/rerank_rule_host.cpp -o rerank_host
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../esrecsys_amd/csrc/esr_rerank_rule.h"

static bool read_floats(FILE* f, std::vector<float>& v) {
  for (auto& x : v) {
    uint32_t bits;
    if (fscanf(f, "%" SCNx32, &bits) != 1) return false;
    memcpy(&x, &bits, 4);
  }
  return true;
}

static bool read_ints(FILE* f, std::vector<int32_t>& v) {
  for (auto& x : v)
    if (fscanf(f, "%" SCNd32, &x) != 1) return false;
  return true;
}

static void print_floats(const std::vector<float>& v) {
  for (float x : v) {
    uint32_t bits;
    memcpy(&bits, &x, 4);
    printf(" %08" PRIx32, bits);
  }
  printf("\n");
}

static void print_ints(const std::vector<int32_t>& v) {
  for (int32_t x : v) printf(" %d", x);
  printf("\n");
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
  printf("geometry %d %d %d %d %d %d %d\n", esr::kRerankMaxRank, esr::kRerankRankMultiple, esr::kRerankMaxWidth,
         esr::kRerankMaxCutoffs, esr::kRerankFailPos, esr::kRerankFailRel, esr::kRerankStageBytes);
  char what[16];
  while (fscanf(f, "%15s", what) == 1) {
    const bool ils = strcmp(what, "ils") == 0;
    if (!ils && strcmp(what, "mmr") != 0) return 3;
    int64_t ni;
    int D, width, n_out = 1, L, nk = 1;
    if (fscanf(f, "%" SCNd64 " %d %d", &ni, &D, &width) != 3) return 4;
    if (!ils && fscanf(f, "%d", &n_out) != 1) return 4;
    if (fscanf(f, "%d", &L) != 1) return 4;
    std::vector<float> lam(1, 0.f);
    if (ils) {
      if (fscanf(f, "%d", &nk) != 1) return 4;
    } else if (!read_floats(f, lam)) {
      return 4;
    }
    if (ni < 1 || D < 4 || D > esr::kRerankMaxRank || D % 4 || width < 1 || width > esr::kRerankMaxWidth || n_out < 1 ||
        n_out > width || nk < 1 || nk > esr::kRerankMaxCutoffs || !(lam[0] >= 0.f && lam[0] <= 1.f)) {
      fprintf(stderr, "case out of range\n");
      return 3;
    }
    std::vector<int32_t> ks((size_t)(ils ? nk : 0)), cand((size_t)width);
    std::vector<float> rows((size_t)(ni * D)), rel((size_t)(ils ? 0 : width));
    if (!read_ints(f, ks) || !read_floats(f, rows) || !read_ints(f, cand) || !read_floats(f, rel)) return 4;
    const int32_t len = L;
    const int LL = esr::rerank_length(L < 0 ? nullptr : &len, 0, width);
    if (ils) {
      std::vector<float> out((size_t)nk);
      std::vector<int32_t> valid((size_t)nk);
      const int failed = esr::rerank_ils_query(rows.data(), ni, D, cand.data(), LL, ks.data(), nk, out.data(), valid.data());
      printf("ils %d %d\n", nk, failed);
      print_floats(out);
      print_ints(valid);
      continue;
    }
    std::vector<int32_t> state((size_t)width), pos((size_t)n_out), item((size_t)n_out);
    std::vector<float> m((size_t)width), orel((size_t)n_out), value((size_t)n_out);
    int32_t length = 0;
    const int failed = esr::rerank_mmr_query(rows.data(), ni, D, cand.data(), rel.data(), LL, n_out, lam[0], state.data(),
                                             m.data(), pos.data(), item.data(), orel.data(), value.data(), &length);
    printf("mmr %d %d %d\n", n_out, length, failed);
    print_ints(pos);
    print_ints(item);
    print_floats(orel);
    print_floats(value);
  }
  fclose(f);
  return 0;
}
