// Stand-alone host program over esr_bag_rule.h (no HIP, no library): reads cases from the file named on the command line
// and prints the bits of every row the header composes or expands for them.  Floats travel as their 32-bit patterns in
// hexadecimal, so nothing is rounded on the way.  A case is the whitespace-separated words
//   sum    nf D nnz n_bags n has_weight has_rows            table[nf * D] offsets[n_bags + 1] feat[nnz] {weight[nnz]} {rows[n]}
//   expand nf D nnz n_bags n has_weight has_rows has_valid reg   ... as sum ...   grad_rows[n * D] {valid[n]}
// (has_rows = 0: the bags 0 .. n - 1 in order).  It is answered by "sum n D failed" and n lines of D words, or by
// "expand M D failed" and M lines "feat word ...", M the sum of the selected bags' lengths, which the program computes
// as the caller of the kernel does.  The arrays are heap allocations of exactly the stated sizes.  Meant to be built with
// -fsanitize=address,undefined:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/bag_rule_host.cpp -o bag_host
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../esrecsys_amd/csrc/esr_bag_rule.h"

static bool read_floats(FILE* f, std::vector<float>& v) {
  for (auto& x : v) {
    uint32_t bits;
    if (fscanf(f, "%" SCNx32, &bits) != 1) return false;
    memcpy(&x, &bits, 4);
  }
  return true;
}

static void print_row(const float* row, int D) {
  for (int c = 0; c < D; ++c) {
    uint32_t bits;
    memcpy(&bits, row + c, 4);
    printf(" %08" PRIx32, bits);
  }
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
  printf("geometry %d %d %d\n", esr::kBagMaxRank, esr::kBagRankMultiple, esr::kBagFailBad);
  char what[16];
  while (fscanf(f, "%15s", what) == 1) {
    const bool expand = strcmp(what, "expand") == 0;
    if (!expand && strcmp(what, "sum") != 0) return 3;
    int64_t nf, D, nnz, n_bags, n;
    int has_weight, has_rows, has_valid = 0;
    float reg = 0.f;
    if (fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %d %d", &nf, &D, &nnz, &n_bags, &n, &has_weight,
               &has_rows) != 7)
      return 4;
    if (expand) {
      std::vector<float> r(1);
      if (fscanf(f, "%d", &has_valid) != 1 || !read_floats(f, r)) return 4;
      reg = r[0];
    }
    if (nf < 1 || D < 4 || D > esr::kBagMaxRank || D % 4 || nnz < 1 || n_bags < 1 || n < 0 || (!has_rows && n > n_bags)) {
      fprintf(stderr, "case out of range\n");
      return 3;
    }
    std::vector<float> table((size_t)(nf * D)), weight((size_t)(has_weight ? nnz : 0)), grads((size_t)(expand ? n * D : 0));
    std::vector<int64_t> offsets((size_t)n_bags + 1);
    std::vector<int32_t> feat((size_t)nnz), rows((size_t)(has_rows ? n : 0)), valid((size_t)(has_valid ? n : 0));
    if (!read_floats(f, table)) return 4;
    for (auto& v : offsets)
      if (fscanf(f, "%" SCNd64, &v) != 1) return 4;
    for (auto& v : feat)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    if (!read_floats(f, weight)) return 4;
    for (auto& v : rows)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    if (!read_floats(f, grads)) return 4;
    for (auto& v : valid)
      if (fscanf(f, "%" SCNd32, &v) != 1) return 4;
    const float* w = has_weight ? weight.data() : nullptr;
    std::vector<float> row((size_t)D);
    int failed = 0;
    if (!expand) {
      std::vector<float> out((size_t)(n * D));
      for (int64_t r = 0; r < n; ++r) {
        const int64_t b = has_rows ? (int64_t)rows[(size_t)r] : r;
        if (!esr::bag_sum_row(table.data(), nf, (int)D, offsets.data(), feat.data(), w, nnz, n_bags, b, out.data() + r * D))
          failed = esr::kBagFailBad;
      }
      printf("sum %" PRId64 " %" PRId64 " %d\n", n, D, failed);
      for (int64_t r = 0; r < n; ++r) print_row(out.data() + r * D, (int)D);
      continue;
    }
    std::vector<int64_t> oo((size_t)n + 1, 0);
    for (int64_t r = 0; r < n; ++r) {
      const int64_t b = has_rows ? (int64_t)rows[(size_t)r] : r;
      int64_t len = 0;
      if (esr::bag_number_ok(b, n_bags)) {
        const esr::BagSpan s = esr::bag_span(offsets.data(), b, nnz);
        len = s.hi - s.lo;
      } else {
        failed = esr::kBagFailBad;
      }
      oo[(size_t)r + 1] = oo[(size_t)r] + len;
    }
    const int64_t M = oo[(size_t)n];
    std::vector<int32_t> out_feat((size_t)M);
    std::vector<float> out_grads((size_t)(M * D));
    for (int64_t r = 0; r < n; ++r) {
      const int64_t b = has_rows ? (int64_t)rows[(size_t)r] : r;
      for (int64_t q = oo[(size_t)r]; q < oo[(size_t)r + 1]; ++q)
        if (!esr::bag_expand_row(table.data(), nf, (int)D, offsets.data(), feat.data(), w, nnz, n_bags, b, q - oo[(size_t)r],
                                 grads.data() + r * D, has_valid ? valid[(size_t)r] != 0 : 1, reg, &out_feat[(size_t)q],
                                 out_grads.data() + q * D))
          failed = esr::kBagFailBad;
    }
    printf("expand %" PRId64 " %" PRId64 " %d\n", M, D, failed);
    for (int64_t q = 0; q < M; ++q) {
      printf("%d", out_feat[(size_t)q]);
      print_row(out_grads.data() + q * D, (int)D);
    }
  }
  fclose(f);
  return 0;
}
