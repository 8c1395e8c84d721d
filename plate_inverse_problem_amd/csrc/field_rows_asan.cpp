// Host-only sanitizer driver of pfr::field_rows (plan.cpp) -- the validation and permutation of pfr_field_sweep's
// row selection, the one piece of host code between the caller's list and the indices k_field_gather reads X through.
// Built by `make asan-field` with -fsanitize=address,undefined (tests/test_asan_field_rows.py).
//
//   field_rows_asan <n>
// runs the selections a caller can pass on a permutation of n rows, each list in a heap block of exactly its size
// (a read past either end is an AddressSanitizer finding), and prints one line per case: "ok <n_sel> <checksum>" or
// "refused <message>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "plan.hpp"

namespace {

int run(const char* name, const std::vector<int32_t>& iperm, const std::vector<int32_t>& rows, int32_t n_rows,
        bool null_list = false) {
  // the caller's list in a block of its own size
  std::unique_ptr<int32_t[]> list(rows.empty() ? nullptr : new int32_t[rows.size()]);
  for (size_t i = 0; i < rows.size(); ++i) list[i] = rows[i];
  std::vector<int32_t> out;
  const std::string refusal = pfr::field_rows(iperm, n_rows, null_list ? nullptr : list.get(), out);
  if (!refusal.empty()) {
    std::printf("%s refused %s\n", name, refusal.c_str());
    return 0;
  }
  if ((int64_t)out.size() != n_rows) return std::printf("%s: %zu rows out for %d in\n", name, out.size(), n_rows), 1;
  uint64_t h = 1469598103934665603ull;
  for (size_t j = 0; j < out.size(); ++j) {
    if (out[j] < 0 || out[j] >= (int32_t)iperm.size() || out[j] != iperm[rows[j]])
      return std::printf("%s: entry %zu = %d\n", name, j, out[j]), 1;
    h = (h ^ (uint32_t)out[j]) * 1099511628211ull;
  }
  std::printf("%s ok %zu %llu\n", name, out.size(), (unsigned long long)h);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const int32_t n = argc > 1 ? std::atoi(argv[1]) : 97;
  if (n < 4) return std::fprintf(stderr, "usage: field_rows_asan <n >= 4>\n"), 2;
  std::vector<int32_t> iperm(n);
  for (int32_t i = 0; i < n; ++i) iperm[i] = (int32_t)(((int64_t)i * 7919 + 13) % n);   // any map into [0, n) will do
  std::vector<int32_t> all(n), desc, one{n - 1};
  for (int32_t i = 0; i < n; ++i) all[i] = i;
  for (int32_t i = n - 1; i >= 0; i -= 2) desc.insert(desc.end(), {i, i});               // descending, with repeats
  int bad = 0;
  bad += run("all", iperm, all, n);
  bad += run("one", iperm, one, 1);
  bad += run("descending", iperm, desc, (int32_t)desc.size());
  bad += run("prefix", iperm, all, n > 33 ? 33 : n / 2);      // n_rows below the block's size: only those are read
  bad += run("index_n", iperm, {0, n, 1}, 3);
  bad += run("index_minus_one", iperm, {2, 1, -1}, 3);
  bad += run("index_int_min", iperm, {INT32_MIN}, 1);
  bad += run("no_rows", iperm, {0, 1}, 0);
  bad += run("negative_count", iperm, {0, 1}, -5);
  bad += run("null_list", iperm, {}, 4, true);
  bad += run("empty_perm", {}, {0}, 1);
  return bad ? 1 : 0;
}
