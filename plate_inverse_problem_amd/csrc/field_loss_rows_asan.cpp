// Host-only sanitizer driver of pfr::field_loss_rows (plan.cpp) -- the validation of pfr_field_loss_sweep's row
// selection and weights, the host code between the caller's lists and the indices k_field_terms / k_field_seed scatter
// the adjoint seed through.  Built by `make asan-field-loss` with -fsanitize=address,undefined
// (tests/test_asan_field_loss_rows.py).
//
//   field_loss_rows_asan <n>
// runs the lists a caller can pass on a permutation of n rows, each list in a heap block of exactly its size (a read
// past either end is an AddressSanitizer finding), and prints one line per case: "<name> ok <n_sel> <checksum>" or
// "<name> refused <message>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "plan.hpp"

namespace {

struct Case {
  std::vector<int32_t> rows;
  int32_t n_rows = 0;
  bool null_rows = false;
  std::vector<double> weights;
  bool null_weights = true;
  bool cotangent = false;
};

int run(const char* name, const std::vector<int32_t>& iperm, const Case& c) {
  // the caller's lists in blocks of their own size
  std::unique_ptr<int32_t[]> rows(c.rows.empty() ? nullptr : new int32_t[c.rows.size()]);
  for (size_t i = 0; i < c.rows.size(); ++i) rows[i] = c.rows[i];
  std::unique_ptr<double[]> wts(c.weights.empty() ? nullptr : new double[c.weights.size()]);
  for (size_t i = 0; i < c.weights.size(); ++i) wts[i] = c.weights[i];
  std::vector<int32_t> out{7, 7, 7};   // stale content: cleared or replaced by the call
  const std::string refusal = pfr::field_loss_rows(iperm, c.n_rows, c.null_rows ? nullptr : rows.get(),
                                                   c.null_weights ? nullptr : wts.get(), c.cotangent, out);
  if (!refusal.empty()) {
    if (!out.empty()) return std::printf("%s: %zu rows out with a refusal\n", name, out.size()), 1;
    std::printf("%s refused %s\n", name, refusal.c_str());
    return 0;
  }
  const size_t want = c.null_rows ? 0 : (size_t)c.n_rows;   // all rows: the list stays empty (the caller walks iperm)
  if (out.size() != want) return std::printf("%s: %zu rows out for %zu\n", name, out.size(), want), 1;
  uint64_t h = 1469598103934665603ull;
  for (size_t j = 0; j < out.size(); ++j) {
    if (out[j] < 0 || out[j] >= (int32_t)iperm.size() || out[j] != iperm[c.rows[j]])
      return std::printf("%s: entry %zu = %d\n", name, j, out[j]), 1;
    h = (h ^ (uint32_t)out[j]) * 1099511628211ull;
  }
  std::printf("%s ok %zu %llu\n", name, c.null_rows ? iperm.size() : out.size(), (unsigned long long)h);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const int32_t n = argc > 1 ? std::atoi(argv[1]) : 97;
  if (n < 4) return std::fprintf(stderr, "usage: field_loss_rows_asan <n >= 4>\n"), 2;
  std::vector<int32_t> iperm(n);
  for (int32_t i = 0; i < n; ++i) iperm[i] = (int32_t)(((int64_t)i * 7919 + 13) % n);   // any map into [0, n) will do
  std::vector<int32_t> all(n), desc;
  for (int32_t i = 0; i < n; ++i) all[i] = i;
  for (int32_t i = n - 1; i >= 0; i -= 2) desc.push_back(i);                             // descending, distinct
  std::vector<double> ones(n, 1.0), ramp(n), zeros(n, 0.0), one_left(n, 0.0), neg(n, 0.5), nan(n, 0.5), inf(n, 0.5);
  for (int32_t i = 0; i < n; ++i) ramp[i] = 0.25 + (double)(i % 7);
  one_left[n - 1] = 1e-300;
  neg[n / 2] = -1e-300;
  nan[n - 1] = std::nan("");
  inf[0] = std::numeric_limits<double>::infinity();
  const int32_t nd = (int32_t)desc.size(), np = n > 33 ? 33 : n / 2;
  auto first = [](const std::vector<double>& v, int32_t k) { return std::vector<double>(v.begin(), v.begin() + k); };
  int bad = 0;
  // valid lists
  bad += run("all", iperm, {.rows = all, .n_rows = n});
  bad += run("null_rows", iperm, {.n_rows = -7, .null_rows = true});
  bad += run("null_rows_weights", iperm, {.null_rows = true, .weights = ramp, .null_weights = false});
  bad += run("one", iperm, {.rows = {n - 1}, .n_rows = 1, .weights = {2.0}, .null_weights = false});
  bad += run("descending", iperm, {.rows = desc, .n_rows = nd, .weights = first(ramp, nd), .null_weights = false});
  bad += run("prefix", iperm, {.rows = all, .n_rows = np, .weights = first(ones, np), .null_weights = false});
  bad += run("one_weight_left", iperm, {.rows = all, .n_rows = n, .weights = one_left, .null_weights = false});
  bad += run("cotangent", iperm, {.rows = desc, .n_rows = nd, .cotangent = true});
  // repeats
  bad += run("repeat_adjacent", iperm, {.rows = {0, 1, 1, 2}, .n_rows = 4});
  bad += run("repeat_ends", iperm, {.rows = {n - 1, 0, 2, n - 1}, .n_rows = 4});
  std::vector<int32_t> twice(all);
  twice.push_back(n / 2);
  bad += run("repeat_after_all", iperm, {.rows = twice, .n_rows = n + 1});
  // rows out of range
  bad += run("index_n", iperm, {.rows = {0, n, 1}, .n_rows = 3});
  bad += run("index_minus_one", iperm, {.rows = {2, 1, -1}, .n_rows = 3});
  bad += run("index_int_min", iperm, {.rows = {INT32_MIN}, .n_rows = 1});
  bad += run("index_int_max", iperm, {.rows = {0, INT32_MAX}, .n_rows = 2});
  // empty lists
  bad += run("no_rows", iperm, {.rows = {0, 1}, .n_rows = 0});
  bad += run("negative_count", iperm, {.rows = {0, 1}, .n_rows = -5});
  bad += run("empty_perm", {}, {.null_rows = true});
  bad += run("empty_perm_row", {}, {.rows = {0}, .n_rows = 1});
  // weights
  bad += run("weights_zero", iperm, {.rows = all, .n_rows = n, .weights = zeros, .null_weights = false});
  bad += run("weights_zero_selected", iperm, {.rows = {0, 1}, .n_rows = 2, .weights = {0.0, 0.0}, .null_weights = false});
  bad += run("weight_negative", iperm, {.null_rows = true, .weights = neg, .null_weights = false});
  bad += run("weight_nan", iperm, {.rows = all, .n_rows = n, .weights = nan, .null_weights = false});
  bad += run("weight_inf", iperm, {.rows = all, .n_rows = n, .weights = inf, .null_weights = false});
  bad += run("weights_cotangent", iperm, {.rows = all, .n_rows = n, .weights = ones, .null_weights = false, .cotangent = true});
  return bad ? 1 : 0;
}
