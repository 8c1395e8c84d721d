// Host-only driver of the symbolic analysis and the launch plans for sanitizer builds (`make asan-host`: g++
// with -fsanitize=address,undefined; no HIP).  The C ABI's pfr_symbolic_create runs exactly this pfr::analyse
// and pfr_solver_create this pfr::build_plan (api.cpp); tests/test_asan_host.py feeds it the plate patterns with
// every ordering option the engine uses, compares the statistics with libpfr's, and has every plan checked
// (pfr::check_plan) for every engine shape: chunks of 64 .. 4,096 frequencies (one or two lanes split a sweep
// into such chunks), Schur block thresholds and solve split targets.  For each shape it also builds the launch
// schedule (pfr::level_schedule, the records the level loops launch) under the environment's knobs, once with every
// front reached and once with the reach of a single leaf row, and has every record checked (pfr::check_schedule).
// Pruning's views go through the same checks for every shape: with a load on one leaf row (the trees
// pfr::loaded_fronts marks for it) the plan and schedule of the loaded trees and of the rest, their reaches the
// load's and the support's rows on each.  `symbolic_asan --forest` runs all of it on a built-in forest of three
// trees (load in the first, sensor rows in the first two) and prints "forest ok <plans checked>"; before that, on two
// forests of two clique trees whose first tree's leaves fit the fused bottom level (fused_forest: the second tree's do
// not / do too), it has both views follow the full plan's decision for level 0, loaded on either tree.
//
// Input file (little-endian): int32 n, int64 nnz, int32 colptr[n + 1], int32 rowind[nnz],
// int32 n_last, int32 last[n_last].  Each further argument is one option set
// "leaf,ordering,symmetric,max_ns,md_delta,use_last"; per set one output line:
// "n_fronts n_levels max_front total_rows nnz_lu factor_flops perm_hash n_dirichlet n_coupling", then one line
// "plan ok <plans checked>" or "plan error <shape>: <violation>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "plan.hpp"
#include "symbolic.hpp"

namespace {
template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}

// Pruning's two views for a load on `load_row` (permuted) and the sensor rows `sup`: plans built with blk_min bm, then
// every index and record checked for chunk Fc under the knobs k.  Returns "" or the first violation.  *split: some
// tree is unloaded (the views differ from the full plan).
struct Views {
  pfr::Plan P[2];
  std::vector<char> mask[2];
  std::vector<int32_t> full_ptr[2], ptr[2][2];
};
std::string build_views(const pfr::Symbolic& S, int bm, int32_t load_row, const std::vector<int32_t>& sup,
                        const std::vector<int32_t>& foc, const std::vector<int32_t>& par, Views& V) {
  std::vector<double> rhs(S.n, 0.0);
  rhs[load_row] = 1.0;
  V.mask[0] = pfr::loaded_fronts(S, rhs.data());
  V.mask[1] = V.mask[0];
  for (char& m : V.mask[1]) m = !m;
  if (!V.mask[0][foc[load_row]]) return "the loaded row's front is not loaded";
  std::vector<int32_t> rows[2] = {{load_row}, sup}, mark, list;
  for (size_t c = 0; c < S.cpl_p.size(); ++c) rows[0].push_back(S.cpl_p[c]);   // pfr_set_rhs: every coupled row
  for (int w = 0; w < 2; ++w) pfr::reach_lists(foc, par, S.level_ptr, S.level_fronts, rows[w], mark, list, V.full_ptr[w]);
  std::string err;
  for (int side = 0; side < 2; ++side) {
    if (pfr::build_plan(S, bm, V.P[side], err, &V.mask[side])) return err;
    for (int w = side; w < 2; ++w)   // the rest carries no load: no forward reach
      pfr::reach_lists(foc, par, V.P[side].level_ptr, V.P[side].level_fronts, pfr::rows_in(S, V.mask[side], rows[w]), mark,
                       list, V.ptr[side][w]);
  }
  // the two views partition the fronts, level by level
  for (size_t l = 0; l + 1 < S.level_ptr.size(); ++l)
    if (V.P[0].level_ptr[l + 1] - V.P[0].level_ptr[l] + V.P[1].level_ptr[l + 1] - V.P[1].level_ptr[l] !=
        S.level_ptr[l + 1] - S.level_ptr[l])
      return "views do not partition a level";
  // the live stiffness matrices of each view's walk (pfr::live_stiffness): matrix 0 with values on the loaded trees'
  // rows only, matrix 1 on the other rows only, matrix 2 nowhere
  std::vector<double> stiff(3 * S.nnz, 0.0);
  bool any[2] = {false, false};
  for (int64_t e = 0; e < S.nnz; ++e) {
    const int side = V.mask[0][foc[S.prow[e]]] ? 0 : 1;
    stiff[3 * e + side] = 1.0 + e;
    any[side] = true;
  }
  const std::vector<uint32_t> bits = pfr::stiffness_bits(stiff.data(), S.nnz, 3);
  for (int side = 0; side < 2; ++side)
    if (pfr::live_stiffness(S, &V.mask[side], bits) != (any[side] ? 1u << side : 0u)) return "live stiffness list of a view";
  if (pfr::live_stiffness(S, nullptr, bits) != ((any[0] ? 1u : 0u) | (any[1] ? 2u : 0u))) return "live stiffness list";
  // the inertia contraction's entry lists (pfr::mass_entries) for the same table as mass components: the two views'
  // lists partition the full one, every entry on the wave that owns it there, each run padded to whole batches
  const pfr::Plan& P0 = V.P[0];
  const std::vector<char> on = pfr::mass_on(stiff.data(), S.nnz, 3);
  const pfr::MassList full = pfr::mass_entries(P0.uent, P0.n_uent, S.n, nullptr, on);
  if (full.n_list != (int)S.nnz || full.list.size() % pfr::MASS_U) return "mass list";
  std::vector<int32_t> wave_of(P0.n_uent, -1);
  for (size_t w = 0; w + 1 < full.ptr.size(); ++w)
    for (int64_t i = (int64_t)full.ptr[w] * pfr::MASS_U; i < (int64_t)full.ptr[w + 1] * pfr::MASS_U; ++i)
      if (full.list[i] >= 0) wave_of[full.list[i]] = (int32_t)w;
  int listed = 0;
  for (int side = 0; side < 2; ++side) {
    const std::vector<char> rows = pfr::front_rows(S, V.mask[side]);
    const pfr::MassList L = pfr::mass_entries(P0.uent, P0.n_uent, S.n, &rows, on);
    if (L.ptr.size() != full.ptr.size() || (int64_t)L.ptr.back() * pfr::MASS_U != (int64_t)L.list.size()) return "mass list of a view";
    for (size_t w = 0; w + 1 < L.ptr.size(); ++w)
      for (int64_t i = (int64_t)L.ptr[w] * pfr::MASS_U; i < (int64_t)L.ptr[w + 1] * pfr::MASS_U; ++i) {
        const int32_t e = L.list[i];
        if (e < 0) continue;
        if (e >= P0.n_uent || wave_of[e] != (int32_t)w || !rows[P0.uent[e].w]) return "mass list entry of a view";
        ++listed;
      }
    if (listed != (side == 0 ? L.n_list : full.n_list)) return "mass list count of a view";
  }
  return "";
}
std::string check_views(const pfr::Symbolic& S, const Views& V, int64_t Fc, const pfr::Knobs& k) {
  for (int side = 0; side < 2; ++side) {
    std::string e = pfr::check_plan(S, V.P[side], Fc);
    if (e.empty()) e = pfr::check_schedule(S, V.P[side], pfr::level_schedule(S, V.P[side], Fc, k, V.ptr[side], &V.full_ptr));
    if (!e.empty()) return std::string(side == 0 ? "loaded view: " : "unloaded view: ") + e;
  }
  return "";
}

// Two trees of cliques (of ms[k][i] nodes) fully coupled to a dense border of s[k] nodes each, the first tree's border
// eliminated last: its leaves fit the fused bottom level (at most F0_NS pivots and F0_RM update rows).  `big`: the
// second tree's leaves do not, so the full plan does not fuse level 0 and neither view may -- the bottom level is
// decided for the whole analysis; otherwise both fit, and the full plan and both views fuse, each view listing its own
// fronts.  Returns "" or the first violation; the views also go through check_views.
std::string fused_forest(bool big) {
  const std::vector<int> ms[2] = {{1, 2, 3, 4, 4}, big ? std::vector<int>{3, 6, 9} : std::vector<int>{2, 2, 4}};
  const int s[2] = {10, big ? 12 : 6};
  std::vector<std::vector<int32_t>> col;
  int32_t border0 = 0;
  for (int k = 0, o = 0; k < 2; ++k) {
    int m_all = 0;
    for (int m : ms[k]) m_all += m;
    const int nb = m_all + s[k], b0 = o + m_all;
    col.resize(o + nb);
    for (int c0 = o, i = 0; i < (int)ms[k].size(); c0 += ms[k][i++])
      for (int a = c0; a < c0 + ms[k][i]; ++a) {
        for (int b = c0; b < c0 + ms[k][i]; ++b) col[a].push_back(b);
        for (int b = b0; b < o + nb; ++b) col[a].push_back(b), col[b].push_back(a);
      }
    for (int a = b0; a < o + nb; ++a)
      for (int b = b0; b < o + nb; ++b) col[a].push_back(b);
    if (k == 0) border0 = b0;
    o += nb;
  }
  std::vector<int32_t> colptr(1, 0), rowind;
  for (auto& c : col) {
    std::sort(c.begin(), c.end());
    rowind.insert(rowind.end(), c.begin(), c.end());
    colptr.push_back((int32_t)rowind.size());
  }
  const int n = (int)col.size();
  pfr::SymbolicOptions o;
  o.symmetric = 1;
  for (int i = 0; i < s[0]; ++i) o.last.push_back(border0 + i);
  pfr::Symbolic S;
  if (pfr::analyse(n, (int64_t)rowind.size(), colptr.data(), rowind.data(), o, S) != 0) return S.error;
  std::vector<int32_t> foc(S.n, -1), par;
  for (size_t t = 0; t < S.fronts.size(); ++t) {
    par.push_back(S.fronts[t].parent);
    for (int a = 0; a < S.fronts[t].ns; ++a) foc[S.fronts[t].col0 + a] = (int32_t)t;
  }
  const int first1 = border0 + s[0];   // the second tree's first node
  pfr::Plan P;
  std::string err;
  if (pfr::build_plan(S, 24, P, err)) return err;
  if (P.fused0 != !big) return "full plan: fused bottom level";
  for (int loaded = 0; loaded < 2; ++loaded) {
    Views V;
    std::string e = build_views(S, 24, S.iperm[loaded ? first1 : 0], {S.iperm[border0], S.iperm[n - 1]}, foc, par, V);
    if (!e.empty()) return e;
    // the view of the first tree alone holds only fronts that fit: it must still follow the full plan
    int fit = 0, n0 = 0;
    const pfr::Plan& first = V.P[loaded];
    for (int e0 = first.level_ptr[0]; e0 < first.level_ptr[1]; ++e0, ++n0) {
      const pfr::Front& F = S.fronts[first.level_fronts[e0]];
      fit += F.ns <= pfr::F0_NS && F.f - F.ns <= pfr::F0_RM;
    }
    if (n0 == 0 || fit != n0) return "the first tree's leaves do not all fit the fused bottom level";
    for (int side = 0; side < 2; ++side)
      if (V.P[side].fused0 != P.fused0) return side == loaded ? "first tree's view: fused bottom level" : "second tree's view: fused bottom level";
    if (P.fused0 && V.P[0].f0_front.size() + V.P[1].f0_front.size() != P.f0_front.size()) return "views do not partition the fused fronts";
    for (int64_t Fc : {64, 512})
      for (int front0 : {1, 0}) {
        pfr::Knobs k = pfr::knobs_from_env(Fc);
        k.front0 = front0;
        e = check_views(S, V, Fc, k);
        if (!e.empty()) return e;
      }
  }
  return "";
}

// three tridiagonal blocks of 40, 33 and 21 nodes: a forest of three elimination trees
int forest() {
  for (int big = 0; big < 2; ++big) {
    const std::string e = fused_forest(big != 0);
    if (!e.empty()) {
      printf("forest error fused bottom level (%s second tree): %s\n", big ? "large" : "small", e.c_str());
      return 1;
    }
  }
  const int sizes[3] = {40, 33, 21};
  std::vector<int32_t> colptr(1, 0), rowind;
  for (int b = 0, o = 0; b < 3; o += sizes[b++])
    for (int j = 0; j < sizes[b]; ++j) {
      for (int i = std::max(0, j - 1); i <= std::min(sizes[b] - 1, j + 1); ++i) rowind.push_back(o + i);
      colptr.push_back((int32_t)rowind.size());
    }
  const int n = (int)colptr.size() - 1;
  int checked = 0;
  for (int leaf : {4, 16, 10000}) {
    pfr::SymbolicOptions o;
    o.leaf_size = leaf;
    o.symmetric = 1;
    pfr::Symbolic S;
    if (pfr::analyse(n, (int64_t)rowind.size(), colptr.data(), rowind.data(), o, S) != 0) {
      printf("forest error %s\n", S.error.c_str());
      return 1;
    }
    std::vector<int32_t> foc(S.n, -1), par;
    for (size_t t = 0; t < S.fronts.size(); ++t) {
      par.push_back(S.fronts[t].parent);
      for (int a = 0; a < S.fronts[t].ns; ++a) foc[S.fronts[t].col0 + a] = (int32_t)t;
    }
    const std::vector<int32_t> sup = {S.iperm[3], S.iperm[17], S.iperm[45], S.iperm[60]};   // trees 0, 0, 1, 1
    for (int bm : {24, 0, 4}) {
      Views V;
      std::string e = build_views(S, bm, S.iperm[7], sup, foc, par, V);
      // the loaded view is exactly tree 0: the fronts whose pivots are among the first block's nodes
      for (size_t t = 0; t < S.fronts.size() && e.empty(); ++t)
        if ((V.mask[0][t] != 0) != (S.perm[S.fronts[t].col0] < sizes[0])) e = "loaded mask is not the first tree";
      // the reaches: the loaded view holds the load's and its sensor rows' fronts, the rest no forward reach and the
      // second tree's sensor rows' fronts; together they are the full reaches (the third tree has no sensor row)
      if (e.empty()) {
        auto total = [](const std::vector<int32_t>& p) { return p.empty() ? 0 : p.back(); };
        // the fronts holding the rows and their ancestors, counted by walking the tree
        auto reached = [&](std::initializer_list<int32_t> rows) {
          std::vector<char> seen(S.fronts.size(), 0);
          int n_seen = 0;
          for (int32_t p : rows)
            for (int t = foc[p]; t >= 0 && !seen[t]; t = par[t]) seen[t] = 1, ++n_seen;
          return n_seen;
        };
        if (total(V.ptr[0][0]) != reached({S.iperm[7]}) || total(V.ptr[1][0]) != 0 ||
            total(V.ptr[0][1]) != reached({S.iperm[3], S.iperm[17]}) ||
            total(V.ptr[1][1]) != reached({S.iperm[45], S.iperm[60]}) ||
            total(V.ptr[0][1]) + total(V.ptr[1][1]) != total(V.full_ptr[1]))
          e = "reaches of the views are not the loaded tree's rows and the second tree's";
      }
      for (int64_t Fc : {64, 512, 2048})
        for (int sp : {256, 0, 1000000}) {
          pfr::Knobs k = pfr::knobs_from_env(Fc);
          k.blk_min = bm;
          k.split_target = sp;
          if (e.empty()) e = check_views(S, V, Fc, k);
          if (!e.empty()) {
            printf("forest error leaf=%d blk_min=%d Fc=%lld split=%d: %s\n", leaf, bm, (long long)Fc, sp, e.c_str());
            return 1;
          }
          ++checked;
        }
    }
  }
  printf("forest ok %d\n", checked);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::string(argv[1]) == "--forest") return forest();
  if (argc < 3) {
    fprintf(stderr, "usage: %s pattern.bin leaf,ordering,symmetric,max_ns,md_delta,use_last ...\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0, n_last = 0;
  int64_t nnz = 0;
  if (!rd(f, &n, 1) || !rd(f, &nnz, 1) || n <= 0 || nnz < 0) return 2;
  std::vector<int32_t> colptr(n + 1), rowind(nnz);
  if (!rd(f, colptr.data(), colptr.size()) || (nnz && !rd(f, rowind.data(), rowind.size())) || !rd(f, &n_last, 1))
    return 2;
  std::vector<int32_t> last(n_last);
  if (n_last && !rd(f, last.data(), last.size())) return 2;
  fclose(f);
  for (int a = 2; a < argc; ++a) {
    int leaf, ordering, symmetric, max_ns, md_delta, use_last;
    if (sscanf(argv[a], "%d,%d,%d,%d,%d,%d", &leaf, &ordering, &symmetric, &max_ns, &md_delta, &use_last) != 6)
      return 2;
    pfr::SymbolicOptions o;
    o.leaf_size = leaf;
    o.ordering = ordering;
    o.symmetric = symmetric;
    o.max_ns = max_ns;
    o.md_delta = md_delta;
    if (use_last) o.last.assign(last.begin(), last.end());
    pfr::Symbolic S;
    if (pfr::analyse(n, nnz, colptr.data(), rowind.data(), o, S) != 0) {
      printf("error %s\n", S.error.c_str());
      continue;
    }
    uint64_t h = 1469598103934665603ull;   // FNV-1a over the permutation
    for (int32_t v : S.perm) h = (h ^ (uint32_t)v) * 1099511628211ull;
    printf("%d %d %d %lld %lld %.17g %llu %d %d\n", (int)S.fronts.size(), (int)S.level_ptr.size() - 1, S.max_front,
           (long long)S.total_rows, (long long)S.nnz_lu, S.factor_flops, (unsigned long long)h, (int)S.dir_p.size(),
           (int)S.cpl_p.size());
    // launch plans of every engine shape
    int checked = 0;
    std::string err;
    std::vector<int32_t> foc(S.n, -1), par, rows, mark, list, ptr;   // reach lists: front of each pivot column, parents
    for (size_t t = 0; t < S.fronts.size(); ++t) {
      par.push_back(S.fronts[t].parent);
      for (int a = 0; a < S.fronts[t].ns; ++a) foc[S.fronts[t].col0 + a] = (int32_t)t;
    }
    // the reaches the schedules are built for: every front, and the ancestors of one leaf row
    pfr::reach_lists(foc, par, S.level_ptr, S.level_fronts, {S.fronts[S.level_fronts[0]].col0}, mark, list, ptr);
    const std::vector<int32_t> reach_all[2] = {S.level_ptr, S.level_ptr}, reach_leaf[2] = {ptr, ptr};
    const int blk_mins[] = {24, 0, 4};
    const int splits[] = {256, 0, 1000000};
    const int64_t chunks[] = {64, 512, 1024, 2048, 4096};
    for (int bm : blk_mins) {
      pfr::Plan P;
      if (pfr::build_plan(S, bm, P, err)) {
        printf("plan error blk_min=%d: %s\n", bm, err.c_str());
        goto next;
      }
      // pruning's views (symmetric analyses): a load on one leaf row, the support (or every 97th row) as sensor rows
      Views V;
      if (S.symmetric) {
        std::vector<int32_t> sup;
        for (int32_t v : last) sup.push_back(S.iperm[v]);
        for (int i = 0; i < S.n && last.empty(); i += 97) sup.push_back(i);
        err = build_views(S, bm, S.fronts[S.level_fronts[0]].col0, sup, foc, par, V);
        if (!err.empty()) {
          printf("plan error blk_min=%d views: %s\n", bm, err.c_str());
          goto next;
        }
      }
      for (int64_t Fc : chunks)
        for (int sp : splits) {
          pfr::Knobs k = pfr::knobs_from_env(Fc);
          k.blk_min = bm;
          k.split_target = sp;
          std::string e = pfr::check_plan(S, P, Fc);
          for (const auto& reach : {&reach_all, &reach_leaf})
            if (e.empty()) e = pfr::check_schedule(S, P, pfr::level_schedule(S, P, Fc, k, *reach));
          if (e.empty() && S.symmetric) e = check_views(S, V, Fc, k);
          if (!e.empty()) {
            printf("plan error blk_min=%d Fc=%lld split=%d: %s\n", bm, (long long)Fc, sp, e.c_str());
            goto next;
          }
          ++checked;
        }
    }
    {
      // reach lists of the loss support (the last nodes, when given) and of every 97th row
      for (int32_t v : last) rows.push_back(S.iperm[v]);
      for (int i = 0; i < S.n; i += 97) rows.push_back(i);
      pfr::reach_lists(foc, par, S.level_ptr, S.level_fronts, rows, mark, list, ptr);
      if ((int)ptr.size() != (int)S.level_ptr.size() || ptr.back() != (int32_t)list.size()) {
        printf("plan error reach lists\n");
        goto next;
      }
    }
    printf("plan ok %d\n", checked);
  next:;
  }
  return 0;
}
