// Host-side launch plans (plan.hpp): built by pfr_solver_create (api.cpp) and, under AddressSanitizer /
// UndefinedBehaviorSanitizer, by the host driver (asan_driver.cpp).  HIP-free.
#include "plan.hpp"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <utility>

namespace pfr {

Workspace workspace(const Symbolic& S, int64_t Fc, int n_crow) {
  Workspace w;
  const int64_t n = S.n;
  w.F = S.factor_entries * Fc;
  w.WV = S.total_rows * Fc;
  w.nvec = n * Fc;
  w.n_nvec = 7;                                             // X, Y, XA, G, Y2, XR, Gx (the refinement's seed)
  w.cpart = (int64_t)residual_parts(S.n) * Fc;             // k_residual: one partial per (workgroup, frequency)
  w.kpart = (int64_t)residual_parts(S.n) * 18 * Fc;        // ... and per stiffness matrix (contraction in the walk)
  w.berr_acc = 2 * Fc;
  w.gind = Fc / 64;
  w.Bc = (int64_t)std::max(1, n_crow) * Fc;
  if (S.symmetric) {                                        // functional from the bottom-up passes
    w.WVk = 3 * S.total_rows * Fc;
    w.YVk = 2 * n * Fc;
    w.fn_parts = 3 * (int64_t)FN_PARTS_HOST * Fc;
    w.fcoef = 3 * Fc;
  }
  int64_t b = 16 * (w.F + w.WV + w.n_nvec * w.nvec + w.cpart + w.kpart + w.WVk + w.YVk + w.fn_parts + w.fcoef + w.Bc);
  b += Fc * (8 + 8 + 4 + 16) + Fc * (8 + 16) + 8 * (w.berr_acc + w.gind);   // freqs, loss, flags, tq; fr0, mscale
  w.bytes = b;
  return w;
}

namespace {

// children's update-matrix entries per A22 position of front t: the first densely (r x r, -1 none), the rare
// further ones (two or more children covering a position) sorted aside as (i r + j, element id)
void a22_sources(const Symbolic& S, const std::vector<std::vector<int>>& kids, int t, bool sym,
                 std::vector<int32_t>& first, std::vector<std::pair<int32_t, int32_t>>& more) {
  const Front& F = S.fronts[t];
  const int r = F.f - F.ns;
  first.assign((size_t)r * r, -1);
  more.clear();
  for (int c : kids[t]) {
    const Front& C = S.fronts[c];
    const int32_t* rp = S.relpos.data() + C.row0;
    for (int a = C.ns; a < C.f; ++a) {
      const int i = rp[a] - F.ns;
      if (i < 0) continue;
      for (int b = C.ns; b < C.f; ++b) {
        const int j = rp[b] - F.ns;
        if (j < 0 || (sym && j > i)) continue;   // symmetric: lower triangle only
        const int32_t id = (int32_t)(C.off + (int64_t)a * C.f + b);
        int32_t& f1 = first[(size_t)i * r + j];
        if (f1 < 0)
          f1 = id;
        else
          more.emplace_back(i * r + j, id);
      }
    }
  }
  std::sort(more.begin(), more.end());
}

template <class F>
void each_more(const std::vector<std::pair<int32_t, int32_t>>& more, int32_t key, F&& fn) {
  auto lo = std::lower_bound(more.begin(), more.end(), std::make_pair(key, INT32_MIN));
  for (; lo != more.end() && lo->first == key; ++lo) fn(lo->second);
}

}  // namespace

int build_plan(const Symbolic& S, int blk_min, Plan& P, std::string& err, const std::vector<char>* mask) {
  P = Plan();
  if (S.max_front > MAX_FRONT) {
    err = "front larger than MAX_FRONT (plan.hpp)";
    return 1;
  }
  if (S.factor_entries > INT32_MAX) {
    err = "front storage exceeds int32 element ids";
    return 1;
  }
  const bool sym = S.symmetric != 0;
  const int L = (int)S.level_ptr.size() - 1;
  const int nfr = (int)S.fronts.size();
  P.L = L;
  P.sym = sym;
  if (mask) {
    if ((int)mask->size() != nfr) {
      err = "front mask size";
      return 1;
    }
    for (int t = 0; t < nfr; ++t)
      if (S.fronts[t].parent >= 0 && (*mask)[t] != (*mask)[S.fronts[t].parent]) {
        err = "front mask splits a tree";
        return 1;
      }
    P.active = *mask;
  } else {
    P.active.assign(nfr, 1);
  }
  P.level_maxns.assign(L, 0);
  P.level_maxf.assign(L, 0);
  P.dec_maxns.assign(L, 0);
  P.dec_maxf.assign(L, 0);
  P.level_ptr.assign(1, 0);
  P.dec_nitems.assign(L, 0);
  for (int l = 0; l < L; ++l) {
    P.dec_nf.push_back(S.level_ptr[l + 1] - S.level_ptr[l]);
    for (int e = S.level_ptr[l]; e < S.level_ptr[l + 1]; ++e) {
      const int t = S.level_fronts[e];
      // L21 (U12) items of the front: one per OFF_G OFF_RPL update rows (general mode: and columns)
      P.dec_nitems[l] += (sym ? 1 : 2) * ((S.fronts[t].f - S.fronts[t].ns + OFF_G * OFF_RPL - 1) / (OFF_G * OFF_RPL));
      P.dec_maxns[l] = std::max(P.dec_maxns[l], S.fronts[t].ns);
      P.dec_maxf[l] = std::max(P.dec_maxf[l], S.fronts[t].f);
      if (!P.active[t]) continue;
      P.level_fronts.push_back(t);
      P.level_maxns[l] = std::max(P.level_maxns[l], S.fronts[t].ns);
      P.level_maxf[l] = std::max(P.level_maxf[l], S.fronts[t].f);
    }
    P.level_ptr.push_back((int32_t)P.level_fronts.size());
  }
  std::vector<std::vector<int>> kids(nfr);
  for (int t = 0; t < nfr; ++t)
    if (S.fronts[t].parent >= 0) kids[S.fronts[t].parent].push_back(t);

  // ---- Schur complement: 16 x 16 blocks (symmetric mode, update blocks of >= blk_min rows) or 4 x 4 tiles, level
  // by level, with the children's update-matrix entries landing in each (the extend-add as a gather)
  P.blk_front.assign(nfr, 0);
  P.gxp.assign(1, 0);
  P.bgxp.assign(1, 0);
  P.tile_ptr.assign(1, 0);
  P.blk_ptr.assign(1, 0);
  std::vector<int32_t> first;
  std::vector<std::pair<int32_t, int32_t>> more;
  for (int l = 0; l < L; ++l) {
    for (int e = P.level_ptr[l]; e < P.level_ptr[l + 1]; ++e) {
      const int t = P.level_fronts[e];
      const Front& F = S.fronts[t];
      const int r = F.f - F.ns;
      a22_sources(S, kids, t, sym, first, more);
      if (sym && blk_min > 0 && r >= blk_min) {
        // blocks touching the lower triangle; wave w owns the 4 x 4 tile (w / 4, w % 4)
        constexpr int B = SCHUR_BLK, BC = SCHUR_BLK, tcw = BC / 4;
        for (int i0 = 0; i0 < r; i0 += B)
          for (int j0 = 0; j0 < i0 + B; j0 += BC) {
            P.blocks.push_back({t, i0, j0, 0});
            for (int w = 0; w < BC; ++w)
              for (int pos = 0; pos < 16; ++pos) {
                const int i = i0 + 4 * (w / tcw) + pos / 4, j = j0 + 4 * (w % tcw) + pos % 4;
                if (i >= r || j > i) {
                  P.bg1.push_back(-1);
                  continue;
                }
                P.bg1.push_back(first[(size_t)i * r + j]);
                each_more(more, i * r + j, [&](int32_t id) { P.bgx.push_back({w * 16 + pos, id}); });
              }
            P.bgxp.push_back((int32_t)P.bgx.size());
          }
        P.blk_front[t] = 1;
        continue;
      }
      // super-tiles (symmetric: those touching the lower triangle); lane group `sub` owns the TM x TN tile at
      // (TM (sub / SC), TN (sub % SC)); per super-tile the dense first-source ids, then one overflow range
      constexpr int TM = SCHUR_TM, TN = SCHUR_TN, SR = SCHUR_SR, SC = SCHUR_SC, STR = TM * SR, STC = TN * SC;
      for (int i0 = 0; i0 < r; i0 += STR)
        for (int j0 = 0; j0 < r && (!sym || j0 <= i0 + STR - 1); j0 += STC) {
          P.tiles.push_back({t, i0, j0, 0});
          for (int sub = 0; sub < SR * SC; ++sub)
            for (int pos = 0; pos < TM * TN; ++pos) {
              const int i = i0 + TM * (sub / SC) + pos / TN, j = j0 + TN * (sub % SC) + pos % TN;
              if (i >= r || j >= r || (sym && j > i)) {
                P.g1.push_back(-1);
                continue;
              }
              P.g1.push_back(first[(size_t)i * r + j]);
              each_more(more, i * r + j, [&](int32_t id) { P.gx.push_back({sub * TM * TN + pos, id}); });
            }
          P.gxp.push_back((int32_t)P.gx.size());
        }
    }
    P.tile_ptr.push_back((int32_t)P.tiles.size());
    P.blk_ptr.push_back((int32_t)P.blocks.size());
  }

  // ---- panel-region sources of every front, as a gather: per entry the original matrix entry (or -1) and the
  // first child update-matrix entry landing there (or -1), rare further child entries in overflow lists
  //  * A11: assembly records (dst, nz, src, -) in chunks of 8 (k_assemble_level), levels padded to 8 records;
  //  * L21 rows / U12 columns: gathered by k_offdiag_level itself at their first load (records (nz, src) per
  //    item x row slot x pivot, item.w = offset), so those entries are never stored before their final value
  P.asm_xp.assign(1, 0);
  P.oxp.assign(1, 0);
  P.asm_ptr.assign(1, 0);
  P.item_ptr.assign(1, 0);
  std::vector<int32_t> nzm, s1m;
  std::vector<std::pair<int32_t, int32_t>> morem;   // (a * f + b, id)
  // the panel-region sources of front t: nzm / s1m (f x f, -1 none) and the sorted overflow list morem
  auto panel_sources = [&](int t) {
    const Front& F = S.fronts[t];
    const int f = F.f, ns = F.ns;
    nzm.assign((size_t)f * f, -1);
    s1m.assign((size_t)f * f, -1);
    morem.clear();
    for (int a = 0; a < f; ++a) {
      const int r = F.row0 + a;
      const int width = a < ns ? f : ns;
      for (int x = S.asm_ptr[r]; x < S.asm_ptr[r + 1]; ++x)
        if (S.asm_col[x] < width) nzm[(size_t)a * f + S.asm_col[x]] = S.asm_nz[x];
      for (int x = S.ea_ptr[r]; x < S.ea_ptr[r + 1]; ++x) {
        const int src = S.ea_src[x];
        const Front& C = S.fronts[S.row_front[src]];
        const int32_t* rp = S.relpos.data() + C.row0;
        for (int b = C.ns; b < C.f; ++b) {
          const int pb = rp[b];
          if (pb >= width) continue;
          // symmetric: the child's update matrix holds its lower triangle only
          const int ca = src - C.row0;
          const int32_t id = (int32_t)(C.off + (sym && ca < b ? (int64_t)b * C.f + ca : (int64_t)ca * C.f + b));
          int32_t& s1 = s1m[(size_t)a * f + pb];
          if (s1 < 0)
            s1 = id;
          else
            morem.emplace_back(a * f + pb, id);
        }
      }
    }
    std::sort(morem.begin(), morem.end());
  };
  // the fused bottom level (k_front0) is a decision for the whole analysis: every level-0 front, covered by this plan
  // or not, within F0_NS pivots and F0_RM update rows and without child entries -- a view fuses its bottom level
  // exactly when the full plan does (and lists only its own fronts)
  std::vector<int32_t> rec0;
  auto front0_ok = [&](int t) {   // after panel_sources(t); rec0: the front's records
    const Front& F = S.fronts[t];
    const int f = F.f, ns = F.ns;
    bool ok = ns <= F0_NS && f - ns <= F0_RM && morem.empty();
    rec0.clear();
    for (int a = 0; a < f && ok; ++a)
      for (int b = 0; b < std::min(a + 1, ns); ++b) {
        ok = ok && s1m[(size_t)a * f + b] < 0;   // leaves: no child entries
        rec0.push_back(nzm[(size_t)a * f + b]);
      }
    return ok;
  };
  bool ok0 = sym;
  for (int e = L > 0 ? S.level_ptr[0] : 0; ok0 && e < (L > 0 ? S.level_ptr[1] : 0); ++e) {
    const int t = S.level_fronts[e];
    if (P.active[t]) continue;   // the covered fronts are checked where their records are built
    ok0 = S.fronts[t].ns <= F0_NS && S.fronts[t].f - S.fronts[t].ns <= F0_RM;
    if (!ok0) break;
    panel_sources(t);
    ok0 = front0_ok(t);
  }
  std::vector<std::pair<int32_t, std::vector<int32_t>>> f0;   // level-0 fronts: (front, records)
  for (int l = 0; l < L; ++l) {
    for (int e = P.level_ptr[l]; e < P.level_ptr[l + 1]; ++e) {
      const int t = P.level_fronts[e];
      const Front& F = S.fronts[t];
      const int f = F.f, ns = F.ns;
      panel_sources(t);
      if (l == 0 && ok0) {
        ok0 = front0_ok(t);
        if (ok0) f0.emplace_back(t, rec0);
      }
      for (int a = 0; a < ns; ++a)
        for (int b = 0; b < (sym ? a + 1 : ns); ++b) {   // symmetric: A11's lower triangle only
          const int k = (int)(P.asm_rec.size() % 8);
          P.asm_rec.push_back({(int32_t)(F.off + (int64_t)a * f + b), nzm[(size_t)a * f + b], s1m[(size_t)a * f + b], 0});
          each_more(morem, a * f + b, [&](int32_t id) { P.asm_x.push_back({k, id}); });
          if (P.asm_rec.size() % 8 == 0) P.asm_xp.push_back((int32_t)P.asm_x.size());
        }
      for (int kind = 0; kind < (sym ? 1 : 2); ++kind)   // symmetric: U12 = diag(U11) L21^T implicit
        for (int i0 = ns; i0 < f; i0 += OFF_G * OFF_RPL) {
          P.items.push_back({t, i0, kind, (int32_t)P.orec.size()});
          for (int slot = 0; slot < OFF_G * OFF_RPL; ++slot)   // row i0 + slot = i0 + OFF_G h + lane group
            for (int c = 0; c < ns; ++c) {
              const int idx = i0 + slot;
              if (idx >= f) {
                P.orec.push_back({-1, -1});
                continue;
              }
              const int a = kind == 0 ? idx : c, b = kind == 0 ? c : idx;
              P.orec.push_back({nzm[(size_t)a * f + b], s1m[(size_t)a * f + b]});
              each_more(morem, a * f + b, [&](int32_t id) { P.ox.push_back({c * OFF_G * OFF_RPL + slot, id}); });
            }
          P.oxp.push_back((int32_t)P.ox.size());
        }
    }
    while (P.asm_rec.size() % 8) {        // pad: no-op records (dst = -1)
      P.asm_rec.push_back({-1, -1, -1, 0});
      if (P.asm_rec.size() % 8 == 0) P.asm_xp.push_back((int32_t)P.asm_x.size());
    }
    P.asm_ptr.push_back((int32_t)P.asm_rec.size());
    P.item_ptr.push_back((int32_t)P.items.size());
  }

  // ---- the fused bottom level
  P.fused0 = ok0 && !f0.empty() && L > 0;
  if (P.fused0) {
    std::stable_partition(f0.begin(), f0.end(), [&](const auto& x) { return S.fronts[x.first].ns <= 2; });
    P.f0_ptr.assign(1, 0);
    for (const auto& x : f0) {
      P.f0_front.push_back(x.first);
      P.f0_nz.insert(P.f0_nz.end(), x.second.begin(), x.second.end());
      P.f0_ptr.push_back((int32_t)P.f0_nz.size());
      P.f0_small += S.fronts[x.first].ns <= 2;
    }
  }

  // ---- algorithmic bytes per frequency and level of classes 0-4 (16 B per complex entry loaded or stored)
  P.lev_bytes.assign(L, std::array<int64_t, NKC>{});
  for (int t = 0; t < nfr; ++t) {
    if (!P.active[t]) continue;
    const Front& F = S.fronts[t];
    const int64_t r = F.f - F.ns, ns = F.ns;
    const int64_t a11 = sym ? ns * (ns + 1) / 2 : ns * ns;
    auto& b = P.lev_bytes[F.level];
    b[0] += 16 * a11;                                                // A11 (symmetric: lower) stores
    b[1] += 16 * (a11 + ns * ns);                                    // A11 read + L11 / U11 write
    b[2] += 16 * ((sym ? 1 : 2) * r * ns + ns * ns);                 // L21 / U12 stores + L11 / U11 read
    b[3 + (P.blk_front[t] ? 0 : 1)] += 16 * ((sym ? r * (r + 1) / 2 : r * r) + (sym ? 1 : 2) * r * ns);   // A22 + L21
  }
  for (int l = 0; l < L; ++l) {                                      // + the children's entries each class gathers
    auto& b = P.lev_bytes[l];
    int64_t g = 0;
    for (int r = P.asm_ptr[l]; r < P.asm_ptr[l + 1]; ++r) g += P.asm_rec[r].z >= 0;
    b[0] += 16 * (g + P.asm_xp[P.asm_ptr[l + 1] / 8] - P.asm_xp[P.asm_ptr[l] / 8]);
    g = 0;
    const int64_t o0 = P.item_ptr[l] < (int)P.items.size() ? P.items[P.item_ptr[l]].w : (int64_t)P.orec.size();
    const int64_t o1 = P.item_ptr[l + 1] < (int)P.items.size() ? P.items[P.item_ptr[l + 1]].w : (int64_t)P.orec.size();
    for (int64_t x = o0; x < o1; ++x) g += P.orec[x].y >= 0;
    b[2] += 16 * (g + P.oxp[P.item_ptr[l + 1]] - P.oxp[P.item_ptr[l]]);
    g = 0;
    for (size_t x = (size_t)P.blk_ptr[l] * SCHUR_BLK_IDS; x < (size_t)P.blk_ptr[l + 1] * SCHUR_BLK_IDS; ++x) g += P.bg1[x] >= 0;
    b[3] += 16 * (g + P.bgxp[P.blk_ptr[l + 1]] - P.bgxp[P.blk_ptr[l]]);
    g = 0;
    for (size_t x = (size_t)P.tile_ptr[l] * SCHUR_TILE; x < (size_t)P.tile_ptr[l + 1] * SCHUR_TILE; ++x) g += P.g1[x] >= 0;
    b[4] += 16 * (g + P.gxp[P.tile_ptr[l + 1]] - P.gxp[P.tile_ptr[l]]);
  }
  if (P.fused0) {   // level 0 in one pass (class 0): A11 block, L21 rows and update block stored once, nothing read back
    auto& b = P.lev_bytes[0];
    b = {};
    for (const int32_t t : P.f0_front) {
      const int64_t ns = S.fronts[t].ns, r = S.fronts[t].f - ns;
      b[0] += 16 * (ns * ns + r * ns + r * (r + 1) / 2);
    }
  }

  // ---- symmetric mode: Dirichlet decoupling lists -- coupled rows (with their entries), per Dirichlet node the
  // entries of its column (adjoint correction), the coupled-row slot of every permuted row
  P.cslot.assign(S.n, -1);
  P.cptr_dir.assign(1, 0);
  P.dptr.assign(1, 0);
  if (sym && !S.dir_p.empty()) {
    for (size_t d = 0; d < S.dir_p.size(); ++d) P.dir.push_back({S.dir_p[d], S.dir_nz[d]});
    for (size_t c = 0; c < S.cpl_p.size(); ++c) {
      if (P.crow.empty() || P.crow.back() != S.cpl_p[c]) {
        if (!P.crow.empty()) P.cptr_dir.push_back((int32_t)P.ce.size());
        P.cslot[S.cpl_p[c]] = (int32_t)P.crow.size();
        P.crow.push_back(S.cpl_p[c]);
      }
      P.ce.push_back({S.cpl_dir[c], S.cpl_nz[c]});
    }
    P.cptr_dir.push_back((int32_t)P.ce.size());
    for (size_t d = 0; d < S.dir_p.size(); ++d) {
      for (size_t c = 0; c < S.cpl_p.size(); ++c)
        if (S.cpl_dir[c] == (int32_t)d) P.de.push_back({S.cpl_p[c], S.cpl_nz[c]});
      P.dptr.push_back((int32_t)P.de.size());
    }
    P.n_dir = (int)S.dir_p.size();
    P.n_crow = (int)(P.cptr_dir.size() - 1);
  }

  // ---- permuted matrix compressed by rows and by columns (residual walks, Hessian tangent operators)
  auto compress = [&](const std::vector<int32_t>& key, const std::vector<int32_t>& other, std::vector<int32_t>& ptr,
                      std::vector<int32_t>& idx, std::vector<int32_t>& nz) {
    ptr.assign(S.n + 1, 0);
    idx.assign(S.nnz, 0);
    nz.assign(S.nnz, 0);
    for (int64_t e = 0; e < S.nnz; ++e) ++ptr[key[e] + 1];
    for (int i = 0; i < S.n; ++i) ptr[i + 1] += ptr[i];
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    for (int64_t e = 0; e < S.nnz; ++e) {
      const int32_t at = fill[key[e]]++;
      idx[at] = other[e];
      nz[at] = (int32_t)e;
    }
  };
  compress(S.prow, S.pcol, P.rptr, P.ridx, P.rnz);
  compress(S.pcol, S.prow, P.cptr, P.cidx, P.cnz);

  // ---- union row structure of the gradient contraction (k_contract_eg): rows in original order (mesh-local:
  // neighbouring walks gather the same solution rows whatever the ordering), entries of a row by permuted column
  {
    std::vector<int64_t> key(S.nnz);
    std::vector<int32_t> ord(S.nnz);
    for (int64_t e = 0; e < S.nnz; ++e) {
      key[e] = (int64_t)S.prow[e] * S.n + S.pcol[e];
      ord[e] = (int32_t)e;
    }
    std::sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
    auto find = [&](int64_t k) -> int32_t {
      auto it = std::lower_bound(ord.begin(), ord.end(), k, [&](int32_t a, int64_t v) { return key[a] < v; });
      return (it != ord.end() && key[*it] == k) ? *it : -1;
    };
    std::vector<std::vector<I4>> rows(S.n);
    for (int32_t e : ord) {   // row-major, columns ascending
      const int32_t i = S.prow[e], j = S.pcol[e];
      rows[i].push_back({j, e, find((int64_t)j * S.n + i), 0});
    }
    for (int32_t e : ord) {   // (i, j) whose mirror (j, i) is not in the pattern: column-only entry of row j
      const int32_t i = S.prow[e], j = S.pcol[e];
      if (find((int64_t)j * S.n + i) < 0) rows[j].push_back({i, -1, e, 0});
    }
    for (int t = 0; t < S.n; ++t) {
      const int i = S.iperm[t];
      std::sort(rows[i].begin(), rows[i].end(), [](const I4& a, const I4& b) { return a.x < b.x; });
      P.uent.push_back({-1, -1, -1, i});
      for (const I4& v : rows[i]) P.uent.push_back({v.x, v.y, v.z, i});
    }
    P.n_uent = (int)P.uent.size();
    for (int pad = 0; pad < 4; ++pad) P.uent.push_back({-1, -1, -1, -1});   // a step reads 4 entries at once
  }
  return 0;
}

std::vector<char> loaded_fronts(const Symbolic& S, const double* rhs_perm) {
  const int nfr = (int)S.fronts.size();
  std::vector<int32_t> front_of_col(S.n, -1), root(nfr);
  for (int t = 0; t < nfr; ++t)
    for (int a = 0; a < S.fronts[t].ns; ++a) front_of_col[S.fronts[t].col0 + a] = t;
  for (int t = 0; t < nfr; ++t) {
    int r = t;
    while (S.fronts[r].parent >= 0) r = S.fronts[r].parent;
    root[t] = r;
  }
  std::vector<char> loaded_root(nfr, 0);
  auto load = [&](int32_t p) {
    if (p >= 0 && p < S.n && front_of_col[p] >= 0) loaded_root[root[front_of_col[p]]] = 1;
  };
  for (int32_t p = 0; p < S.n; ++p)
    if (rhs_perm[p] != 0.0) load(p);
  for (size_t c = 0; c < S.cpl_p.size(); ++c)
    if (rhs_perm[S.dir_p[S.cpl_dir[c]]] != 0.0) load(S.cpl_p[c]);
  // a Dirichlet node whose column reaches a loaded tree stays with it (the node's own value is zero: its forward
  // solution is zero too, but its 1 x 1 front is not worth a second kind of tree -- the loaded set is then the union
  // of the pattern's connected components that hold a loaded row)
  const std::vector<char> by_value(loaded_root);
  for (size_t c = 0; c < S.cpl_p.size(); ++c)
    if (by_value[root[front_of_col[S.cpl_p[c]]]]) load(S.dir_p[S.cpl_dir[c]]);
  std::vector<char> mask(nfr);
  for (int t = 0; t < nfr; ++t) mask[t] = loaded_root[root[t]];
  return mask;
}

std::vector<uint32_t> stiffness_bits(const double* stiff, int64_t nnz, int n_stiff) {
  std::vector<uint32_t> bits(nnz, 0);
  for (int64_t nz = 0; nz < nnz; ++nz)
    for (int k = 0; k < n_stiff; ++k)
      if (stiff[nz * n_stiff + k] != 0.0) bits[nz] |= 1u << k;
  return bits;
}

uint32_t live_stiffness(const Symbolic& S, const std::vector<char>* mask, const std::vector<uint32_t>& bits) {
  std::vector<char> row_on(S.n, mask ? 0 : 1);
  if (mask)
    for (size_t t = 0; t < S.fronts.size(); ++t)
      if ((*mask)[t])
        for (int a = 0; a < S.fronts[t].ns; ++a) row_on[S.fronts[t].col0 + a] = 1;
  uint32_t live = 0;
  for (int64_t nz = 0; nz < S.nnz && nz < (int64_t)bits.size(); ++nz)
    if (row_on[S.prow[nz]]) live |= bits[nz];
  return live;
}

std::vector<char> mass_on(const double* mass, int64_t nnz, int n_mass) {
  std::vector<char> on(nnz, 0);
  for (int64_t nz = 0; nz < nnz; ++nz)
    for (int j = 0; j < n_mass; ++j)
      if (mass[nz * n_mass + j] != 0.0) on[nz] = 1;
  return on;
}

std::vector<char> front_rows(const Symbolic& S, const std::vector<char>& mask) {
  std::vector<char> row_on(S.n, 0);
  for (size_t t = 0; t < S.fronts.size() && t < mask.size(); ++t)
    if (mask[t])
      for (int a = 0; a < S.fronts[t].ns; ++a) row_on[S.fronts[t].col0 + a] = 1;
  return row_on;
}

MassList mass_entries(const std::vector<I4>& uent, int n_uent, int n, const std::vector<char>* row_on,
                      const std::vector<char>& on) {
  MassList L;
  n_uent = std::min<int64_t>(n_uent, (int64_t)uent.size());
  const int waves = 4 * contract_mass_parts(n, n_uent), seg = mass_segment(n, n_uent);
  L.ptr.assign(1, 0);
  for (int w = 0; w < waves; ++w) {
    for (int64_t e = (int64_t)w * seg; e < std::min<int64_t>((int64_t)(w + 1) * seg, n_uent); ++e) {
      const I4& u = uent[e];
      if (u.x < 0 || u.y < 0 || u.y >= (int64_t)on.size() || u.w < 0) continue;
      if (row_on && (u.w >= (int64_t)row_on->size() || !(*row_on)[u.w])) continue;
      if (!on[u.y]) continue;
      L.list.push_back((int32_t)e);
      ++L.n_list;
    }
    while (L.list.size() % MASS_U) L.list.push_back(-1);
    L.ptr.push_back((int32_t)(L.list.size() / MASS_U));
  }
  return L;
}

std::vector<int32_t> rows_in(const Symbolic& S, const std::vector<char>& mask, const std::vector<int32_t>& prows) {
  std::vector<char> row_on(S.n, 0);
  for (size_t t = 0; t < S.fronts.size(); ++t)
    if (mask[t])
      for (int a = 0; a < S.fronts[t].ns; ++a) row_on[S.fronts[t].col0 + a] = 1;
  std::vector<int32_t> out;
  for (int32_t p : prows)
    if (p >= 0 && p < S.n && row_on[p]) out.push_back(p);
  return out;
}

void reach_lists(const std::vector<int32_t>& front_of_col, const std::vector<int32_t>& front_parent,
                 const std::vector<int32_t>& level_ptr, const std::vector<int32_t>& level_fronts,
                 const std::vector<int32_t>& prows, std::vector<int32_t>& mark, std::vector<int32_t>& list,
                 std::vector<int32_t>& ptr) {
  mark.assign(front_parent.size(), 0);
  for (int32_t p : prows)
    for (int t = front_of_col[p]; t >= 0 && !mark[t]; t = front_parent[t]) mark[t] = 1;
  const int L = (int)level_ptr.size() - 1;
  list.clear();
  ptr.assign(1, 0);
  for (int l = 0; l < L; ++l) {
    for (int e = level_ptr[l]; e < level_ptr[l + 1]; ++e)
      if (mark[level_fronts[e]]) list.push_back(level_fronts[e]);
    ptr.push_back((int32_t)list.size());
  }
}

std::string field_rows(const std::vector<int32_t>& iperm, int32_t n_rows, const int32_t* rows, std::vector<int32_t>& out) {
  out.clear();
  if (!rows || n_rows <= 0) return "field sweep: a row list needs at least one row";
  const int64_t n = (int64_t)iperm.size();
  out.reserve((size_t)n_rows);
  for (int32_t j = 0; j < n_rows; ++j) {
    if (rows[j] < 0 || rows[j] >= n) {
      char buf[128];
      snprintf(buf, sizeof buf, "field sweep: row %d = %d outside [0, %lld)", (int)j, (int)rows[j], (long long)n);
      return buf;
    }
    out.push_back(iperm[rows[j]]);
  }
  return "";
}

std::string field_loss_rows(const std::vector<int32_t>& iperm, int32_t n_rows, const int32_t* rows,
                            const double* weights, bool cotangent, std::vector<int32_t>& out) {
  out.clear();
  char buf[160];
  const int64_t n = (int64_t)iperm.size();
  if (!rows && n <= 0) return "field loss sweep: no rows";
  if (rows && n_rows <= 0) return "field loss sweep: a row list needs at least one row";
  if (weights && cotangent)
    return "field loss sweep: weights do not apply to PFR_LOSS_FCOTANGENT (the cotangent carries them)";
  if (weights) {
    const int64_t n_sel = rows ? n_rows : n;
    bool any = false;
    for (int64_t j = 0; j < n_sel; ++j) {
      const double v = weights[j];
      if (!(v >= 0.0) || v > 1.7976931348623157e308) {   // negative, NaN or infinite
        snprintf(buf, sizeof buf, "field loss sweep: weight %lld = %g is negative or not finite", (long long)j, v);
        return buf;
      }
      any = any || v > 0.0;
    }
    if (!any) return "field loss sweep: every weight is zero";
  }
  if (!rows) return "";
  std::string refusal = field_rows(iperm, n_rows, rows, out);
  std::vector<char> seen((size_t)n, 0);
  for (int32_t j = 0; refusal.empty() && j < n_rows; ++j) {
    if (seen[rows[j]]) {
      snprintf(buf, sizeof buf, "field loss sweep: row %d = %d repeats an earlier one", (int)j, (int)rows[j]);
      refusal = buf;
    }
    seen[rows[j]] = 1;
  }
  if (!refusal.empty()) out.clear();
  return refusal;
}

std::string check_plan(const Symbolic& S, const Plan& P, int64_t Fc) {
  char buf[256];
  auto bad = [&](const char* what, int64_t at, int64_t v, int64_t lim) {
    snprintf(buf, sizeof buf, "%s: entry %lld = %lld outside [0, %lld)", what, (long long)at, (long long)v, (long long)lim);
    return std::string(buf);
  };
  const int64_t FE = S.factor_entries, NNZ = S.nnz;
  const int nfr = (int)S.fronts.size(), L = P.L;
  auto id_ok = [&](int64_t v) { return v >= -1 && v < FE; };   // element id or -1
  auto nz_ok = [&](int64_t v) { return v >= -1 && v < NNZ; };
  if (Fc <= 0 || Fc % 64) return "chunk not a multiple of 64";
  // fronts: storage, work vectors, pivot columns, index staging
  for (int t = 0; t < nfr; ++t) {
    const Front& F = S.fronts[t];
    if (F.off < 0 || F.off + (int64_t)F.f * F.f > FE) return bad("front storage", t, F.off, FE);
    if (F.row0 < 0 || F.row0 + (int64_t)F.f > S.total_rows) return bad("front rows", t, F.row0, S.total_rows);
    if (F.col0 < 0 || F.col0 + F.ns > S.n) return bad("front pivots", t, F.col0, S.n);
    if (F.f > MAX_FRONT || F.ns < 1 || F.ns > F.f) return bad("front size", t, F.f, MAX_FRONT + 1);
    if (F.parent >= nfr || F.level < 0 || F.level >= L) return bad("front parent / level", t, F.parent, nfr);
  }
  for (int64_t r = 0; r < S.total_rows; ++r)
    if (S.idx[r] < 0 || S.idx[r] >= S.n) return bad("front row index", r, S.idx[r], S.n);
  // the covered fronts: whole trees, each listed once in its level; every record's front among them
  if ((int)P.active.size() != nfr || (int)P.level_ptr.size() != L + 1 || (int)P.level_maxf.size() != L ||
      (int)P.level_maxns.size() != L || P.level_ptr[0] != 0 || P.level_ptr[L] != (int)P.level_fronts.size())
    return "covered fronts";
  {
    int64_t n_act = 0;
    for (int t = 0; t < nfr; ++t) {
      n_act += P.active[t] != 0;
      if (S.fronts[t].parent >= 0 && P.active[t] != P.active[S.fronts[t].parent]) return bad("view splits a tree", t, P.active[t], 2);
    }
    if (n_act != (int64_t)P.level_fronts.size()) return bad("covered front lists", 0, (int64_t)P.level_fronts.size(), n_act + 1);
    for (int l = 0; l < L; ++l)
      for (int e = P.level_ptr[l]; e < P.level_ptr[l + 1]; ++e) {
        const int t = P.level_fronts[e];
        if (t < 0 || t >= nfr || !P.active[t] || S.fronts[t].level != l) return bad("covered front", e, t, nfr);
        if (S.fronts[t].ns > P.level_maxns[l] || S.fronts[t].f > P.level_maxf[l]) return bad("level geometry", l, S.fronts[t].f, P.level_maxf[l] + 1);
      }
  }
  // A11 assembly: records in chunks of 8 per launch (grid covers asm_ptr[l + 1] - asm_ptr[l] records)
  if (P.asm_rec.size() % 8 || P.asm_xp.size() != P.asm_rec.size() / 8 + 1) return "assembly chunks";
  for (size_t x = 0; x < P.asm_rec.size(); ++x) {
    const I4& a = P.asm_rec[x];
    if (!id_ok(a.x) || !nz_ok(a.y) || !id_ok(a.z)) return bad("assembly record", x, a.x, FE);
  }
  for (size_t c = 0; c + 1 < P.asm_xp.size(); ++c)
    if (P.asm_xp[c] > P.asm_xp[c + 1] || P.asm_xp[c + 1] > (int64_t)P.asm_x.size()) return bad("assembly overflow", c, P.asm_xp[c], P.asm_x.size());
  for (size_t x = 0; x < P.asm_x.size(); ++x)
    if (P.asm_x[x].x < 0 || P.asm_x[x].x >= 8 || P.asm_x[x].y < 0 || P.asm_x[x].y >= FE) return bad("assembly extra", x, P.asm_x[x].y, FE);
  for (int l = 0; l <= L; ++l)
    if (P.asm_ptr[l] % 8) return bad("assembly level padding", l, P.asm_ptr[l], 8);
  // L21 items: each item's OFF_G OFF_RPL rows x ns records inside orec, rows inside the front
  if (P.oxp.size() != P.items.size() + 1) return "item overflow ranges";
  for (size_t i = 0; i < P.items.size(); ++i) {
    const I4& it = P.items[i];
    if (it.x < 0 || it.x >= nfr || !P.active[it.x]) return bad("item front", i, it.x, nfr);
    const Front& F = S.fronts[it.x];
    if (it.y < F.ns || it.y >= F.f) return bad("item row", i, it.y, F.f);
    if (it.w < 0 || it.w + (int64_t)OFF_G * OFF_RPL * F.ns > (int64_t)P.orec.size()) return bad("item records", i, it.w, P.orec.size());
    if (P.oxp[i] > P.oxp[i + 1] || P.oxp[i + 1] > (int64_t)P.ox.size()) return bad("item overflow", i, P.oxp[i], P.ox.size());
    for (int x = P.oxp[i]; x < P.oxp[i + 1]; ++x)
      if (P.ox[x].x < 0 || P.ox[x].x >= OFF_G * OFF_RPL * F.ns || P.ox[x].y < 0 || P.ox[x].y >= FE)
        return bad("item extra", x, P.ox[x].y, FE);
  }
  for (size_t x = 0; x < P.orec.size(); ++x)
    if (!nz_ok(P.orec[x].x) || !id_ok(P.orec[x].y)) return bad("item record", x, P.orec[x].y, FE);
  // Schur tiles / blocks: origins inside the update block, first-source ids and overflow ranges
  if (P.g1.size() != P.tiles.size() * SCHUR_TILE || P.gxp.size() != P.tiles.size() + 1) return "tile sources";
  if (P.bg1.size() != P.blocks.size() * SCHUR_BLK_IDS || P.bgxp.size() != P.blocks.size() + 1) return "block sources";
  for (size_t i = 0; i < P.tiles.size(); ++i) {
    const I4& tt = P.tiles[i];
    if (tt.x < 0 || tt.x >= nfr || !P.active[tt.x]) return bad("tile front", i, tt.x, nfr);
    const int r = S.fronts[tt.x].f - S.fronts[tt.x].ns;
    if (tt.y < 0 || tt.y >= r || tt.z < 0 || tt.z >= r) return bad("tile origin", i, tt.y, r);
    if (P.gxp[i] > P.gxp[i + 1] || P.gxp[i + 1] > (int64_t)P.gx.size()) return bad("tile overflow", i, P.gxp[i], P.gx.size());
  }
  for (size_t i = 0; i < P.blocks.size(); ++i) {
    const I4& bk = P.blocks[i];
    if (bk.x < 0 || bk.x >= nfr || !P.active[bk.x]) return bad("block front", i, bk.x, nfr);
    const int r = S.fronts[bk.x].f - S.fronts[bk.x].ns;
    if (bk.y < 0 || bk.y >= r || bk.z < 0 || bk.z > bk.y + SCHUR_BLK) return bad("block origin", i, bk.y, r);
    if (P.bgxp[i] > P.bgxp[i + 1] || P.bgxp[i + 1] > (int64_t)P.bgx.size()) return bad("block overflow", i, P.bgxp[i], P.bgx.size());
  }
  for (size_t x = 0; x < P.g1.size(); ++x)
    if (!id_ok(P.g1[x])) return bad("tile source", x, P.g1[x], FE);
  for (size_t x = 0; x < P.bg1.size(); ++x)
    if (!id_ok(P.bg1[x])) return bad("block source", x, P.bg1[x], FE);
  for (size_t x = 0; x < P.gx.size(); ++x)
    if (P.gx[x].x < 0 || P.gx[x].x >= SCHUR_TILE || P.gx[x].y < 0 || P.gx[x].y >= FE) return bad("tile extra", x, P.gx[x].y, FE);
  for (size_t x = 0; x < P.bgx.size(); ++x)
    if (P.bgx[x].x < 0 || P.bgx[x].x >= SCHUR_BLK_IDS || P.bgx[x].y < 0 || P.bgx[x].y >= FE) return bad("block extra", x, P.bgx[x].y, FE);
  // the fused bottom level: every level-0 front listed once, <= 2-pivot fronts first, records of its panel
  if (P.fused0) {
    const int n0 = (int)P.f0_front.size();
    if ((int)P.f0_ptr.size() != n0 + 1 || P.f0_ptr[0] != 0 || P.f0_ptr[n0] != (int)P.f0_nz.size() ||
        n0 != P.level_ptr[1] - P.level_ptr[0] || P.f0_small < 0 || P.f0_small > n0)
      return "fused level 0 lists";
    // decided for the whole analysis: every level-0 front fits, whether this plan covers it or not
    for (int e = S.level_ptr[0]; e < S.level_ptr[1]; ++e) {
      const Front& F = S.fronts[S.level_fronts[e]];
      if (F.ns > F0_NS || F.f - F.ns > F0_RM) return bad("fused level 0 decided for the view alone", S.level_fronts[e], F.ns, F0_NS + 1);
    }
    for (int i = 0; i < n0; ++i) {
      const int t = P.f0_front[i];
      if (t < 0 || t >= (int)S.fronts.size() || !P.active[t]) return bad("fused level 0 front", i, t, (int64_t)S.fronts.size());
      const Front& F = S.fronts[t];
      const int r = F.f - F.ns;
      if (F.level != 0 || F.ns > F0_NS || r > F0_RM || (F.ns <= 2) != (i < P.f0_small) ||
          P.f0_ptr[i + 1] - P.f0_ptr[i] != F.ns * (F.ns + 1) / 2 + r * F.ns)
        return bad("fused level 0 front", i, F.ns, r);
    }
    for (size_t x = 0; x < P.f0_nz.size(); ++x)
      if (P.f0_nz[x] < -1 || P.f0_nz[x] >= S.nnz) return bad("fused level 0 nz", x, P.f0_nz[x], S.nnz);
  } else if (P.sym && L > 0 && P.level_ptr[1] > P.level_ptr[0]) {
    // ... and the other way round: a plan with level-0 fronts leaves them unfused only if some level-0 front of the
    // analysis does not fit (one without children has no child entries)
    bool fits = true;
    std::vector<char> has_child(nfr, 0);
    for (int t = 0; t < nfr; ++t)
      if (S.fronts[t].parent >= 0) has_child[S.fronts[t].parent] = 1;
    for (int e = S.level_ptr[0]; e < S.level_ptr[1] && fits; ++e) {
      const Front& F = S.fronts[S.level_fronts[e]];
      fits = F.ns <= F0_NS && F.f - F.ns <= F0_RM && !has_child[S.level_fronts[e]];
    }
    if (fits) return "level 0 not fused where the whole analysis' fronts fit";
  }
  // per-level ranges monotone and complete
  if ((int)P.tile_ptr.size() != L + 1 || (int)P.blk_ptr.size() != L + 1 || (int)P.item_ptr.size() != L + 1 ||
      (int)P.asm_ptr.size() != L + 1)
    return "level ranges";
  for (int l = 0; l < L; ++l)
    if (P.tile_ptr[l] > P.tile_ptr[l + 1] || P.blk_ptr[l] > P.blk_ptr[l + 1] || P.item_ptr[l] > P.item_ptr[l + 1] ||
        P.asm_ptr[l] > P.asm_ptr[l + 1])
      return bad("level range order", l, P.tile_ptr[l], P.tile_ptr[l + 1]);
  // the whole analysis' item count per level (the L21 prefix is decided for it): the view's items are among them
  if ((int)P.dec_nitems.size() != L || (int)P.dec_nf.size() != L) return "level item counts";
  for (int l = 0; l < L; ++l) {
    const int ni = P.item_ptr[l + 1] - P.item_ptr[l], full = P.level_ptr[l + 1] - P.level_ptr[l] == P.dec_nf[l];
    if (ni > P.dec_nitems[l] || (full && ni != P.dec_nitems[l])) return bad("level item count", l, ni, P.dec_nitems[l] + 1);
  }
  // Dirichlet lists
  const Workspace W = workspace(S, Fc, P.n_crow);
  for (size_t d = 0; d < P.dir.size(); ++d)
    if (P.dir[d].x < 0 || P.dir[d].x >= S.n || !nz_ok(P.dir[d].y)) return bad("Dirichlet node", d, P.dir[d].x, S.n);
  for (size_t c = 0; c < P.crow.size(); ++c)
    if (P.crow[c] < 0 || P.crow[c] >= S.n) return bad("coupled row", c, P.crow[c], S.n);
  for (size_t x = 0; x < P.ce.size(); ++x)
    if (P.ce[x].x < 0 || P.ce[x].x >= P.n_dir || !nz_ok(P.ce[x].y)) return bad("coupling entry", x, P.ce[x].x, P.n_dir);
  for (size_t x = 0; x < P.de.size(); ++x)
    if (P.de[x].x < 0 || P.de[x].x >= S.n || !nz_ok(P.de[x].y)) return bad("Dirichlet column entry", x, P.de[x].x, S.n);
  for (int p = 0; p < S.n; ++p)   // k_dirichlet_rhs writes Bc[cslot * Fc + q]
    if (P.cslot[p] >= P.n_crow || (int64_t)(P.cslot[p] + 1) * Fc > W.Bc) return bad("coupled-row slot", p, P.cslot[p], P.n_crow);
  // compressed rows / columns
  for (int64_t e = 0; e < S.nnz; ++e)
    if (P.ridx[e] < 0 || P.ridx[e] >= S.n || P.cidx[e] < 0 || P.cidx[e] >= S.n || P.rnz[e] >= NNZ || P.cnz[e] >= NNZ)
      return bad("compressed index", e, P.ridx[e], S.n);
  // contraction entries: rows / columns inside n, nz inside nnz, 4 padding entries for the 4-entry steps
  if ((int64_t)P.uent.size() != P.n_uent + 4) return "contraction padding";
  for (int e = 0; e < P.n_uent; ++e) {
    const I4& u = P.uent[e];
    if (u.w < 0 || u.w >= S.n || u.x < -1 || u.x >= S.n || !nz_ok(u.y) || !nz_ok(u.z)) return bad("contraction entry", e, u.x, S.n);
  }
  // per-workgroup partial buffers against the grids that write them
  if ((int64_t)residual_parts(S.n) * Fc > W.cpart) return "k_residual partials";                  // cpart[bx Fc + q]
  if ((int64_t)residual_parts(S.n) * 18 * Fc > W.kpart) return "k_residual contraction partials"; // kpart[(bx 18 + k) Fc + q]
  if ((int64_t)contract_q_parts(S.n, P.n_uent) * 18 * Fc > W.kpart) return "k_contract_q contraction partials";
  // mpart[(bx MASS_NM + j) Fc + q] reuses kpart once k_jac_finish has read it; every entry has its wave
  if ((int64_t)4 * contract_mass_parts(S.n, P.n_uent) * mass_segment(S.n, P.n_uent) < P.n_uent) return "k_contract_mass segments";
  if ((int64_t)contract_mass_parts(S.n, P.n_uent) * MASS_NM * Fc > W.kpart) return "k_contract_mass inertia partials";
  {
    const int64_t partial = (int64_t)std::max<int64_t>(contract_eg_parts(P.n_uent), Fc / 64) * 18;   // api.cpp's size
    if ((int64_t)contract_eg_parts(P.n_uent) * 18 > partial || (Fc / 64) * 18 > partial) return "gradient partials";
  }
  return "";
}

// ---- the launch schedule
Knobs knobs_from_env(int64_t Fc) {
  auto knob = [](const char* name, int def, int lo, int hi) {
    const char* e = getenv(name);
    return e ? std::max(lo, std::min(hi, atoi(e))) : def;
  };
  Knobs k;
  k.solve_wmax = knob("PFR_SOLVE_WMAX", k.solve_wmax, 1, 8);
  k.fac_wmax = knob("PFR_FAC_WMAX", k.fac_wmax, 1, 16);
  k.fac_g_wg = knob("PFR_FAC_G_WG", k.fac_g_wg, 0, 1 << 20);
  k.fac_gbig = knob("PFR_FAC_GBIG", k.fac_gbig, 2, 8);
  if (k.fac_gbig != 2 && k.fac_gbig != 8) k.fac_gbig = 4;
  k.fac_g_ns = knob("PFR_FAC_G_NS", k.fac_g_ns, 0, 1 << 20);
  k.us2_small = knob("PFR_US2_SMALL", k.us2_small, 0, MAX_FRONT);
  k.split_target = knob("PFR_SOLVE_SPLIT", k.split_target, 0, 1 << 20);
  k.us2_nar = knob("PFR_US2_NAR", k.us2_nar, 0, 1 << 30);
  k.fac_lds = knob("PFR_FAC_LDS", k.fac_lds, -1, 64);
  k.us2_tiny = knob("PFR_US2_TINY", k.us2_tiny, 0, 8);
  k.us2_rl = knob("PFR_US2_RL", k.us2_rl, 0, 1);
  k.ls_rl = knob("PFR_LS_RL", Fc <= 1024 ? 1 : 0, 0, 1);
  k.off_pu_waves = knob("PFR_OFF_PU_WAVES", Fc <= 1024 ? 8000 : 0, 0, 1 << 30);
  k.front0 = knob("PFR_FRONT0", k.front0, 0, 1);
  k.blk_min = knob("PFR_SCHUR_BLK_MIN", k.blk_min, 0, MAX_FRONT);
  return k;
}

namespace {

int ceil_div(int a, int b) { return (a + b - 1) / b; }

// nf: the fronts the launch shape is decided for (the full plan's count); count: the fronts the launch covers
SolveLevel solve_level(const Schedule& sc, int l, int nf, int count) {
  SolveLevel r{};
  r.nf = count;
  r.level_w = waves_for(sc.level_maxf[l]);
  // raised (up to solve_wmax) when the launch has too few workgroups to fill the chip -- the sparse passes and the
  // top levels, which are latency-bound: every wave more takes rows off each wave's chain
  r.waves = solve_waves(r.level_w, nf, sc.Fc, sc.knobs.solve_wmax);
  // the update parts split over several workgroups: L solves, and U solves in symmetric mode
  r.split_L = solve_split(nf, sc.Fc, sc.knobs.split_target);
  r.split_U = sc.sym ? r.split_L : 1;
  return r;
}

}  // namespace

void schedule_reach(Schedule& sc, const std::vector<int32_t> (&reach_ptr)[2], const std::vector<int32_t> (*decide)[2]) {
  const Knobs& k = sc.knobs;
  const int L = (int)sc.level_nf.size();
  const int64_t ng = sc.Fc / 64;
  auto count_of = [&](const std::vector<int32_t>& r, int l) { return r.empty() ? 0 : r[l + 1] - r[l]; };
  auto count = [&](int w, int l) { return count_of(reach_ptr[w], l); };
  auto dec = [&](int w, int l) { return count_of(decide ? (*decide)[w] : reach_ptr[w], l); };
  sc.chain.assign(L, ChainLevel{});
  for (int w = 0; w < 2; ++w) sc.solve[SUBSET_REACH0 + w].resize(L);
  for (int l = 0; l < L; ++l) {
    for (int w = 0; w < 2; ++w) sc.solve[SUBSET_REACH0 + w][l] = solve_level(sc, l, dec(w, l), count(w, l));
    ChainLevel& c = sc.chain[l];
    const int maxns = sc.level_maxns[l];
    c.nf0 = count(0, l);
    c.nf1 = count(1, l);
    c.nmax = std::max(c.nf0, c.nf1);
    if (c.nmax == 0) continue;
    c.nsum = c.nf0 + 3 * c.nf1;
    const int dsum = dec(0, l) + 3 * dec(1, l), dmax = std::max(dec(0, l), dec(1, l));   // what the shape is decided for
    c.split = solve_split(dsum, sc.Fc, k.split_target);
    c.waves = solve_waves(waves_for(sc.level_maxf[l]), dmax, sc.Fc, k.solve_wmax);
    // the narrow forms need the update rows apart (split > 1) and the largest pivot block in LDS
    const bool nar = c.split > 1 && dsum * ng < k.us2_nar && ls_nar_fits(maxns);
    c.rows = nar ? ROWS_ZC : c.split > 1 ? ROWS_Z : ROWS_NONE;
    if (nar) c.RB = ceil_div(std::max(1, sc.level_maxf[l] - 1), LRC_SR);
    if (nar && k.ls_rl && maxns <= 16 * RL_WMAX) {   // k_lsolve_rl_z: at most 4 rows per lane slot
      c.form = CHAIN_RL;
      c.rpl = rl_rpl(maxns);
      c.waves = rl_waves(maxns);
    } else if (nar) {
      c.form = CHAIN_NAR;
      c.lds_bytes = maxns * 64 * 16;
    }
  }
}

Schedule level_schedule(const Symbolic& S, const Plan& P, int64_t Fc, const Knobs& k,
                        const std::vector<int32_t> (&reach_ptr)[2], const std::vector<int32_t> (*decide)[2]) {
  Schedule sc;
  sc.Fc = Fc;
  sc.knobs = k;
  sc.sym = P.sym;
  // the launch shapes are decided for the whole analysis' level geometry (a view keeps the full plan's decisions on
  // the fronts it covers: the same kernel form, split and wave count per front, so the same arithmetic); the records'
  // counts are the view's
  sc.level_maxns = P.dec_maxns;
  sc.level_maxf = P.dec_maxf;
  const int L = P.L;
  const int64_t ng = Fc / 64;
  for (int l = 0; l < L; ++l) sc.level_nf.push_back(P.level_ptr[l + 1] - P.level_ptr[l]);
  sc.factor.assign(L, FactorLevel{});
  sc.pair.assign(L, PairLevel{});
  sc.solve[SUBSET_ALL].resize(L);
  for (int l = 0; l < L; ++l) {
    const int nf = P.dec_nf[l], maxns = sc.level_maxns[l];
    const SolveLevel all = sc.solve[SUBSET_ALL][l] = solve_level(sc, l, nf, sc.level_nf[l]);
    FactorLevel& f = sc.factor[l];
    f.nf = sc.level_nf[l];
    f.maxns = maxns;
    f.fused0 = l == 0 && P.fused0 && k.front0;
    f.f0_small = f.fused0 ? P.f0_small : 0;
    f.lds = P.sym && maxns <= 64 &&
            (k.fac_lds > 0 ? maxns >= k.fac_lds : k.fac_lds < 0 && maxns >= 16 && nf * ng * FAC_G < k.fac_lds_wg);
    // lane groups per wave of the symmetric A11 kernel: FAC_G; fac_gbig on the levels with a pivot block of more
    // than fac_g_ns pivots, whose long chains gain from more row slots per wave (the deep tree's level 25 with its
    // 76-pivot separator at 2,048 frequencies: 0.61 -> 0.41 ms with 4; the levels of 2-3 fronts of <= 35 pivots
    // below it were slower with 4); raised to 4 / 8 while the launch has fewer than fac_g_wg workgroups (default off)
    f.G = (P.sym && maxns > k.fac_g_ns) ? k.fac_gbig : FAC_G;
    while (P.sym && f.G < 8 && nf * ng * f.G < k.fac_g_wg) f.G *= 2;
    // panel: enough workgroups (front x 16 frequencies) to fill the chip -> one wave each (no idle waves at the
    // block barriers); few large fronts -> more waves (symmetric kernel: up to 16 waves -- the top levels' few
    // fronts are latency-bound, every wave more takes rows off each wave's serial chain)
    const int64_t wgs = nf * ng * f.G, wfill = (4096 + wgs - 1) / wgs;
    f.waves = (int)std::max<int64_t>(1, std::min<int64_t>(P.sym ? k.fac_wmax : all.level_w, wfill));
    f.nasm = P.asm_ptr[l + 1] - P.asm_ptr[l];
    f.nitems = P.item_ptr[l + 1] - P.item_ptr[l];
    f.nblocks = P.blk_ptr[l + 1] - P.blk_ptr[l];
    f.ntiles = P.tile_ptr[l + 1] - P.tile_ptr[l];
    f.off_small = maxns <= 8;
    // the software-pipelined L21 prefix on the launches with few waves (symmetric analyses, not the SMALL form)
    f.off_pu = P.sym && !f.off_small && P.dec_nitems[l] * ng < k.off_pu_waves ? 3 : 2;   // the full plan's item count

    PairLevel& p = sc.pair[l];
    p.nf = sc.level_nf[l];
    p.small = sc.level_maxf[l] <= k.us2_small;
    p.tiny = k.us2_tiny > 0 && maxns <= k.us2_tiny ? (maxns <= 4 ? 4 : 8) : 0;
    const bool nar = nf * ng < k.us2_nar;
    p.split = nar ? std::max(2, all.split_L) : all.split_L;
    if (p.tiny > 0 && p.split <= 1) {   // every pivot block of the level <= tiny: one wave per (front, group)
      p.form = p.tiny == 4 ? PAIR_TINY4 : PAIR_TINY8;
      p.waves = 4;
      continue;
    }
    p.upd = p.split <= 1 ? UPD_NONE : nar ? UPD_COLS : UPD_ROWS;
    if (nar) p.RB = ceil_div(maxns, UPC_SR);
    if (nar && k.us2_rl && maxns <= 16 * RL_WMAX) {   // k_usolve2_rl: at most 4 rows per lane slot
      p.form = PAIR_RL;
      p.rpl = rl_rpl(maxns);
      p.waves = rl_waves(maxns);
    } else {
      p.form = p.small ? PAIR_SMALL : PAIR_BIG;
      p.waves = all.waves;
    }
  }
  schedule_reach(sc, reach_ptr, decide);
  return sc;
}

std::string check_schedule(const Symbolic& S, const Plan& P, const Schedule& sc) {
  char buf[256];
  auto bad = [&](const char* what, int l, int64_t v, int64_t lim) {
    snprintf(buf, sizeof buf, "schedule, level %d: %s %lld against %lld", l, what, (long long)v, (long long)lim);
    return std::string(buf);
  };
  const int L = P.L;
  if ((int)sc.factor.size() != L || (int)sc.pair.size() != L || (int)sc.chain.size() != L) return "schedule levels";
  for (const auto& v : sc.solve)
    if ((int)v.size() != L) return "schedule levels";
  auto waves_ok = [](int w, int hi) { return w >= 1 && w <= hi; };
  for (int l = 0; l < L; ++l) {
    // the records are decided for the analysis' level geometry, which bounds the view's
    const int nf = P.level_ptr[l + 1] - P.level_ptr[l], maxns = P.dec_maxns[l], maxf = P.dec_maxf[l];
    if (P.level_maxns[l] > maxns || P.level_maxf[l] > maxf || nf > P.dec_nf[l]) return bad("level geometry", l, P.level_maxns[l], maxns);
    const FactorLevel& f = sc.factor[l];
    const PairLevel& p = sc.pair[l];
    const ChainLevel& c = sc.chain[l];
    if (f.nf != nf || p.nf != nf || sc.solve[SUBSET_ALL][l].nf != nf) return bad("fronts", l, f.nf, nf);
    if (f.maxns != maxns) return bad("largest pivot block", l, f.maxns, maxns);
    if (nf == 0) {           // a view without a front on this level: no record may launch
      if (c.nmax != 0 || f.nasm != 0 || f.nitems != 0 || f.nblocks != 0 || f.ntiles != 0) return bad("empty level", l, c.nmax, 0);
      for (const auto& v : sc.solve)
        if (v[l].nf != 0) return bad("empty level", l, v[l].nf, 0);
    }
    if (f.lds && (maxns > 64 || fac_lds_bytes(maxns) > LDS_BYTES)) return bad("A11 LDS", l, maxns, 64);
    if (f.fused0 && (l != 0 || !P.fused0 || f.f0_small != P.f0_small)) return bad("fused level", l, f.fused0, 0);
    if (f.G != 2 && f.G != 4 && f.G != 8) return bad("lane groups", l, f.G, 8);
    if (!waves_ok(f.waves, 16)) return bad("panel waves", l, f.waves, 16);
    if (f.off_pu == 3 ? f.off_small != 0 : f.off_pu != 2) return bad("L21 prefix", l, f.off_pu, 3);
    // the split parts' strides: the rows [lo, hi) of a front, `rows` per step, every one exactly once
    std::vector<int> seen;
    auto covered = [&](int lo, int hi, int rows, int split) {
      seen.assign(std::max(hi, 0), 0);
      for (int part = 0; part < split; ++part)
        for (int w = 0; w < SPLIT_W; ++w)
          for (int i0 = lo + rows * (part * SPLIT_W + w); i0 < hi; i0 += rows * SPLIT_W * split)
            for (int r = 0; r < rows && i0 + r < hi; ++r) ++seen[i0 + r];
      for (int a = lo; a < hi; ++a)
        if (seen[a] != 1) return false;
      return true;
    };
    auto split_ok = [&](int split, bool pivots, int rows) {   // over every front of the level
      if (split < 1 || split > 16) return false;
      for (int e = P.level_ptr[l]; e < P.level_ptr[l + 1]; ++e) {
        const Front& F = S.fronts[P.level_fronts[e]];
        if (!(pivots ? covered(0, F.ns, rows, split) : covered(F.ns, F.f, rows, split))) return false;
      }
      return true;
    };
    // paired top-down
    if (p.form == PAIR_TINY4 || p.form == PAIR_TINY8) {
      const int t = p.form == PAIR_TINY4 ? 4 : 8;
      if (maxns > t || p.tiny != t || p.split > 1 || p.upd != UPD_NONE) return bad("tiny level", l, maxns, t);
    } else {
      if ((p.upd == UPD_NONE) != (p.split <= 1)) return bad("paired update part", l, p.upd, p.split);
      if (p.upd == UPD_ROWS && !split_ok(p.split, true, US2_UPD_SR)) return bad("paired split coverage", l, p.split, 16);
      if (p.upd == UPD_COLS && p.RB * UPC_SR < maxns) return bad("paired row blocks", l, p.RB * UPC_SR, maxns);
      if (p.form == PAIR_RL) {
        if (p.upd != UPD_COLS || maxns > 16 * RL_WMAX || 4 * p.rpl * p.waves < maxns || p.waves > RL_WMAX ||
            (p.rpl != 1 && p.rpl != 2 && p.rpl != 4))
          return bad("right-looking paired level", l, 4 * p.rpl * p.waves, maxns);
      } else if (p.form != (p.small ? PAIR_SMALL : PAIR_BIG)) {
        return bad("paired form", l, p.form, p.small);
      }
    }
    if (!waves_ok(p.waves, 8)) return bad("paired waves", l, p.waves, 8);
    // bottom-up chain
    if (c.nf0 < 0 || c.nf0 > nf || c.nf1 < 0 || c.nf1 > nf || c.nmax != std::max(c.nf0, c.nf1))
      return bad("chain fronts", l, c.nmax, nf);
    if (c.nmax > 0) {
      if (c.nsum != c.nf0 + 3 * c.nf1) return bad("chain slices", l, c.nsum, c.nf0 + 3 * c.nf1);
      if ((c.rows == ROWS_NONE) != (c.split <= 1)) return bad("chain update rows", l, c.rows, c.split);
      if ((c.form != CHAIN_PLAIN) != (c.rows == ROWS_ZC)) return bad("chain form", l, c.form, c.rows);
      if (c.rows == ROWS_Z && !split_ok(c.split, false, SRB)) return bad("chain split coverage", l, c.split, 16);
      if (c.rows == ROWS_ZC && c.RB * LRC_SR < maxf - 1) return bad("chain row blocks", l, c.RB * LRC_SR, maxf - 1);
      if (c.form == CHAIN_NAR && (!ls_nar_fits(maxns) || c.lds_bytes != (int64_t)maxns * 64 * 16))
        return bad("chain LDS", l, c.lds_bytes, LS_NAR_DYN_MAX);
      if (c.form == CHAIN_RL && (maxns > 16 * RL_WMAX || 4 * c.rpl * c.waves < maxns || c.waves > RL_WMAX ||
                                 (c.rpl != 1 && c.rpl != 2 && c.rpl != 4)))
        return bad("right-looking chain level", l, 4 * c.rpl * c.waves, maxns);
      if (!waves_ok(c.waves, 8)) return bad("chain waves", l, c.waves, 8);
    }
    // unpaired passes
    for (const auto& v : sc.solve) {
      const SolveLevel& r = v[l];
      if (r.nf < 0 || r.nf > nf) return bad("solve fronts", l, r.nf, nf);
      if (!waves_ok(r.waves, 8) || r.level_w > r.waves) return bad("solve waves", l, r.waves, 8);
      if (!split_ok(r.split_L, false, SRB) || !split_ok(r.split_U, true, SRB)) return bad("solve split coverage", l, r.split_L, 16);
    }
  }
  return "";
}

}  // namespace pfr
