// Host-side launch plans of the numeric factorisation and solves: everything libpfr derives from the symbolic
// analysis before any device work -- level tables, gather records of every kernel class, Dirichlet lists,
// compressed rows / columns, the contraction's entry list, reach lists -- and the element counts of every
// device buffer a solver allocates.  HIP-free (plain C++17): pfr_solver_create (api.cpp) uploads a Plan,
// and the sanitizer driver (asan_driver.cpp, tests/test_asan_host.py) builds plans for every engine shape
// under -fsanitize=address,undefined and checks each index a launch will use against the buffer it addresses
// (check_plan).  Which kernel form every tree level launches, with what grid, block and LDS size, is decided here
// too, once per solver: level_schedule turns the launch-shape knobs (Knobs) and the level geometry into one record
// per pass and level (Schedule).  The level loops of api.cpp walk those records, the launchers (kernels.hip) map
// a record to a kernel instantiation, check_schedule checks every record, and pfr_symbolic_schedule /
// pfr_solver_schedule hand the same records to the tests -- so the checks, the tests and the launches cannot drift
// apart.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "symbolic.hpp"

namespace pfr {

// layouts of HIP's int2 / int4 (device records are uploaded byte for byte)
struct I2 {
  int32_t x, y;
};
struct I4 {
  int32_t x, y, z, w;
};

// ---- kernel shape constants (device_types.hpp / kernels.hip use these)
// Schur super-tile: a wavefront = SCHUR_QG frequencies x (SCHUR_SR x SCHUR_SC) lane groups, each lane group one
// SCHUR_TM x SCHUR_TN register tile.  Lane = frequency, one 4 x 4 tile per wave (measured 10 % faster than 16
// frequencies x a 2 x 2 arrangement of 4 x 4 tiles).
constexpr int SCHUR_SR = 1, SCHUR_SC = 1, SCHUR_QG = 64 / (SCHUR_SR * SCHUR_SC);
constexpr int SCHUR_TM = 4, SCHUR_TN = 4;
static_assert(SCHUR_SR * SCHUR_SC * SCHUR_QG == 64, "one wavefront per super-tile");
constexpr int SCHUR_TILE = SCHUR_TM * SCHUR_TN * SCHUR_SR * SCHUR_SC;   // first-source ids per tile
constexpr int SCHUR_BLK = 16;                 // k_schur_sym_blk block edge (16 waves x 4 x 4 tiles)
constexpr int SCHUR_BLK_IDS = 16 * SCHUR_BLK; // first-source ids per block (wave x position)
// Off-diagonal panel kernel: a wave = OFF_G lane groups of 64 / OFF_G frequencies, OFF_RPL rows (columns) per
// lane.  Lane = frequency, two rows per lane (measured best of 1 / 2 lane groups and 1 / 2 / 4 rows per lane).
constexpr int OFF_G = 1;
constexpr int OFF_RPL = 2;
constexpr int FAC_G = 2;                      // A11 LU: lane groups per wave (64 / FAC_G frequencies each)
constexpr int MAX_FRONT = 1024;               // largest front the solve kernels stage index lists for in LDS
constexpr int NKC = 5;                        // factorisation kernel classes: assembly, A11 LU, L21 rows, Schur
                                              // blocks, Schur tiles
constexpr int FN_PARTS_HOST = 16;             // k_fn_dot partials per frequency group (kernels.hip: FN_PARTS)
constexpr int REFINE_CAP = 4;                 // groups of the selective adjoint refinement per chunk
constexpr int SPLIT_W = 4;                    // waves per workgroup of the split solve update parts
constexpr int SRB = 4;                        // rows per step of lsolve_rows / usolve_upd (the split parts' stride)
constexpr int US2_UPD_SR = 2;                 // pivot rows per step of k_usolve2_upd
// right-looking pivot-block solves (k_usolve2_rl / k_lsolve_rl_z): RL_Q frequencies per workgroup, at most RL_WMAX
// waves of 4 row slots, 1 / 2 / 4 rows per lane slot
constexpr int RL_Q = 16, RL_WMAX = 8;
inline int rl_rpl(int maxns) { return maxns <= 4 * RL_WMAX ? 1 : maxns <= 8 * RL_WMAX ? 2 : 4; }
inline int rl_waves(int maxns) { return std::min(RL_WMAX, (maxns + 4 * rl_rpl(maxns) - 1) / (4 * rl_rpl(maxns))); }
constexpr int UPC_SR = 2, UPC_W = 8;          // k_usolve2_updc: pivot rows per workgroup, waves
constexpr int LRC_SR = 4, LRC_W = 4;          // k_lsolve_rows_zc: update rows per workgroup, waves
constexpr int CEG_EW = 8;                     // entries per wave of k_contract_eg
constexpr int64_t LDS_BYTES = 160 * 1024;

// ---- launch geometry shared by the launchers and the checks
inline int residual_parts(int n) { return (int)std::min<int64_t>((n + 3) / 4, 256); }   // k_residual grid.x
inline int contract_eg_parts(int nent) { return ((nent + CEG_EW - 1) / CEG_EW + 3) / 4; }   // k_contract_eg grid
// k_contract_q grid.x: at least 16 entries per wave, never more workgroups than k_residual's (kpart holds them)
inline int contract_q_parts(int n, int nent) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(residual_parts(n), ((int64_t)nent + 63) / 64));
}
// k_contract_mass: MASS_NM component columns (fewer registered: zero columns), MASS_U list entries per batch; grid.x
// from the contraction entries (not from a view's list): at least 16 entries per wave, never more workgroups than
// k_residual's (mpart lives in kpart)
constexpr int MASS_NM = 4, MASS_U = 4;
inline int contract_mass_parts(int n, int nlist) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(residual_parts(n), ((int64_t)nlist + 63) / 64));
}
// dynamic LDS of k_factor_sym_lds for a level whose largest pivot block is maxns (triangle + 8 W columns)
inline int64_t fac_lds_bytes(int maxns) { return ((int64_t)maxns * (maxns + 1) / 2 + (int64_t)maxns * 8) * 16; }
// k_lsolve_level_z's NAR form: the level's largest pivot block's values in dynamic LDS (ns x 64 x 16 B), beside
// the frontal gather's static index staging (~36 KiB)
constexpr int64_t LS_NAR_DYN_MAX = 112 * 1024;
inline bool ls_nar_fits(int maxns) { return (int64_t)maxns * 64 * 16 <= LS_NAR_DYN_MAX; }
// waves per workgroup for a level whose largest front is maxf
inline int waves_for(int maxf) { return std::max(1, std::min(8, (maxf + 23) / 24)); }
// Workgroups per (front, frequency group) for the update part of a solve launch over nf fronts: 1 when the
// launch already has `target` workgroups, else enough to reach it (at most 16)
inline int solve_split(int64_t nf, int64_t Fc, int target) {
  const int64_t wgs = nf * (Fc / 64);
  if (target <= 0 || wgs <= 0 || wgs >= target) return 1;
  return (int)std::min<int64_t>(16, (target + wgs - 1) / wgs);
}
// Waves per workgroup of a solve launch over nf fronts of a level with size-based count level_w, raised (up to
// wmax) when the launch has too few workgroups to fill the chip
inline int solve_waves(int level_w, int64_t nf, int64_t Fc, int wmax) {
  const int64_t wgs = std::max<int64_t>(1, nf * (Fc / 64));
  const int64_t fill = (4096 + wgs - 1) / wgs;
  return (int)std::max<int64_t>(level_w, std::min<int64_t>(wmax, fill));
}

// The bottom level fused (k_front0): symmetric analyses whose level-0 fronts (leaves) all have at most F0_NS pivots
// and F0_RM update rows -- per (front, frequency) A11, L21 and the update block formed in registers, one pass
constexpr int F0_NS = 4, F0_RM = 10;

struct Plan {
  int L = 0;                             // levels
  bool sym = false;
  // the fronts the plan covers, level by level: every front of the analysis, or (a view, build_plan's mask) whole
  // trees of its elimination forest -- the levels keep their numbers, a level may hold no front
  std::vector<char> active;              // per front (all 1 without a mask)
  std::vector<int32_t> level_ptr, level_fronts, level_maxf;
  std::vector<int32_t> level_maxns;      // largest pivot block per level
  // the level geometry of the whole analysis (every front, whatever the mask): what level_schedule decides the
  // launch shapes for
  std::vector<int32_t> dec_nf, dec_maxns, dec_maxf, dec_nitems;   // fronts, largest pivot block / front, L21 items
  std::vector<char> blk_front;           // front's Schur complement by the block kernel
  // Schur tiles (front, i0, j0, -) by level, per tile SCHUR_TILE first child sources, overflow ranges
  std::vector<I4> tiles;
  std::vector<int32_t> g1, gxp, tile_ptr;
  std::vector<I2> gx;                    // (lane group * TM TN + position, element id)
  // Schur blocks (front, i0, j0, -) by level, per block SCHUR_BLK_IDS first child sources, overflow ranges
  std::vector<I4> blocks;
  std::vector<int32_t> bg1, bgxp, blk_ptr;
  std::vector<I2> bgx;                   // (wave * 16 + position, element id)
  // A11 assembly records (dst, nz, first child source, -) in chunks of 8, levels padded to 8
  std::vector<I4> asm_rec;
  std::vector<int32_t> asm_xp, asm_ptr;  // per chunk: overflow range; per level: first record
  std::vector<I2> asm_x;                 // (record within the chunk, element id)
  // L21 (U12) items (front, first row, kind, record offset) by level; per item x row slot x pivot (nz, source)
  std::vector<I4> items;
  std::vector<I2> orec;
  std::vector<int32_t> oxp, item_ptr;
  bool fused0 = false;                   // level 0 through k_front0 (operator-form sweeps)
  int f0_small = 0;                      // the first f0_small listed fronts have <= 2 pivots
  std::vector<int32_t> f0_front, f0_ptr; // level-0 fronts (<= 2 pivots first); their first record
  std::vector<int32_t> f0_nz;            // per front: A11 lower (a >= b) then the L21 rows: original nz or -1
  std::vector<I2> ox;                    // (pivot * OFF_G OFF_RPL + row slot, element id)
  // algorithmic bytes per frequency, level and kernel class (operator-form sweeps)
  std::vector<std::array<int64_t, NKC>> lev_bytes;
  // symmetric mode: Dirichlet decoupling lists
  int n_dir = 0, n_crow = 0;
  std::vector<I2> dir, ce, de;           // (permuted node, diagonal nz); (Dirichlet slot, nz); (permuted row, nz)
  std::vector<int32_t> crow, cptr_dir, dptr, cslot;
  // permuted matrix compressed by rows and by columns (ptr, index, nz)
  std::vector<int32_t> rptr, ridx, rnz, cptr, cidx, cnz;
  // contraction entries: per permuted row a pseudo-entry (-1, -1, -1, i), then (column, nz of (i, j) or -1, nz of
  // (j, i) or -1, i); padded by 4 entries
  std::vector<I4> uent;
  int n_uent = 0;
};

// Element counts of the device buffers a solver with chunk Fc allocates (api.cpp allocates exactly these)
struct Workspace {
  int64_t F = 0, WV = 0, nvec = 0;       // factor entries x Fc, total rows x Fc, one n x Fc vector
  int64_t n_nvec = 0;                    // n-vectors: X, Y, XA, G, Y2, XR, Gx
  int64_t cpart = 0, kpart = 0, partial = 0, berr_acc = 0, gind = 0;
  int64_t WVk = 0, YVk = 0, fn_parts = 0, fcoef = 0, Bc = 0;
  int64_t bytes = 0;                     // all of it (pfr_solver_workspace_bytes)
};
Workspace workspace(const Symbolic& S, int64_t Fc, int n_crow);

// Builds the plan (blk_min: Knobs::blk_min); returns 0, or non-zero with err set (a front too large for the kernels,
// int32 overflow).  mask (per front, may be NULL: every front): the gather records of the factor classes, the level
// lists and the level geometry over the masked fronts only -- a view of the plan; the mask must hold whole trees
// (a front with its parent).  The Dirichlet lists, compressed rows / columns and contraction entries do not depend
// on it.
int build_plan(const Symbolic& S, int blk_min, Plan& P, std::string& err, const std::vector<char>* mask = nullptr);

// The trees of the elimination forest that carry load ("Pruning"): per front 1 when its tree
// holds a permuted row with a non-zero entry of rhs_perm (the right-hand side vector, permuted) or a coupled row of a
// Dirichlet node whose entry of rhs_perm is non-zero (the analysis' coupling lists, by value), and the decoupled
// Dirichlet nodes whose column reaches such a tree.  On the other trees the forward solution of the operator right-hand
// side is exactly zero.
std::vector<char> loaded_fronts(const Symbolic& S, const double* rhs_perm);
// The stiffness matrices a residual walk's gradient contraction needs ("Live matrices"), by value:
// stiffness_bits gives per matrix entry nz the set of k with stiff[nz * n_stiff + k] != 0.0 (bit k); live_stiffness
// the union over the entries of the rows a walk visits -- the pivot rows of the fronts in `mask` (a view's walk
// list), every row for mask == NULL.  A matrix outside the set holds exact zeros on every entry the walk multiplies.
std::vector<uint32_t> stiffness_bits(const double* stiff, int64_t nnz, int n_stiff);
uint32_t live_stiffness(const Symbolic& S, const std::vector<char>* mask, const std::vector<uint32_t>& bits);
// The entries the inertia contraction walks (k_contract_mass), by value: the positions e of the
// contraction entries uent[0 .. n_uent) -- in that order -- with an entry (i, j) of A (x, y >= 0) on which some mass
// component is non-zero (on[uent[e].y] != 0; mass_on gives `on` from the (nnz, n_mass) table) and whose row uent[e].w
// is on in row_on (per permuted row; front_rows: the pivot rows of the fronts in a view's mask; NULL: every row).
// Wave w of the launch's 4 contract_mass_parts(n, n_uent) waves owns the entries [w seg, (w + 1) seg), seg =
// mass_segment(n, n_uent) -- whatever the list keeps of them, so that an entry is accumulated by the same wave in the
// same order on every view and a view's rows match the full walk's bit for bit (what it drops adds exact zeros there).
// list: the kept positions wave by wave, each wave's run padded with -1 to whole MASS_U-entry batches (a wave reads a
// batch at once); ptr (waves + 1): each run's first batch; n_list: the kept positions.
struct MassList {
  std::vector<int32_t> list, ptr;
  int n_list = 0;
};
inline int mass_segment(int n, int n_uent) {
  const int64_t waves = 4 * (int64_t)contract_mass_parts(n, n_uent);
  return (int)std::max<int64_t>(MASS_U, ((n_uent + waves - 1) / waves + MASS_U - 1) / MASS_U * MASS_U);
}
std::vector<char> mass_on(const double* mass, int64_t nnz, int n_mass);
std::vector<char> front_rows(const Symbolic& S, const std::vector<char>& mask);
MassList mass_entries(const std::vector<I4>& uent, int n_uent, int n, const std::vector<char>* row_on,
                      const std::vector<char>& on);
// rows of `prows` on fronts of the mask (a reach restricted to a view)
std::vector<int32_t> rows_in(const Symbolic& S, const std::vector<char>& mask, const std::vector<int32_t>& prows);

// The fronts holding the given permuted rows and all their ancestors: per-front flags and the marked fronts
// level by level (level order kept; ptr per level).  front_of_col: the front of each pivot column (permuted).
void reach_lists(const std::vector<int32_t>& front_of_col, const std::vector<int32_t>& front_parent,
                 const std::vector<int32_t>& level_ptr, const std::vector<int32_t>& level_fronts,
                 const std::vector<int32_t>& prows, std::vector<int32_t>& mark, std::vector<int32_t>& list,
                 std::vector<int32_t>& ptr);

// The row selection of a field sweep (pfr_field_sweep): rows[0 .. n_rows) in the caller's numbering, repeats and any
// order allowed, as the permuted rows iperm[rows[j]] the gather kernel reads.  Returns "" or the refusal (no rows, a
// null list, an index outside [0, n)); `out` is complete only on "".
std::string field_rows(const std::vector<int32_t>& iperm, int32_t n_rows, const int32_t* rows, std::vector<int32_t>& out);

// The selection and weights of a field-loss sweep (pfr_field_loss_sweep).  rows as in field_rows, but no row twice (the
// adjoint seed is a scatter); rows NULL: all n rows in order (n_rows ignored, `out` left empty: the caller walks iperm).
// weights (NULL: all 1): one per selected row, finite, >= 0, not all zero; refused together with cotangent (the
// caller's dL/dx carries them).  Returns "" or the refusal; `out` is complete only on "".
std::string field_loss_rows(const std::vector<int32_t>& iperm, int32_t n_rows, const int32_t* rows,
                            const double* weights, bool cotangent, std::vector<int32_t>& out);

// Every index each launch of a solver with chunk Fc takes from the plan, against the buffer it addresses
// (element ids < factor entries, nz < nnz, record offsets and overflow ranges inside their arrays, the
// per-workgroup partial buffers against the grids that write them).  Returns "" or the first violation.
std::string check_plan(const Symbolic& S, const Plan& P, int64_t Fc);

// ---- the launch schedule
// Launch-shape knobs, read from the environment when a solver is created (so that a process can build solvers
// with different settings, e.g. tests forcing each kernel variant).  The measured-slower variants of rounds 1-4
// are in git history.
struct Knobs {
  int solve_wmax = 8;     // PFR_SOLVE_WMAX: waves per solve workgroup, at most
  int fac_wmax = 16;      // PFR_FAC_WMAX: waves per A11 LU workgroup, at most
  int fac_g_wg = 0;       // PFR_FAC_G_WG: k_factor_sym launches below this many workgroups take G = 4 / 8
  int fac_gbig = 4;       // PFR_FAC_GBIG / PFR_FAC_G_NS: k_factor_sym's lane groups per wave on the levels whose
  int fac_g_ns = 64;      // largest pivot block exceeds PFR_FAC_G_NS pivots
  int us2_small = 110;    // PFR_US2_SMALL: largest front of a level the paired top-down solve treats with its
                          // low-register small-front variant
  int split_target = 256; // PFR_SOLVE_SPLIT: solve launches with fewer (front, group) workgroups than this (one per
                          // CU) split their update parts up to about this many workgroups (0: off)
  int us2_nar = 256;      // PFR_US2_NAR: solve launches (paired top-down, bottom-up chain) with fewer (front, group)
                          // workgroups than this take the narrow-level forms -- pivot blocks in LDS, left-looking,
                          // the update parts with their columns split over the waves (k_usolve2_updc + k_usolve2_rl,
                          // k_lsolve_level_z<., true> + k_lsolve_rows_zc); 0: never.  Measured best at 256 for both
                          // passes (1,024 / 4,096: no gain at 512 frequencies, slower at 4,096)
  int fac_lds = -1;       // PFR_FAC_LDS: which levels factor A11 in LDS (k_factor_sym_lds): n > 0 those whose largest
                          // pivot block has at least n pivots, 0 none, -1 auto: the levels on which the global-memory
                          // kernel would get fewer than fac_lds_wg workgroups (the top of the tree in small chunks:
                          // 512 frequencies levels 10-16, 2,048 level 16 -- faster per level there, slower elsewhere;
                          // 512-frequency sweeps 31.8k -> 32.6k freq-solves/s, 4,096 unchanged)
  int fac_lds_wg = 160;   // auto mode threshold (workgroups of k_factor_sym)
  int us2_tiny = 8;       // PFR_US2_TINY (0 / 4 / 8): levels whose pivot blocks are <= this, one wave per front (8: the
                          // bottom two levels at 2,048 frequencies 685 / 612 -> 509 / 489 us)
  int us2_rl = 1;         // PFR_US2_RL: k_usolve2_rl for the narrow levels' paired pivot blocks
  int ls_rl = 1;          // PFR_LS_RL: k_lsolve_rl_z for the bottom-up chain's narrow pivot blocks; on by default on
                          // chunks of up to 1,024 frequencies (512-frequency sweeps forward solves 1.65 -> 1.33 ms per
                          // step; on 2,048-frequency chunks 0.37 -> 0.50 ms per sweep: four slices x 128 groups of 16
                          // frequencies each stage the frontal index chains, profiles/EXPERIMENTS.md, round 6)
  int off_pu_waves = 0;   // PFR_OFF_PU_WAVES: L21 launches with fewer waves run the pipelined prefix; 8,000 by default
                          // on chunks of up to 1,024 frequencies (the narrow levels of C4's per-rank sweeps: 512
                          // frequencies 35.3-35.7k -> 36.2-36.6k freq-solves/s; 2,048-frequency chunks unchanged)
  int front0 = 1;         // PFR_FRONT0=0: level 0 through the four class kernels instead of the fused k_front0
                          // (tests/test_gpu_bitwise.py checks the two give the same factors bit for bit)
  int blk_min = 24;       // PFR_SCHUR_BLK_MIN: update blocks of at least this many rows through the block kernel
};
// The knobs of a solver with chunk Fc from the environment, clamped
Knobs knobs_from_env(int64_t Fc);

// One record per pass and level: everything a launch of that level needs beyond pointers.  Plain int32 columns, in
// this order the rows of pfr_symbolic_schedule / pfr_solver_schedule (include/pfr.h).  nf = 0: the level launches
// nothing in that pass.
struct FactorLevel {
  int32_t nf, maxns;
  int32_t fused0;          // operator-form sweeps run the level through k_front0 (level 0 only)
  int32_t f0_small;        // ... whose first f0_small listed fronts have <= 2 pivots
  int32_t lds;             // A11 by k_factor_sym_lds (else k_factor_sym<G> / k_factor_level)
  int32_t G, waves;        // lane groups per wave and panel waves of the global-memory A11 kernel
  int32_t off_small;       // L21: the SMALL form (pivot blocks <= 8)
  int32_t off_pu;          // L21: 3 = the pipelined prefix (operator-form sweeps), 2 = plain
  int32_t nasm, nitems, nblocks, ntiles;   // assembly records, L21 items, Schur blocks and tiles
};
enum PairForm { PAIR_TINY4, PAIR_TINY8, PAIR_RL, PAIR_SMALL, PAIR_BIG };   // the pivot-block kernel
enum UpdForm { UPD_NONE, UPD_ROWS, UPD_COLS };   // update part: in the level kernel, k_usolve2_upd, k_usolve2_updc
struct PairLevel {         // paired top-down pass (sym_top_down_pair), over all fronts of the level
  int32_t nf, form, upd;
  int32_t split;           // workgroups per (front, group) of UPD_ROWS; > 1 whenever the update part runs apart
  int32_t waves;           // of the pivot-block kernel's workgroup
  int32_t rpl;             // PAIR_RL: rows per lane slot (else 0)
  int32_t RB;              // UPD_COLS: row blocks per front (else 0)
  int32_t tiny, small;     // the level's classes under PFR_US2_TINY (0 / 4 / 8) and PFR_US2_SMALL, whichever form runs
};
enum ChainForm { CHAIN_PLAIN, CHAIN_NAR, CHAIN_RL };    // k_lsolve_level_z<., false | true>, k_lsolve_rl_z
enum RowsForm { ROWS_NONE, ROWS_Z, ROWS_ZC };           // update rows: in the level kernel, k_lsolve_rows_z, ..._zc
struct ChainLevel {        // bottom-up chain (fn_bottom_up): slice 0 over reach 0, slices 1-3 over reach 1
  int32_t nf0, nf1, nmax, nsum;
  int32_t form, rows, split, waves;
  int32_t rpl;             // CHAIN_RL (else 0)
  int32_t RB;              // ROWS_ZC (else 0)
  int32_t lds_bytes;       // CHAIN_NAR: dynamic LDS (else 0)
};
struct SolveLevel {        // unpaired passes (solve_all, sym_top_down_support) over one subset of the level's fronts
  int32_t nf;
  int32_t level_w, waves;  // the level's size-based wave count; the launch's
  int32_t split_L, split_U;
};
enum Subset { SUBSET_ALL, SUBSET_REACH0, SUBSET_REACH1 };
struct Schedule {
  // what the reach-dependent records are rebuilt from
  int64_t Fc = 0;
  Knobs knobs;
  bool sym = false;
  std::vector<int32_t> level_nf, level_maxns, level_maxf;
  std::vector<FactorLevel> factor;
  std::vector<PairLevel> pair;
  std::vector<ChainLevel> chain;
  std::vector<SolveLevel> solve[3];      // by Subset
};
template <class R> constexpr int schedule_cols() { return (int)(sizeof(R) / sizeof(int32_t)); }
// Pure: the schedule of a solver with chunk Fc under the knobs k, for the reaches given by their per-level ranges
// (reach_lists' ptr; an empty vector: no front reached)
// decide (a view; NULL: reach_ptr): the full plan's reaches.  A view's records take every launch-shape decision as
// the full plan takes it -- from the analysis' level geometry (Plan::dec_*) and the full reaches -- and only their
// counts from the view, so each front it covers runs the arithmetic it runs under the full plan, in the same order
Schedule level_schedule(const Symbolic& S, const Plan& P, int64_t Fc, const Knobs& k,
                        const std::vector<int32_t> (&reach_ptr)[2], const std::vector<int32_t> (*decide)[2] = nullptr);
// The records that depend on the reaches (chain, solve[SUBSET_REACH*]) again, after a reach changed
void schedule_reach(Schedule& sc, const std::vector<int32_t> (&reach_ptr)[2],
                    const std::vector<int32_t> (*decide)[2] = nullptr);
// Every record against the kernels' limits (LDS sizes, rows per lane slot, wave counts, the row blocks and the
// split parts covering every row once).  Returns "" or the first violation.
std::string check_schedule(const Symbolic& S, const Plan& P, const Schedule& sc);

}  // namespace pfr
