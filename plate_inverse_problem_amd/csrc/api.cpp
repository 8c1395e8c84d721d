// C ABI of libpfr.so (see include/pfr.h).  Host orchestration of the HIP kernels:
// level-scheduled launches over frequency chunks, workspaces, timing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "launch.hpp"

using pfr::DevPattern;
using pfr::Front;
using pfr::Symbolic;
using pfr::Walk;

struct pfr_symbolic {
  Symbolic S;
};

namespace {
thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

// after a group of launches: a refused launch configuration (pfr::launch_refused) or a launch error
#define LAUNCH_TRY()                                                                      \
  do {                                                                                    \
    if (const char* _k = pfr::launch_refused())                                           \
      return fail(PFR_ERR_HIP, std::string("hipFuncSetAttribute refused the dynamic LDS size of ") + _k); \
    HIP_TRY(hipGetLastError());                                                           \
  } while (0)

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess)                                                                 \
      return fail(_e == hipErrorOutOfMemory ? PFR_ERR_NOMEM : PFR_ERR_HIP,                \
                  std::string(#expr) + ": " + hipGetErrorString(_e));                     \
  } while (0)

template <class T>
int upload(T** dst, const std::vector<T>& src) {
  *dst = nullptr;
  if (src.empty()) return PFR_OK;
  HIP_TRY(hipMalloc(dst, src.size() * sizeof(T)));
  HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
  return PFR_OK;
}

int64_t round64(int64_t x) { return (x + 63) / 64 * 64; }

}  // namespace

// What the level loops of a sweep walk: the level lists, the gather records of the factor classes, the reaches, the
// row lists derived from them and the launch schedule of a set of whole elimination trees -- every front (the solver
// itself: the full view), the loaded trees (pfr_set_prune: pfr_solver::act) or the unloaded ones (pfr_solver::comp,
// built when pfr_debug_solution completes the adjoint).  All views index the same factor storage and vectors.
struct SolverView {
  std::vector<char> active;             // per front: covered by the view
  std::vector<int32_t> level_ptr;       // per level: first front of the view's list
  std::vector<int32_t> tile_ptr, blk_ptr, asm_ptr, item_ptr;   // per level: first Schur tile / block, A11 record, L21 item
  std::vector<void*> mine;              // device arrays of a view built after the solver (freed with the view)
  int32_t* d_walk = nullptr;            // the residual walks' row list (original order); -1: a row the view skips
  // the stiffness matrices with a non-zero value on an entry of the walk's rows (update_live; all of them until then)
  // and, where the walk's contraction takes the live ones only, the stiffness table compacted to them
  uint32_t live = 0;
  int n_live = 0;
  double* d_se_live = nullptr;          // se_live[nz * n_live + i] on the entries of the walk's rows, or NULL
  // the contraction entries with a non-zero mass component on the walk's rows (update_mass; pfr_set_inertia), padded
  int32_t *d_mlist = nullptr, *d_mptr = nullptr;   // ... and each wave's batch range of it
  int n_mlist = 0, len_mlist = 0;
  int post_n = 0;                       // Dirichlet nodes on the view's fronts, with their column entries
  int2* post_dir = nullptr;             // (k_dirichlet_post over them)
  int32_t* post_dptr = nullptr;
  int2* post_de = nullptr;
  int32_t* d_level_fronts = nullptr;
  int4* d_tiles = nullptr;              // Schur tiles (front, i0, j0, 0), grouped by level
  int4* d_items = nullptr;              // off-diagonal panel items (front, first row/col, kind, record offset)
  int2* d_orec = nullptr;               // per item x lane group x pivot: (nz, first child source) of the entry
  int32_t *d_f0_front = nullptr, *d_f0_ptr = nullptr, *d_f0_nz = nullptr;
  int32_t* d_oxp = nullptr;             // per item: range of further child sources in d_ox
  int2* d_ox = nullptr;                 // (pivot * OFF_G OFF_RPL + row slot, element id)
  int32_t* d_g1 = nullptr;              // per super-tile, lane group, position: first child source (or -1)
  int32_t* d_gxp = nullptr;             // per super-tile: range of further sources in d_gx
  int2* d_gx = nullptr;                 // (lane group * 16 + position, element id) of the rare extra sources
  // symmetric mode, fronts with large update blocks: 16 x 16 Schur blocks (k_schur_sym_blk)
  int4* d_blocks = nullptr;             // (front, i0, j0, 0), grouped by level
  int32_t* d_bg1 = nullptr;             // per block, wave, position: first child source (or -1)
  int32_t* d_bgxp = nullptr;            // per block: range of further sources in d_bgx
  int2* d_bgx = nullptr;                // (wave * 16 + position, element id)
  int4* d_asm = nullptr;                // panel-entry assembly records (dst, nz, first child source, 0), by level
  int32_t* d_asm_xp = nullptr;          // per 8-record chunk: range of further child sources in d_asm_x
  int2* d_asm_x = nullptr;              // (record within chunk, child element id)
  // right-hand-side reach (0 = forward operator rhs, 1 = loss adjoint on the functional support):
  // the fronts holding a support row and their elimination-tree ancestors -- the only fronts
  // whose bottom-up solve can be non-zero (per-front flags + the fronts level by level)
  std::vector<int32_t> level_fronts_host;
  std::vector<char> reach_host[2];
  int32_t* d_reach[2] = {nullptr, nullptr};
  int32_t* d_reach_fronts[2] = {nullptr, nullptr};
  std::vector<int32_t> reach_ptr[2];
  bool fn_ready = false;                // row lists below match the current reaches
  int2* d_fn_rows = nullptr;            // (row, factor element of U(row, row)): pivot rows in both reaches
  int n_fn_rows = 0;
  int32_t* d_sup_rows = nullptr;        // pivot rows of the support-reach fronts
  int n_sup_rows = 0;
  // algorithmic HBM bytes per frequency of each factorisation kernel class, per level (16 B per complex entry
  // loaded or stored; index data is shared by all frequencies and not counted)
  std::vector<std::array<int64_t, pfr::NKC>> lev_bytes;
  // which kernel form every level launches in every pass, with what shape (plan.hpp): built with the view from the
  // launch-shape knobs (sched.knobs, read from the environment when the solver is created), its reach-dependent
  // records again whenever a reach changes (set_reach)
  pfr::Schedule sched;
};

struct pfr_solver : SolverView {
  int device = 0;
  int n = 0;
  int64_t nnz = 0;
  int64_t Fc = 0;  // frequencies per chunk (multiple of 64)
  std::vector<int32_t> perm, iperm;
  DevPattern P{};
  // owned device arrays
  std::vector<void*> owned;
  // pruning (pfr_set_prune): the operator-form sweeps on the loaded trees only.  S: the analysis
  // (kept by symmetric solvers: views are built from it); act: the loaded trees' view, NULL while pruning is off or
  // every tree is loaded; comp: its complement; unl_rows: the pivot rows of the unloaded fronts as [first, last)
  // ranges; unl_dirty: a sweep on the full view (or the accessor's completion) wrote rows of unloaded trees in X / XA,
  // zeroed again before the next pruned sweep; comp_done: the accessor completed the last chunk's adjoint already
  int prune = 0;
  Symbolic S;
  std::vector<pfr::I2> h_dir, h_de;
  std::vector<int32_t> h_dptr;
  std::vector<int32_t> reach_rows[2];   // the rows the full view's reaches were set from
  SolverView* act = nullptr;
  SolverView* comp = nullptr;
  std::vector<std::pair<int32_t, int32_t>> unl_rows;
  bool unl_dirty = false, comp_done = false, last_pruned = false;
  pfr::ChunkOp last_op;                 // the last chunk's operator (the accessor's completion factorises with it)
  hipStream_t last_st = nullptr;        // ... and its stream
  bool last_adj = false;                // ... which solved an adjoint (G holds its seed)
  pfr::Reach last_reach = pfr::REACH_SUPPORT;   // ... over these fronts (a field loss: every front)
  int32_t* d_colptr = nullptr;
  int32_t* d_rowind = nullptr;
  // symmetric mode (options.symmetric): U never formed; Dirichlet nodes decoupled
  bool sym = false;
  int n_dir = 0, n_crow = 0;
  int2* d_dir = nullptr;                // per Dirichlet node: (permuted node, diagonal entry)
  int32_t* d_crow = nullptr;            // coupled rows (permuted)
  int32_t* d_cptr_dir = nullptr;        // their entry ranges in d_ce
  int2* d_ce = nullptr;                 // (Dirichlet slot, entry) by coupled row
  int32_t* d_dptr = nullptr;            // per Dirichlet node: entry range in d_de
  int2* d_de = nullptr;                 // (permuted row, entry) by Dirichlet node
  int32_t* d_cslot = nullptr;           // per permuted row: coupled-row slot or -1
  double2* Bc = nullptr;                // forward right-hand-side corrections (n_crow x Fc)
  std::vector<int32_t> front_of_col, front_parent, front_ns, front_f;
  // functional from the bottom-up passes (symmetric loss / correction sweeps, PFR_FN_DOT, default on):
  // slices 1-3 of the forward bottom-up chain solve L w_k = a_k over the support's reach; F_k = w_k^T
  // diag(U)^-1 y; the adjoint's bottom-up result = sum_k c_k w_k -- no top-down pass over the support's
  // fronts and no separate adjoint bottom-up pass
  int fn_dot = 1;
  std::vector<int32_t> front_off, front_col0;
  std::vector<double> a_perm;           // 3 x n: a_k at the permuted support rows
  double* d_aP = nullptr;               // device copy of a_perm
  int32_t* d_noslot = nullptr;          // n x -1 (no coupling slot: slices 1-3)
  double2* WVk = nullptr;               // 3 x total_rows x Fc (slices 1-3 work vectors)
  double2* YVk = nullptr;               // 2 x n x Fc (slices 2, 3 solutions; slice 1's is Y2)
  double2* fn_parts = nullptr;          // FN_PARTS x 3 x Fc
  double2* fcoef = nullptr;             // 3 x Fc
  // the gradient contraction fused into the forward residual walk (PFR_CONTRACT_WALK, default on; needs
  // the functional correction's walk): per (workgroup, k, frequency) sums, reduced with m_q by k_reduce_q
  int contract_walk = 1;
  double2* kpart = nullptr;
  // ... over the live stiffness matrices of the view's walk only (PFR_CONTRACT_LIVE, default on; 0: all n_stiff);
  // stiff_bits: per matrix entry the k with a non-zero value (pfr_set_stiffness); live_unroll: the six-matrix walk's
  // gather batch (PFR_LIVE_UNROLL, 4 / 8); d_live_bad: set by k_gather_live on a non-zero value in a dropped matrix
  int contract_live = 1, live_unroll = 8;
  std::vector<uint32_t> stiff_bits;
  int32_t* d_live_bad = nullptr;
  double2 *F = nullptr, *WV = nullptr, *X = nullptr, *Y = nullptr, *XA = nullptr, *G = nullptr, *Y2 = nullptr;
  double2* XR = nullptr;                // refinement correction of the adjoint (PFR_CHECK_REFINE)
  // Hessian sweep: permuted matrix by rows and by columns ((ptr, index, nz) each),
  // tangent solution / adjoint vectors, combined tangent operators (lazily allocated)
  int32_t *d_rptr = nullptr, *d_ridx = nullptr, *d_rnz = nullptr;
  // d_walk (SolverView): rows (permuted numbering) in original order: the residual walks' order (mesh-local
  // gathers, whatever the ordering)
  int32_t *d_cptr = nullptr, *d_cidx = nullptr, *d_cnz = nullptr;
  double2 *DX = nullptr, *DL = nullptr, *Kdir = nullptr;
  // gradient contraction entries (k_contract_eg): per permuted row a pseudo-entry (-1, -1, -1, i), then
  // (column, nz of (i, j) or -1, nz of (j, i) or -1, i) over the union of the row's and the column's patterns
  int4* d_uent = nullptr;
  int n_uent = 0;
  double* d_se = nullptr;               // entry-ordered S_k(i, j) (pfr_set_stiffness)
  // inertia rows (pfr_set_inertia): the registered mass components G_j and their load weights d_j, the entry-ordered
  // copy G_j(i, j) padded to MASS_NM columns, per matrix entry whether some component is non-zero there, and the
  // host copy of the contraction entries the views' lists are compacted from
  const double* mass = nullptr;
  int n_mass = 0;
  pfr::MassWeights mass_d{};
  double* d_me = nullptr;
  std::vector<char> mass_nz;
  std::vector<pfr::I4> h_uent;
  int n_kdir = 0;
  double2 *partial = nullptr, *tq = nullptr;
  double *freqs = nullptr, *loss_terms = nullptr;
  // functional correction (PFR_CHECK_CORRECT): fr of the solve, per-frequency cotangent scale, and
  // the residual walk's per-workgroup dot-product partials (residual_parts(n) x Fc)
  double* fr0 = nullptr;
  double2* h0 = nullptr;                // the complex response of the solve (pfr_sweep_complex; allocated on first use)
  // the field loss (pfr_field_loss_sweep; allocated on first use): the tiles' partial sums (fpart_cap doubles) and
  // the seed coefficients per frequency (3 x Fc)
  double* fpart = nullptr;
  int64_t fpart_cap = 0;
  double* fseed = nullptr;
  double2 *mscale = nullptr, *cpart = nullptr;     // mscale complex: the solve-error scale (k_correct_finish)
  int scale_corr = 1;                   // PFR_SCALE_CORR: the solve-error scale of the loss sweeps' cotangent
  int32_t* flags = nullptr;
  // operator / rhs / functional / stiffness state
  const double2* K = nullptr;
  const double* M = nullptr;
  double* rhsP = nullptr;
  int32_t* rhs_sup = nullptr;
  double* rhs_val = nullptr;
  int n_rhs_sup = 0;
  std::vector<double> rhs_host;         // last Dirichlet vector uploaded (original order)
  double beta_re = 0, beta_im = 0, mass_sum = 0;
  bool has_rhs = false;
  pfr::FunctionalArgs fn{};
  bool has_fn = false;
  const double* stiff = nullptr;
  int n_stiff = 0;
  pfr::CoefPack e{};
  // timing: bit 0 = phases, bit 1 = factorisation kernel classes (5 events per level).
  // Events of every chunk of the last call are kept and read only when the caller
  // asks (pfr_last_timings): no host synchronisation inside a call, so solvers on
  // different streams overlap.
  struct ChunkEvents {
    hipEvent_t ev[6]{};
    std::vector<hipEvent_t> kev;        // factorisation kernel classes: NKC + 1 events per level
    bool used[5]{};
    bool f0 = false;                    // level 0 ran fused (k_front0): its launches are all class 0
  };
  int timing = 0;
  std::vector<ChunkEvents> tev;
  int n_tev = 0;                        // chunks recorded by the last call
  pfr::Workspace ws;                    // element counts of the chunk buffers (plan.cpp; what is allocated)
  int res_unroll = 8;                   // PFR_RES_UNROLL: entries per gather batch of the adjoint check walk (4 / 8)
  // backward-error checks (pfr_set_check): PFR_CHECK_* bits, tolerance, optional per-item output;
  // per-frequency maxima scratch, forward and adjoint (kept zero between checks)
  int check_mode = 0;
  double check_tol = 1e-10;
  double refine_tol = 2e-8;             // PFR_CHECK_REFINE_ADJ group threshold (pfr_set_refine_tol)
  double* gind = nullptr;               // per 64-frequency group: largest |correction| / |fr| of the chunk
  int32_t* glist = nullptr;             // the groups whose adjoint is refined (REFINE_CAP, -1: none)
  double2* Gx = nullptr;                // the fr seed of the forward solution (support rows; zero elsewhere)
  double* berr_out = nullptr;
  double* d_berr_acc = nullptr;
  // sweep graphs (PFR_GRAPH=1): a pfr_sweep called again with the same arguments and solver state (gen:
  // bumped by every setter that changes what a sweep enqueues) is captured once into a hipGraph and from then on
  // replayed with one hipGraphLaunch instead of ~160-290 kernel launches; any other sweep runs the launches
  // directly.  graph_off: a capture failed on this solver, no further attempts.
  int graph_mode = 0;
  bool graph_off = false;
  uint64_t gen = 0;
  std::array<uint64_t, 14> gkey{};
  bool gkey_valid = false;
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  int64_t graph_launches = 0;           // sweeps replayed from the graph (pfr_sweep_graph_launches)
  // host tables of pfr_combine_batch (slot 0), pfr_population_sweep (slot 1) and pfr_field_sweep /
  // pfr_field_loss_sweep (slot 2: the row selection, behind the weights) on their way to the device: a pinned
  // staging block, its device copy and the event after the copy (waited for before the block is refilled)
  struct Stage {
    void* host = nullptr;
    void* dev = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool busy = false;
  } stage[3];

  void drop_graph() {
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (graph) (void)hipGraphDestroy(graph);
    gexec = nullptr;
    graph = nullptr;
  }
  ~pfr_solver() {
    drop_graph();
    delete act;    // their device arrays are in `owned`
    delete comp;
    for (void* p : owned) (void)hipFree(p);
    for (auto& g : stage) {
      if (g.host) (void)hipHostFree(g.host);
      if (g.dev) (void)hipFree(g.dev);
      if (g.ev) (void)hipEventDestroy(g.ev);
    }
    for (auto& c : tev) {
      for (auto& x : c.ev)
        if (x) (void)hipEventDestroy(x);
      for (auto& x : c.kev)
        if (x) (void)hipEventDestroy(x);
    }
  }
  template <class T>
  int alloc(T** p, int64_t count) {
    *p = nullptr;
    if (count <= 0) return PFR_OK;
    HIP_TRY(hipMalloc(p, count * sizeof(T)));
    owned.push_back(*p);
    return PFR_OK;
  }
  template <class T>
  int up(T** p, const std::vector<T>& v) {
    int rc = upload(p, v);
    if (rc == PFR_OK && *p) owned.push_back(*p);
    return rc;
  }
  // a plan record array (pfr::I2 / I4) as its HIP vector type (same layout), never empty on the device
  template <class D, class H>
  int up_rec(D** p, const std::vector<H>& v, H pad) {
    static_assert(sizeof(D) == sizeof(H), "record layout");
    std::vector<H> w(v);
    if (w.empty()) w.push_back(pad);
    *p = nullptr;
    HIP_TRY(hipMalloc(p, w.size() * sizeof(H)));
    owned.push_back(*p);
    HIP_TRY(hipMemcpy(*p, w.data(), w.size() * sizeof(H), hipMemcpyHostToDevice));
    return PFR_OK;
  }
};

namespace {

int64_t workspace_bytes(const Symbolic& S, int64_t Fc) {
  int n_crow = 0;                     // coupled rows (Dirichlet decoupling): count as in build_plan
  for (size_t c = 0; c < S.cpl_p.size(); ++c) n_crow += c == 0 || S.cpl_p[c] != S.cpl_p[c - 1];
  return pfr::workspace(S, Fc, S.symmetric ? n_crow : 0).bytes;
}

// start the timing record of a new chunk (events created once per chunk slot)
int begin_chunk(pfr_solver* s) {
  if (!s->timing) return PFR_OK;
  if ((int)s->tev.size() <= s->n_tev) {
    s->tev.emplace_back();
    for (auto& e : s->tev.back().ev) HIP_TRY(hipEventCreate(&e));
  }
  auto& c = s->tev[s->n_tev];
  const size_t nk = (pfr::NKC + 1) * (s->level_ptr.size() - 1);
  while ((s->timing & 2) && c.kev.size() < nk) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    c.kev.push_back(e);
  }
  return PFR_OK;
}

void record(pfr_solver* s, int i, hipStream_t st) {
  if (s->timing) (void)hipEventRecord(s->tev[s->n_tev].ev[i], st);
}

int finish_timing(pfr_solver* s, const bool* used) {
  if (!s->timing) return PFR_OK;
  for (int i = 0; i < 5; ++i) s->tev[s->n_tev].used[i] = used[i];
  ++s->n_tev;
  return PFR_OK;
}

void reset_timing(pfr_solver* s) { s->n_tev = 0; }

// The operator and the operator right-hand side of the chunk starting at q0 (pfr::ChunkOp), built once per chunk and
// passed to everything that launches on it: the solver's K and rhs scale, or in a population sweep (pop != NULL: the
// sweep's group table, a device table padded to whole chunks; chunks start at multiples of Fc) the members'
// operators popK and the chunk's part of the table
pfr::ChunkOp chunk_op(const pfr_solver* s, const double2* popK = nullptr, const pfr::PopArgs* pop = nullptr,
                      int64_t q0 = 0) {
  pfr::ChunkOp op{.K = pop ? popK : s->K, .M = s->M, .freqs = s->freqs, .rhsP = s->rhsP, .beta_re = s->beta_re,
                 .beta_im = s->beta_im, .mass_sum = s->mass_sum};
  if (pop) {
    op.pop = *pop;
    op.pop.member += q0 / 64;
  }
  return op;
}

// kernel right-hand sides: the operator's (RHS 0) and a permuted vector (RHS 2)
pfr::RhsArgs rhs_operator(const pfr::ChunkOp& op) {
  return {.rhsP = op.rhsP, .beta_re = op.beta_re, .beta_im = op.beta_im, .mass_sum = op.mass_sum, .freqs = op.freqs};
}
pfr::RhsArgs rhs_vector(const double2* G) { return {.G = G}; }

// pruning (pfr_set_prune): the operator-form sweeps walk the loaded trees' view; the refinement modes keep the full
// one (their corrections solve right-hand sides that are not the operator's)
bool sweeps_pruned(const pfr_solver* s, int mode) {
  return s->act && !(mode & (PFR_CHECK_REFINE | PFR_CHECK_REFINE_ADJ));
}
bool sweeps_pruned(const pfr_solver* s) { return sweeps_pruned(s, s->check_mode); }

// bytes of a host table to the device on stream st (stage slot `slot`); *dev: the device copy
int stage_upload(pfr_solver* s, int slot, const void* src, size_t bytes, void** dev, hipStream_t st) {
  auto& g = s->stage[slot];
  if (g.busy) HIP_TRY(hipEventSynchronize(g.ev));   // the previous copy out of the staging block
  g.busy = false;
  if (bytes > g.cap) {
    HIP_TRY(hipStreamSynchronize(st));              // the kernels reading the old device copy
    if (g.host) (void)hipHostFree(g.host);
    if (g.dev) (void)hipFree(g.dev);
    g.host = g.dev = nullptr;
    g.cap = 0;
    const size_t cap = std::max<size_t>(4096, 2 * bytes);
    HIP_TRY(hipHostMalloc(&g.host, cap));
    HIP_TRY(hipMalloc(&g.dev, cap));
    g.cap = cap;
  }
  if (!g.ev) HIP_TRY(hipEventCreateWithFlags(&g.ev, hipEventDisableTiming));
  std::memcpy(g.host, src, bytes);
  HIP_TRY(hipMemcpyAsync(g.dev, g.host, bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(g.ev, st));
  g.busy = true;
  *dev = g.dev;
  return PFR_OK;
}

// v (here and below): the view whose fronts the pass walks -- *s for every front
int factor_all(pfr_solver* s, const SolverView& v, const pfr::ChunkOp& op, pfr::Mat mode, const double2* data,
               int64_t ds, int nvalid, hipStream_t st) {
  const int L = (int)s->level_ptr.size() - 1;
  const int ngroups = (int)(s->Fc / 64);
  const bool kt = (s->timing & 2) && s->n_tev < (int)s->tev.size() && !s->tev[s->n_tev].kev.empty();
  hipEvent_t* kev = kt ? s->tev[s->n_tev].kev.data() : nullptr;
  auto mark = [&](int l, int c) {
    if (kt) (void)hipEventRecord(kev[(pfr::NKC + 1) * l + c], st);
  };
  if (kt) s->tev[s->n_tev].f0 = false;
  for (int l = 0; l < L; ++l) {
    const pfr::FactorLevel& r = v.sched.factor[l];
    const int32_t* lvl = v.d_level_fronts + v.level_ptr[l];
    mark(l, 0);
    if (r.fused0 && mode == pfr::MAT_OPERATOR) {
      if (kt) s->tev[s->n_tev].f0 = true;
      // the bottom level's leaf fronts in one pass (k_front0): A11, L21 and update block per frequency in registers
      pfr::launch_front0(s->P, v.d_f0_front, r, v.d_f0_ptr, v.d_f0_nz, ngroups, s->F, s->Fc, op, s->flags, st);
      for (int c = 1; c <= 5; ++c) mark(l, c);
      continue;
    }
    pfr::launch_assemble(mode, v.d_asm + v.asm_ptr[l], r.nasm, v.d_asm_xp + v.asm_ptr[l] / 8, v.d_asm_x, ngroups,
                         s->F, s->Fc, op, data, ds, nvalid, st);
    mark(l, 1);
    if (r.lds)
      pfr::launch_factor_lds(s->P, lvl, r, s->F, s->Fc, s->flags, st);
    else
      pfr::launch_factor(s->sym, s->P, lvl, r, ngroups, s->F, s->Fc, s->flags, st);
    mark(l, 2);
    pfr::launch_offdiag(mode, s->P, v.d_items + v.item_ptr[l], r, v.d_orec, v.d_oxp + v.item_ptr[l], v.d_ox,
                        ngroups, s->F, s->Fc, op, data, ds, nvalid, st);
    mark(l, 3);
    pfr::launch_schur_blk(s->P, v.d_blocks + v.blk_ptr[l], r.nblocks,
                          v.d_bg1 + (int64_t)v.blk_ptr[l] * 16 * 16, v.d_bgxp + v.blk_ptr[l], v.d_bgx, ngroups, s->F,
                          s->Fc, st);
    mark(l, 4);
    pfr::launch_schur(s->sym, s->P, v.d_tiles + v.tile_ptr[l], r.ntiles,
                      v.d_g1 + (int64_t)v.tile_ptr[l] * pfr::SCHUR_TM * pfr::SCHUR_TN * pfr::SCHUR_SR * pfr::SCHUR_SC,
                      v.d_gxp + v.tile_ptr[l], v.d_gx, ngroups, s->F, s->Fc, st);
    mark(l, 5);
  }
  LAUNCH_TRY();
  return PFR_OK;
}

// one triangular pass (pfr::Tri): bottom-up for L and U^T, top-down for U and L^T
// subset (the rhs reach, the support's, or every front): bottom-up passes visit only the reached
// fronts; top-down passes treat the pivot values of unreached fronts as zero
int solve_all(pfr_solver* s, const SolverView& v, const pfr::ChunkOp& op, pfr::Tri which, pfr::Rhs rhs_mode,
              const pfr::RhsArgs& rd, const double2* Yin, double2* Out, hipStream_t st, pfr::Reach subset = pfr::REACH_ALL,
              const int* glist = nullptr) {
  const int L = (int)s->level_ptr.size() - 1;
  const int ngroups = glist ? pfr::REFINE_CAP : (int)(s->Fc / 64);
  const bool up = (which == pfr::TRI_L || which == pfr::TRI_UT);
  const int* reach = subset >= 0 ? v.d_reach[subset] : nullptr;
  for (int t = 0; t < L; ++t) {
    int l = up ? t : L - 1 - t;
    // bottom-up over the subset's fronts only, top-down over the whole level
    const bool part = up && subset >= 0;
    const int32_t* lvl = part ? v.d_reach_fronts[subset] + v.reach_ptr[subset][l] : v.d_level_fronts + v.level_ptr[l];
    const pfr::SolveLevel& r = v.sched.solve[part ? pfr::SUBSET_REACH0 + subset : pfr::SUBSET_ALL][l];
    pfr::launch_solve(which, rhs_mode, s->sym, s->P, lvl, r, ngroups, s->F, s->Fc, s->WV, rd, op.pop, Yin, Out, reach, st,
                      glist);
  }
  LAUNCH_TRY();
  return PFR_OK;
}

pfr::DirArgs dir_desc(const pfr_solver* s, const pfr::ChunkOp& op) {
  return {.dir = s->d_dir, .crow = s->d_crow, .cptr = s->d_cptr_dir, .ce = s->d_ce, .dptr = s->d_dptr, .de = s->d_de,
          .K = op.K, .M = op.M, .freqs = op.freqs};
}
// the adjoint's Dirichlet rows (k_dirichlet_post) over the nodes on the view's fronts
pfr::DirArgs post_desc(const pfr_solver* s, const SolverView& v, const pfr::ChunkOp& op) {
  pfr::DirArgs d = dir_desc(s, op);
  d.dir = v.post_dir;
  d.dptr = v.post_dptr;
  d.de = v.post_de;
  return d;
}

// A x = b on the chunk's factors, x -> Out (permuted).  RHS_OPERATOR: operator right-hand side
// (rd.rhsP ...); RHS_VECTOR: vector rd.G (overwritten in symmetric mode).  Symmetric mode: Dirichlet
// columns moved to the right-hand side first, then L and U = diag(U) L^T.
int forward_solve(pfr_solver* s, const SolverView& v, const pfr::ChunkOp& op, pfr::Rhs rhs_mode, pfr::RhsArgs rd,
                  double2* Out, hipStream_t st, pfr::Reach subset = pfr::REACH_ALL) {
  int rc;
  if (s->sym) {
    const pfr::DirArgs dd = dir_desc(s, op);
    if (rhs_mode == pfr::RHS_OPERATOR) {
      pfr::launch_dirichlet_rhs(pfr::RHS_OPERATOR, dd, op.pop, s->n_crow, rd, nullptr, s->Bc, s->Fc, st);
      rd.cslot = s->d_cslot;
      rd.Bc = s->Bc;
      if (s->n_crow > 0) rhs_mode = pfr::RHS_OPERATOR_DIR;
    } else {
      pfr::launch_dirichlet_rhs(pfr::RHS_VECTOR, dd, op.pop, s->n_crow, rd, const_cast<double2*>(rd.G), nullptr, s->Fc, st);
    }
  }
  if ((rc = solve_all(s, v, op, pfr::TRI_L, rhs_mode, rd, nullptr, s->Y, st, subset))) return rc;
  return solve_all(s, v, op, pfr::TRI_U, pfr::RHS_OPERATOR, rd, s->Y, Out, st, subset);
}

// A^T l = g (g = rg.G, permuted), l -> Out.  Symmetric mode: the decoupled matrix is symmetric,
// so L and U = diag(U) L^T again, then the Dirichlet rows of l are corrected.
int adjoint_solve(pfr_solver* s, const SolverView& v, const pfr::ChunkOp& op, const pfr::RhsArgs& rg, double2* Out,
                  hipStream_t st, pfr::Reach subset = pfr::REACH_ALL, const int* glist = nullptr) {
  int rc;
  if (s->sym) {
    if ((rc = solve_all(s, v, op, pfr::TRI_L, pfr::RHS_VECTOR, rg, nullptr, s->Y, st, subset, glist)) ||
        (rc = solve_all(s, v, op, pfr::TRI_U, pfr::RHS_OPERATOR, rg, s->Y, Out, st, subset, glist)))
      return rc;
    pfr::launch_dirichlet_post(post_desc(s, v, op), op.pop, v.post_n, Out, s->Fc, st, glist);
    return PFR_OK;
  }
  if ((rc = solve_all(s, v, op, pfr::TRI_UT, pfr::RHS_VECTOR, rg, nullptr, s->Y, st, subset))) return rc;
  return solve_all(s, v, op, pfr::TRI_LT, pfr::RHS_OPERATOR, rg, s->Y, Out, st, subset);
}

// Row lists and buffers of the functional-from-bottom-up path (allocated on first use, lists rebuilt
// whenever a reach changed)
int fn_setup(pfr_solver* s, SolverView& v) {
  int rc;
  const int64_t n = s->n;
  if (!s->WVk) {
    if ((rc = s->alloc(&s->WVk, s->ws.WVk)) || (rc = s->alloc(&s->YVk, s->ws.YVk)) ||
        (rc = s->alloc(&s->fn_parts, s->ws.fn_parts)) || (rc = s->alloc(&s->fcoef, s->ws.fcoef)) ||
        (rc = s->up(&s->d_noslot, std::vector<int32_t>(n, -1))) || (rc = s->alloc(&s->d_aP, 3 * n)))
      return rc;
    HIP_TRY(hipMemcpy(s->d_aP, s->a_perm.data(), s->a_perm.size() * 8, hipMemcpyHostToDevice));
  }
  if (!v.d_fn_rows) {
    if ((rc = s->alloc(&v.d_fn_rows, n)) || (rc = s->alloc(&v.d_sup_rows, n))) return rc;
    if (&v != s) v.mine.insert(v.mine.end(), {(void*)v.d_fn_rows, (void*)v.d_sup_rows});
  }
  if (v.fn_ready) return PFR_OK;
  std::vector<int2> both;
  std::vector<int32_t> sup;
  // a view keeps the full list's slots (k_fn_dot assigns a slot to a partial and a wave by its position, and the
  // partials must add the same terms in the same order); the rows it does not reach become skip entries (-1)
  for (size_t t = 0; t < s->front_ns.size(); ++t) {
    if (!s->reach_host[1][t]) continue;
    for (int a = 0; a < s->front_ns[t]; ++a) {
      const int32_t row = s->front_col0[t] + a;
      if (v.reach_host[1][t]) sup.push_back(row);
      if (s->reach_host[0][t])
        both.push_back(v.reach_host[1][t] && v.reach_host[0][t]
                           ? make_int2(row, s->front_off[t] + a * s->front_f[t] + a)
                           : make_int2(-1, -1));
    }
  }
  v.n_fn_rows = (int)both.size();
  v.n_sup_rows = (int)sup.size();
  // at most n rows each (pivot rows are distinct): into the buffers allocated for n
  if (!both.empty()) HIP_TRY(hipMemcpy(v.d_fn_rows, both.data(), both.size() * sizeof(int2), hipMemcpyHostToDevice));
  if (!sup.empty()) HIP_TRY(hipMemcpy(v.d_sup_rows, sup.data(), sup.size() * 4, hipMemcpyHostToDevice));
  v.fn_ready = true;
  return PFR_OK;
}

// forward bottom-up over the rhs reach (slice 0) and L w_k = a_k over the support reach (slices 1-3),
// one launch chain
int fn_bottom_up(pfr_solver* s, const SolverView& v, const pfr::ChunkOp& op, pfr::Rhs rhs_mode, const pfr::RhsArgs& rf,
                 hipStream_t st) {
  const int L = (int)s->level_ptr.size() - 1;
  const int ngroups = (int)(s->Fc / 64);
  int64_t total_rows = 0;
  for (size_t t = 0; t < s->front_f.size(); ++t) total_rows += s->front_f[t];
  pfr::RhsArgs rd[4] = {rf, rf, rf, rf};
  double2* WV[4] = {s->WV, s->WVk, s->WVk + total_rows * s->Fc, s->WVk + 2 * total_rows * s->Fc};
  double2* Y[4] = {s->Y, s->Y2, s->YVk, s->YVk + (int64_t)s->n * s->Fc};
  const int* reach[4] = {v.d_reach[0], v.d_reach[1], v.d_reach[1], v.d_reach[1]};
  for (int k = 1; k < 4; ++k) {
    rd[k].rhsP = s->d_aP + (int64_t)(k - 1) * s->n;
    rd[k].mass_sum = 0.0;
    rd[k].beta_re = 1.0;
    rd[k].beta_im = 0.0;
    rd[k].cslot = s->d_noslot;
  }
  for (int l = 0; l < L; ++l) {
    const int32_t* sup = v.d_reach_fronts[1] + v.reach_ptr[1][l];
    const int* lvl[4] = {v.d_reach_fronts[0] + v.reach_ptr[0][l], sup, sup, sup};
    pfr::launch_lsolve_multi(rhs_mode, s->P, 4, lvl, v.sched.chain[l], ngroups, s->F, s->Fc, WV, rd, op.pop, Y, reach, st);
  }
  LAUNCH_TRY();
  return PFR_OK;
}

// Symmetric mode, loss + gradient: the forward top-down pass first over the fronts the loss
// support reaches only (they hold every support row), then -- once the loss cotangent is known
// and its bottom-up pass (same fronts) done -- ONE top-down pass computes the adjoint on every
// front and the forward solution on the rest, each factor value loaded once for both.
int sym_top_down_support(pfr_solver* s, const SolverView& v, hipStream_t st) {
  const int L = (int)s->level_ptr.size() - 1;
  const int ngroups = (int)(s->Fc / 64);
  for (int l = L - 1; l >= 0; --l) {
    pfr::launch_solve(pfr::TRI_U, pfr::RHS_OPERATOR, true, s->P, v.d_reach_fronts[1] + v.reach_ptr[1][l],
                      v.sched.solve[pfr::SUBSET_REACH1][l], ngroups, s->F, s->Fc, s->WV, pfr::RhsArgs(), pfr::PopArgs(), s->Y,
                      s->X, v.d_reach[0], st);
  }
  LAUNCH_TRY();
  return PFR_OK;
}

int sym_top_down_pair(pfr_solver* s, const SolverView& v, hipStream_t st, bool fwd_all = false) {
  const int L = (int)s->level_ptr.size() - 1;
  const int ngroups = (int)(s->Fc / 64);
  for (int l = L - 1; l >= 0; --l) {
    pfr::launch_usolve2(s->P, v.d_level_fronts + v.level_ptr[l], v.sched.pair[l], ngroups, s->F, s->Fc, s->Y, s->X,
                        v.d_reach[0], fwd_all ? nullptr : v.d_reach[1], s->Y2, s->XA, v.d_reach[1], st);
  }
  LAUNCH_TRY();
  return PFR_OK;
}

// Mark the fronts holding the given permuted rows and all their ancestors; upload the flags and
// the marked fronts level by level (level_fronts order kept).
// (a view other than the solver itself takes the rows on its own fronts only)
int set_reach(pfr_solver* s, SolverView& v, int which, const std::vector<int32_t>& prows) {
  std::vector<int32_t> mark, list;
  pfr::reach_lists(s->front_of_col, s->front_parent, v.level_ptr, v.level_fronts_host, prows, mark, list,
                   v.reach_ptr[which]);
  v.reach_host[which].assign(mark.begin(), mark.end());
  v.fn_ready = false;
  if (&v == s && s->act) s->act->fn_ready = false;
  // a view decides its launch shapes for the full reaches (set before the view's): plan.hpp, level_schedule
  pfr::schedule_reach(v.sched, v.reach_ptr, &v != s ? &s->reach_ptr : nullptr);
  HIP_TRY(hipMemcpy(v.d_reach[which], mark.data(), mark.size() * 4, hipMemcpyHostToDevice));
  if (!list.empty()) HIP_TRY(hipMemcpy(v.d_reach_fronts[which], list.data(), list.size() * 4, hipMemcpyHostToDevice));
  return PFR_OK;
}

// a residual walk (launch.hpp): a checked one finishes into the chunk's flags and the caller's berr slots, the correction's
// dot products go to s->cpart, the fused contraction to s->kpart (a walk into R has neither: no maxima, no flags)
void run_walk(pfr_solver* s, const SolverView& v, const pfr::ChunkOp& op, const Walk& w, int nvalid, hipStream_t st) {
  const bool fwd = w.sys == Walk::FORWARD;
  // w.contract: the gradient contraction fused into the forward walk -- stiffness values nz-major, kpart out; over
  // the view's live matrices where their compact table was built (update_live), else over all n_stiff
  const bool compact = w.contract && v.d_se_live;
  const unsigned all = w.contract ? (1u << s->n_stiff) - 1u : 0u;
  const pfr::ResidArgs d{.ptr = fwd ? s->d_rptr : s->d_cptr, .idx = fwd ? s->d_ridx : s->d_cidx,
                         .nzs = fwd ? s->d_rnz : s->d_cnz, .n = s->n, .K = op.K, .M = op.M, .freqs = op.freqs,
                         .data = w.data, .data_stride = w.ds, .nvalid = nvalid, .rhsP = w.rd.rhsP,
                         .beta_re = w.rd.beta_re, .beta_im = w.rd.beta_im, .mass_sum = w.rd.mass_sum, .B = w.rd.B,
                         .b_stride = w.rd.b_stride, .perm = s->P.perm, .G = w.rd.G, .walk = v.d_walk,
                         .se = compact ? v.d_se_live : w.contract ? s->stiff : nullptr,
                         .kpart = w.contract ? s->kpart : nullptr, .live = compact ? v.live : all,
                         .nslot = w.contract ? s->n_stiff : 0, .glist = w.glist};
  const int n_stiff = w.contract ? s->n_stiff : 0;
  pfr::launch_residual(w.mat, w.rhs, d, n_stiff, w.contract ? s->live_unroll : s->res_unroll, op.pop, w.X, s->Fc, w.R,
                       w.check ? s->d_berr_acc : nullptr, st, w.Mu, w.Mu ? s->cpart : nullptr);
  if (!w.check) return;
  pfr::launch_berr_finish(s->d_berr_acc, s->Fc, nvalid, s->check_tol,
                          fwd ? PFR_FLAG_BACKWARD_ERROR : PFR_FLAG_BACKWARD_ERROR_ADJ, s->flags,
                          w.q0 >= 0 ? s->berr_out : nullptr, w.q0, w.sys, st);
}

// s_{q,k} partials of sum_nz S_k(nz) lam[row] x[col] over the union pattern's distinct entries
// (k_contract_eg, the loss sweep's contraction; no checks)
void contract_rows(pfr_solver* s, const double2* lam, const double2* x, int nv, hipStream_t st) {
  pfr::launch_contract_eg(s->d_uent, s->n_uent, s->d_se, s->n_stiff, lam, x, s->Fc, nv, s->partial, st);
}

// The device side of a view: the plan's level lists and factor-class records, the walk list (rows of other fronts
// -1), the reach arrays, and the schedule with no front reached yet.  v == *s: the solver's own (full) view.
int upload_view(pfr_solver* s, SolverView& v, const Symbolic& S, const pfr::Plan& pl, const pfr::Knobs& knobs) {
  int rc;
  const size_t own0 = s->owned.size();
  const int nf = (int)S.fronts.size();
  v.active = pl.active;
  v.level_ptr = pl.level_ptr;
  v.level_fronts_host = pl.level_fronts;
  v.tile_ptr = pl.tile_ptr;
  v.blk_ptr = pl.blk_ptr;
  v.asm_ptr = pl.asm_ptr;
  v.item_ptr = pl.item_ptr;
  v.lev_bytes = pl.lev_bytes;
  for (auto& r : v.reach_ptr) r.clear();
  v.sched = pfr::level_schedule(S, pl, s->Fc, knobs, v.reach_ptr);
  const pfr::I2 z2{0, 0}, n2{-1, -1};
  const pfr::I4 z4{0, 0, 0, 0}, n4{-1, -1, -1, -1};
  std::vector<int32_t> walk(S.iperm);
  for (int32_t& p : walk)
    if (!pl.active[s->front_of_col[p]]) p = -1;
  if ((rc = s->up_rec(&v.d_level_fronts, pl.level_fronts, 0)) || (rc = s->up(&v.d_walk, walk)) ||
      (rc = s->up_rec(&v.d_tiles, pl.tiles, z4)) || (rc = s->up_rec(&v.d_g1, pl.g1, -1)) || (rc = s->up(&v.d_gxp, pl.gxp)) ||
      (rc = s->up_rec(&v.d_gx, pl.gx, z2)) || (rc = s->up_rec(&v.d_blocks, pl.blocks, z4)) ||
      (rc = s->up_rec(&v.d_bg1, pl.bg1, -1)) || (rc = s->up(&v.d_bgxp, pl.bgxp)) || (rc = s->up_rec(&v.d_bgx, pl.bgx, z2)) ||
      (rc = s->up_rec(&v.d_asm, pl.asm_rec, n4)) || (rc = s->up(&v.d_asm_xp, pl.asm_xp)) ||
      (rc = s->up_rec(&v.d_asm_x, pl.asm_x, z2)) || (rc = s->up_rec(&v.d_items, pl.items, z4)) ||
      (rc = s->up_rec(&v.d_orec, pl.orec, n2)) || (rc = s->up(&v.d_oxp, pl.oxp)) || (rc = s->up_rec(&v.d_ox, pl.ox, z2)))
    return rc;
  if (v.sched.factor[0].fused0 && ((rc = s->up(&v.d_f0_front, pl.f0_front)) || (rc = s->up(&v.d_f0_ptr, pl.f0_ptr)) ||
                                   (rc = s->up(&v.d_f0_nz, pl.f0_nz))))
    return rc;
  for (int w = 0; w < 2; ++w) {
    if ((rc = s->alloc(&v.d_reach[w], nf)) || (rc = s->alloc(&v.d_reach_fronts[w], nf))) return rc;
    if ((rc = set_reach(s, v, w, {}))) return rc;
  }
  if (&v != s) v.mine.assign(s->owned.begin() + own0, s->owned.end());
  return PFR_OK;
}

void release_view(pfr_solver* s, SolverView*& v) {
  if (!v) return;
  (void)hipDeviceSynchronize();   // launches that read the view's arrays
  for (void* p : v->mine) {
    s->owned.erase(std::remove(s->owned.begin(), s->owned.end(), p), s->owned.end());
    (void)hipFree(p);
  }
  delete v;
  v = nullptr;
}

// The live stiffness matrices of a view's walk (plan.hpp, live_stiffness: decided by value from the registered
// table, once per view and pfr_set_stiffness) and, where they are 6 or 12 of more, the table compacted to them for
// the walk's contraction (PFR_CONTRACT_LIVE=0, any other count, or a solver that keeps no analysis: all n_stiff)
int update_live(pfr_solver* s, SolverView& v) {
  if (v.d_se_live) {
    (void)hipDeviceSynchronize();   // launches that read the table
    s->owned.erase(std::remove(s->owned.begin(), s->owned.end(), (void*)v.d_se_live), s->owned.end());
    v.mine.erase(std::remove(v.mine.begin(), v.mine.end(), (void*)v.d_se_live), v.mine.end());
    (void)hipFree(v.d_se_live);
    v.d_se_live = nullptr;
  }
  v.live = s->n_stiff ? (1u << s->n_stiff) - 1u : 0u;
  v.n_live = s->n_stiff;
  if (!s->stiff || !s->sym || s->stiff_bits.empty()) return PFR_OK;
  v.live = pfr::live_stiffness(s->S, &v == s ? nullptr : &v.active, s->stiff_bits);
  v.n_live = __builtin_popcount(v.live);
  if (!s->contract_live || v.n_live >= s->n_stiff || (v.n_live != 6 && v.n_live != 12)) return PFR_OK;
  int rc;
  if (!s->d_live_bad && (rc = s->alloc(&s->d_live_bad, 1))) return rc;
  if ((rc = s->alloc(&v.d_se_live, s->nnz * v.n_live))) return rc;
  if (&v != s) v.mine.push_back(v.d_se_live);
  HIP_TRY(hipMemsetAsync(s->d_live_bad, 0, 4, nullptr));
  HIP_TRY(hipMemsetAsync(v.d_se_live, 0, (size_t)s->nnz * v.n_live * 8, nullptr));
  pfr::launch_gather_live(v.d_walk, s->n, s->d_rptr, s->d_rnz, s->stiff, s->n_stiff, v.live, v.n_live, v.d_se_live,
                          s->d_live_bad, nullptr);
  int32_t bad = 0;
  HIP_TRY(hipMemcpy(&bad, s->d_live_bad, 4, hipMemcpyDeviceToHost));
  if (bad) return fail(PFR_ERR_STATE, "a stiffness matrix outside the live list is non-zero on a visited entry");
  return PFR_OK;
}

// The inertia contraction's entry list of a view's walk (plan.hpp, mass_entries: decided by value from the registered
// components, once per view and pfr_set_inertia)
int update_mass(pfr_solver* s, SolverView& v) {
  if (v.d_mptr) (void)hipDeviceSynchronize();   // launches that read the list
  for (int32_t** p : {&v.d_mlist, &v.d_mptr}) {
    if (!*p) continue;
    s->owned.erase(std::remove(s->owned.begin(), s->owned.end(), (void*)*p), s->owned.end());
    v.mine.erase(std::remove(v.mine.begin(), v.mine.end(), (void*)*p), v.mine.end());
    (void)hipFree(*p);
    *p = nullptr;
  }
  v.n_mlist = v.len_mlist = 0;
  if (!s->mass) return PFR_OK;
  std::vector<char> rows;
  if (&v != s) rows = pfr::front_rows(s->S, v.active);
  const pfr::MassList L = pfr::mass_entries(s->h_uent, s->n_uent, s->n, &v != s ? &rows : nullptr, s->mass_nz);
  v.n_mlist = L.n_list;
  v.len_mlist = (int)L.list.size();
  int rc;
  if ((rc = s->up_rec(&v.d_mlist, L.list, (int32_t)-1)) || (rc = s->up(&v.d_mptr, L.ptr))) return rc;
  if (&v != s) v.mine.insert(v.mine.end(), {(void*)v.d_mlist, (void*)v.d_mptr});
  return PFR_OK;
}

// A view of the fronts in `mask` (whole trees): its plan and schedule, the Dirichlet nodes on its fronts, and the
// solver's current reaches restricted to it (keep0 = false: no forward reach -- the complement carries no load)
int make_view(pfr_solver* s, const std::vector<char>& mask, bool keep0, SolverView** out) {
  pfr::Plan pl;
  std::string perr;
  if (pfr::build_plan(s->S, s->sched.knobs.blk_min, pl, perr, &mask)) return fail(PFR_ERR_ARG, perr);
  auto* v = new SolverView();
  int rc = upload_view(s, *v, s->S, pl, s->sched.knobs);
  std::vector<pfr::I2> dir, de;
  std::vector<int32_t> dptr(1, 0);
  for (size_t d = 0; d < s->h_dir.size() && rc == PFR_OK; ++d) {
    if (!mask[s->front_of_col[s->h_dir[d].x]]) continue;
    dir.push_back(s->h_dir[d]);
    de.insert(de.end(), s->h_de.begin() + s->h_dptr[d], s->h_de.begin() + s->h_dptr[d + 1]);
    dptr.push_back((int32_t)de.size());
  }
  const size_t own0 = s->owned.size();
  v->post_n = (int)dir.size();
  if (rc == PFR_OK)
    (void)((rc = s->up_rec(&v->post_dir, dir, pfr::I2{0, 0})) || (rc = s->up(&v->post_dptr, dptr)) ||
           (rc = s->up_rec(&v->post_de, de, pfr::I2{0, 0})));
  v->mine.insert(v->mine.end(), s->owned.begin() + own0, s->owned.end());
  for (int w = keep0 ? 0 : 1; w < 2 && rc == PFR_OK; ++w) rc = set_reach(s, *v, w, pfr::rows_in(s->S, mask, s->reach_rows[w]));
  if (rc != PFR_OK) {
    release_view(s, v);
    return rc;
  }
  *out = v;
  return PFR_OK;
}

// The loaded trees' view for the solver's right-hand side vector (pfr_set_prune, pfr_set_rhs): built when pruning
// is on and some tree carries no load, kept while the set of loaded trees stays the same
int update_prune(pfr_solver* s) {
  std::vector<char> mask;
  bool any_off = false;
  if (s->prune && s->sym && s->has_rhs) {
    std::vector<double> rp(s->n);
    for (int p = 0; p < s->n; ++p) rp[p] = s->rhs_host[s->perm[p]];
    mask = pfr::loaded_fronts(s->S, rp.data());
    for (char m : mask) any_off = any_off || !m;
  }
  if (s->act && any_off && s->act->active == mask) return PFR_OK;
  ++s->gen;
  release_view(s, s->act);
  release_view(s, s->comp);
  s->unl_rows.clear();
  s->comp_done = false;
  if (!any_off) return PFR_OK;
  for (size_t t = 0; t < mask.size(); ++t) {
    if (mask[t]) continue;
    const int32_t a = s->front_col0[t], b = a + s->front_ns[t];
    s->unl_rows.emplace_back(a, b);
  }
  std::sort(s->unl_rows.begin(), s->unl_rows.end());
  size_t k = 0;
  for (size_t i = 1; i < s->unl_rows.size(); ++i) {
    if (s->unl_rows[i].first == s->unl_rows[k].second)
      s->unl_rows[k].second = s->unl_rows[i].second;
    else
      s->unl_rows[++k] = s->unl_rows[i];
  }
  if (!s->unl_rows.empty()) s->unl_rows.resize(k + 1);
  s->unl_dirty = true;   // the rows of the unloaded trees in X / XA: exact zeros from the first pruned sweep on
  if (int rc = make_view(s, mask, true, &s->act)) return rc;
  if (int rc = update_live(s, *s->act)) return rc;
  return update_mass(s, *s->act);
}

}  // namespace

extern "C" {

const char* pfr_version(void) { return "pfr 0.1.0 (gfx950, frequency-minor multifrontal)"; }
const char* pfr_last_error(void) { return g_last_error.c_str(); }

void pfr_symbolic_options_default(pfr_symbolic_options* o) {
  pfr::SymbolicOptions d;
  o->leaf_size = d.leaf_size;
  o->ordering = d.ordering;
  o->relax_small = d.relax_small;
  o->relax_mid = d.relax_mid;
  o->relax_big = d.relax_big;
  o->zrelax_mid = d.zrelax_mid;
  o->zrelax_big = d.zrelax_big;
  o->symmetric = d.symmetric;
  o->n_last = 0;
  o->last = nullptr;
  o->max_ns = d.max_ns;
  o->md_delta = d.md_delta;
}

int pfr_symbolic_create(int32_t n, int64_t nnz, const int32_t* colptr, const int32_t* rowind,
                        const pfr_symbolic_options* opt, pfr_symbolic** out) {
  if (!out || !colptr || (nnz > 0 && !rowind) || n <= 0 || nnz < 0) return fail(PFR_ERR_ARG, "bad arguments");
  if (nnz > INT32_MAX) return fail(PFR_ERR_ARG, "nnz exceeds int32 (cf. Problem.py:311 TODO)");
  pfr::SymbolicOptions o;
  if (opt) {
    o.leaf_size = opt->leaf_size;
    o.ordering = opt->ordering;
    o.relax_small = opt->relax_small;
    o.relax_mid = opt->relax_mid;
    o.relax_big = opt->relax_big;
    o.zrelax_mid = opt->zrelax_mid;
    o.zrelax_big = opt->zrelax_big;
    o.symmetric = opt->symmetric;
    o.max_ns = opt->max_ns;
    o.md_delta = opt->md_delta;
    if (opt->n_last > 0) {
      if (!opt->last) return fail(PFR_ERR_ARG, "n_last > 0 without last nodes");
      o.last.assign(opt->last, opt->last + opt->n_last);
    }
  }
  auto* sym = new pfr_symbolic();
  if (pfr::analyse(n, nnz, colptr, rowind, o, sym->S) != 0) {
    std::string msg = "symbolic analysis failed: " + sym->S.error;
    delete sym;
    return fail(PFR_ERR_SYMBOLIC, msg);
  }
  *out = sym;
  return PFR_OK;
}

int pfr_symbolic_stats_get(const pfr_symbolic* sym, pfr_symbolic_stats* o) {
  if (!sym || !o) return fail(PFR_ERR_ARG, "null argument");
  const Symbolic& S = sym->S;
  o->n = S.n;
  o->nnz = S.nnz;
  o->n_fronts = (int32_t)S.fronts.size();
  o->n_levels = (int32_t)S.level_ptr.size() - 1;
  o->max_front = S.max_front;
  o->total_rows = S.total_rows;
  o->factor_entries = S.factor_entries;
  o->nnz_lu = S.nnz_lu;
  o->factor_flops = S.factor_flops;
  o->symmetric = S.symmetric;
  o->n_dirichlet = (int32_t)S.dir_p.size();
  o->n_coupling = (int64_t)S.cpl_p.size();
  return PFR_OK;
}

int pfr_symbolic_export(const pfr_symbolic* sym, int32_t what, void* dst, int64_t cap) {
  if (!sym || !dst) return fail(PFR_ERR_ARG, "null argument");
  const Symbolic& S = sym->S;
  const void* src = nullptr;
  int64_t bytes = 0;
  std::vector<int64_t> fr;
  std::vector<int32_t> tmp;
  auto pick = [&](const std::vector<int32_t>& v) {
    src = v.data();
    bytes = (int64_t)v.size() * 4;
  };
  switch (what) {
    case PFR_EXPORT_PERM: pick(S.perm); break;
    case PFR_EXPORT_IPERM: pick(S.iperm); break;
    case PFR_EXPORT_FRONTS:
      for (const Front& f : S.fronts) {
        int64_t v[8] = {f.ns, f.f, f.row0, f.col0, f.parent, f.level, f.off, f.wv};
        fr.insert(fr.end(), v, v + 8);
      }
      src = fr.data();
      bytes = (int64_t)fr.size() * 8;
      break;
    case PFR_EXPORT_IDX: pick(S.idx); break;
    case PFR_EXPORT_RELPOS: pick(S.relpos); break;
    case PFR_EXPORT_ASM_PTR: pick(S.asm_ptr); break;
    case PFR_EXPORT_ASM_COL: pick(S.asm_col); break;
    case PFR_EXPORT_ASM_NZ: pick(S.asm_nz); break;
    case PFR_EXPORT_EA_PTR: pick(S.ea_ptr); break;
    case PFR_EXPORT_EA_SRC: pick(S.ea_src); break;
    case PFR_EXPORT_LEVEL_PTR: pick(S.level_ptr); break;
    case PFR_EXPORT_LEVEL_FRONTS: pick(S.level_fronts); break;
    case PFR_EXPORT_DIRICHLET:
      for (size_t d = 0; d < S.dir_p.size(); ++d) tmp.insert(tmp.end(), {S.dir_p[d], S.dir_nz[d]});
      pick(tmp);
      break;
    case PFR_EXPORT_COUPLING:
      for (size_t c = 0; c < S.cpl_p.size(); ++c) tmp.insert(tmp.end(), {S.cpl_p[c], S.cpl_dir[c], S.cpl_nz[c]});
      pick(tmp);
      break;
    default: return fail(PFR_ERR_ARG, "unknown export id");
  }
  if (bytes > cap) return fail(PFR_ERR_ARG, "destination too small");
  if (bytes) std::memcpy(dst, src, bytes);
  return PFR_OK;
}

void pfr_symbolic_destroy(pfr_symbolic* sym) { delete sym; }

int64_t pfr_solver_workspace_bytes(const pfr_symbolic* sym, int32_t max_batch) {
  if (!sym || max_batch <= 0) return -1;
  return workspace_bytes(sym->S, round64(max_batch));
}

int pfr_solver_create(const pfr_symbolic* sym, const int32_t* colptr, const int32_t* rowind, int32_t device,
                      int32_t max_batch, pfr_solver** out) {
  if (!sym || !out || max_batch <= 0 || !colptr || !rowind) return fail(PFR_ERR_ARG, "bad arguments");
  HIP_TRY(hipSetDevice(device));
  const Symbolic& S = sym->S;
  auto* s = new pfr_solver();
  auto bail = [&](int rc) {
    delete s;
    return rc;
  };
  s->device = device;
  auto knob = [](const char* name, int def, int lo, int hi) {
    const char* e = getenv(name);
    return e ? std::max(lo, std::min(hi, atoi(e))) : def;
  };
  // path knobs: the functional from the bottom-up passes, the contraction in the forward walk, the cotangent's
  // solve-error scale, the check walk's gather batch, sweep graphs (the launch-shape knobs: pfr::knobs_from_env)
  s->res_unroll = knob("PFR_RES_UNROLL", 8, 4, 8) == 8 ? 8 : 4;
  s->fn_dot = knob("PFR_FN_DOT", 1, 0, 1);
  s->contract_walk = knob("PFR_CONTRACT_WALK", 1, 0, 1);
  s->contract_live = knob("PFR_CONTRACT_LIVE", 1, 0, 1);
  s->live_unroll = knob("PFR_LIVE_UNROLL", 8, 4, 8) == 8 ? 8 : 4;
  s->scale_corr = knob("PFR_SCALE_CORR", 1, 0, 1);
  // PFR_GRAPH=1: repeated sweeps captured into and replayed from a hipGraph (off by default: bitwise the same
  // results and the host's enqueue of a 512-frequency sweep 427 -> 75 us, but 512 frequencies within the spread
  // and 4,096 frequencies 1 % slower on the device, 67.0-67.6k -> 66.5-66.8k, gpurun_out/r6r_e4096)
  s->graph_mode = knob("PFR_GRAPH", 0, 0, 1);
  s->n = S.n;
  s->nnz = S.nnz;
  s->Fc = round64(max_batch);
  s->level_ptr = S.level_ptr;
  s->perm = S.perm;
  s->iperm = S.iperm;
  // the launch plan (host, plan.cpp): every record array the kernels gather through, level by level, and the
  // launch schedule of every level (no front reached yet: set_reach below)
  const pfr::Knobs knobs = pfr::knobs_from_env(s->Fc);
  pfr::Plan pl;
  std::string perr;
  if (pfr::build_plan(S, knobs.blk_min, pl, perr)) return bail(fail(PFR_ERR_ARG, perr));
  s->sym = pl.sym;
  Front* d_fronts = nullptr;
  int rc = PFR_OK;
  std::vector<Front> fv(S.fronts);
  if ((rc = s->up(&d_fronts, fv))) return bail(rc);
  int32_t *idx, *relpos, *rowf, *ap, *ac, *an, *ep, *es, *pm, *pr, *pc;
  if ((rc = s->up(&idx, S.idx)) || (rc = s->up(&relpos, S.relpos)) || (rc = s->up(&rowf, S.row_front)) ||
      (rc = s->up(&ap, S.asm_ptr)) || (rc = s->up(&ac, S.asm_col)) || (rc = s->up(&an, S.asm_nz)) ||
      (rc = s->up(&ep, S.ea_ptr)) || (rc = s->up(&es, S.ea_src)) || (rc = s->up(&pm, S.perm)) ||
      (rc = s->up(&pr, S.prow)) || (rc = s->up(&pc, S.pcol)))
    return bail(rc);
  const pfr::I2 z2{0, 0};
  const pfr::I4 n4{-1, -1, -1, -1};
  std::vector<int32_t> cp(colptr, colptr + S.n + 1), ri(rowind, rowind + S.nnz);
  if ((rc = s->up(&s->d_colptr, cp)) || (rc = s->up(&s->d_rowind, ri))) return bail(rc);
  if (s->sym && !S.dir_p.empty()) {
    s->n_dir = pl.n_dir;
    s->n_crow = pl.n_crow;
    if ((rc = s->up_rec(&s->d_dir, pl.dir, z2)) || (rc = s->up_rec(&s->d_crow, pl.crow, 0)) ||
        (rc = s->up(&s->d_cptr_dir, pl.cptr_dir)) || (rc = s->up_rec(&s->d_ce, pl.ce, z2)) ||
        (rc = s->up(&s->d_dptr, pl.dptr)) || (rc = s->up_rec(&s->d_de, pl.de, z2)) || (rc = s->up(&s->d_cslot, pl.cslot)) ||
        (rc = s->alloc(&s->Bc, pfr::workspace(S, s->Fc, s->n_crow).Bc)))
      return bail(rc);
  }
  if ((rc = s->up(&s->d_rptr, pl.rptr)) || (rc = s->up(&s->d_ridx, pl.ridx)) || (rc = s->up(&s->d_rnz, pl.rnz)) ||
      (rc = s->up(&s->d_cptr, pl.cptr)) || (rc = s->up(&s->d_cidx, pl.cidx)) || (rc = s->up(&s->d_cnz, pl.cnz)) ||
      (rc = s->up_rec(&s->d_uent, pl.uent, n4)))
    return bail(rc);
  s->n_uent = pl.n_uent;
  s->h_uent = pl.uent;
  s->P = DevPattern{d_fronts, idx, relpos, rowf, ap, ac, an, ep, es, pm, pr, pc, S.n};
  {
    const int nf = (int)S.fronts.size();
    s->front_of_col.assign(S.n, -1);
    s->front_parent.resize(nf);
    for (int t = 0; t < nf; ++t) {
      const Front& F = S.fronts[t];
      s->front_parent[t] = F.parent;
      s->front_ns.push_back(F.ns);
      s->front_f.push_back(F.f);
      s->front_off.push_back((int32_t)F.off);
      s->front_col0.push_back(F.col0);
      for (int a = 0; a < F.ns; ++a) s->front_of_col[F.col0 + a] = t;
    }
  }
  // the full view: every front (no front reached yet: set_reach)
  if ((rc = upload_view(s, *s, S, pl, knobs))) return bail(rc);
  s->post_n = s->n_dir;
  s->post_dir = s->d_dir;
  s->post_dptr = s->d_dptr;
  s->post_de = s->d_de;
  if (s->sym) {   // what a pruned view is built from (pfr_set_prune)
    s->S = S;
    s->h_dir = pl.dir;
    s->h_dptr = pl.dptr;
    s->h_de = pl.de;
  }
  const int64_t Fc = s->Fc;
  s->ws = pfr::workspace(S, Fc, s->n_crow);
  if ((rc = s->alloc(&s->F, s->ws.F)) || (rc = s->alloc(&s->WV, s->ws.WV)) ||
      (rc = s->alloc(&s->X, (int64_t)S.n * Fc)) || (rc = s->alloc(&s->Y, (int64_t)S.n * Fc)) ||
      (rc = s->alloc(&s->XA, (int64_t)S.n * Fc)) || (rc = s->alloc(&s->G, (int64_t)S.n * Fc)) ||
      (rc = s->alloc(&s->Y2, (int64_t)S.n * Fc)) || (rc = s->alloc(&s->XR, (int64_t)S.n * Fc)) ||
      (rc = s->alloc(&s->freqs, Fc)) || (rc = s->alloc(&s->loss_terms, Fc)) || (rc = s->alloc(&s->flags, Fc)) ||
      (rc = s->alloc(&s->tq, Fc)) || (rc = s->alloc(&s->d_berr_acc, 2 * Fc)) || (rc = s->alloc(&s->fr0, Fc)) ||
      (rc = s->alloc(&s->mscale, Fc)) || (rc = s->alloc(&s->cpart, s->ws.cpart)) ||
      (rc = s->alloc(&s->gind, Fc / 64)) || (rc = s->alloc(&s->glist, pfr::REFINE_CAP)))
    return bail(rc);
  HIP_TRY(hipMemset(s->d_berr_acc, 0, 2 * Fc * sizeof(double)));
  *out = s;
  return PFR_OK;
}

void pfr_solver_destroy(pfr_solver* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  (void)hipDeviceSynchronize();
  delete s;
}

int32_t pfr_solver_max_batch(const pfr_solver* s) { return s ? (int32_t)s->Fc : 0; }

namespace {
// the six tables of a schedule, one after the other (include/pfr.h)
int schedule_out(const pfr::Schedule& sc, int32_t* dst, int64_t cap) {
  static_assert(pfr::schedule_cols<pfr::FactorLevel>() == PFR_SCHED_FACTOR_COLS &&
                    pfr::schedule_cols<pfr::PairLevel>() == PFR_SCHED_PAIR_COLS &&
                    pfr::schedule_cols<pfr::ChainLevel>() == PFR_SCHED_CHAIN_COLS &&
                    pfr::schedule_cols<pfr::SolveLevel>() == PFR_SCHED_SOLVE_COLS,
                "include/pfr.h documents the records' columns");
  if (!dst || cap < (int64_t)sc.factor.size() * PFR_SCHED_COLS * 4) return fail(PFR_ERR_ARG, "destination too small");
  auto put = [&](const auto& v) {
    const size_t bytes = v.size() * sizeof(v[0]);
    if (bytes) std::memcpy(dst, v.data(), bytes);
    dst += bytes / 4;
  };
  put(sc.factor);
  put(sc.pair);
  put(sc.chain);
  for (const auto& v : sc.solve) put(v);
  return PFR_OK;
}
}  // namespace

int pfr_symbolic_schedule(const pfr_symbolic* sym, int32_t max_batch, int32_t* dst, int64_t cap) {
  if (!sym || max_batch <= 0) return fail(PFR_ERR_ARG, "bad arguments");
  const int64_t Fc = round64(max_batch);
  const pfr::Knobs knobs = pfr::knobs_from_env(Fc);
  pfr::Plan pl;
  std::string perr;
  if (pfr::build_plan(sym->S, knobs.blk_min, pl, perr)) return fail(PFR_ERR_ARG, perr);
  const std::vector<int32_t> all[2] = {sym->S.level_ptr, sym->S.level_ptr};   // every front reached
  return schedule_out(pfr::level_schedule(sym->S, pl, Fc, knobs, all), dst, cap);
}

int pfr_symbolic_prune(const pfr_symbolic* sym, int32_t max_batch, const double* rhs, int32_t n_support,
                       const int32_t* index, int32_t* mask_out, int32_t* sched_active, int32_t* sched_rest,
                       int32_t* sched_full, int64_t cap) {
  if (!sym || max_batch <= 0 || !rhs || n_support < 0 || (n_support > 0 && !index) || !mask_out)
    return fail(PFR_ERR_ARG, "bad arguments");
  const Symbolic& S = sym->S;
  const int64_t Fc = round64(max_batch);
  const pfr::Knobs knobs = pfr::knobs_from_env(Fc);
  std::vector<double> rp(S.n);
  for (int p = 0; p < S.n; ++p) rp[p] = rhs[S.perm[p]];
  std::vector<char> mask = pfr::loaded_fronts(S, rp.data());
  for (size_t t = 0; t < mask.size(); ++t) mask_out[t] = mask[t];
  // the reaches a solver sets (pfr_set_rhs, pfr_set_functional): the vector's support and every coupled row; the
  // functional's support
  std::vector<int32_t> rows[2], front_of_col(S.n, -1), front_parent;
  for (const Front& F : S.fronts) {
    for (int a = 0; a < F.ns; ++a) front_of_col[F.col0 + a] = (int32_t)front_parent.size();
    front_parent.push_back(F.parent);
  }
  for (int p = 0; p < S.n; ++p)
    if (rp[p] != 0.0) rows[0].push_back(p);
  for (size_t c = 0; c < S.cpl_p.size(); ++c)
    if (c == 0 || S.cpl_p[c] != S.cpl_p[c - 1]) rows[0].push_back(S.cpl_p[c]);
  for (int i = 0; i < n_support; ++i) {
    if (index[i] < 0 || index[i] >= S.n) return fail(PFR_ERR_ARG, "functional index out of range");
    rows[1].push_back(S.iperm[index[i]]);
  }
  std::vector<int32_t> full_ptr[2], mark, list;
  for (int w = 0; w < 2; ++w)
    pfr::reach_lists(front_of_col, front_parent, S.level_ptr, S.level_fronts, rows[w], mark, list, full_ptr[w]);
  for (int side = 0; side < 3; ++side) {   // the loaded trees, the rest (no forward reach there), every front
    int32_t* dst = side == 0 ? sched_active : side == 1 ? sched_rest : sched_full;
    if (side == 1)
      for (char& m : mask) m = !m;
    if (side == 2) mask.assign(mask.size(), 1);
    pfr::Plan pl;
    std::string perr;
    if (pfr::build_plan(S, knobs.blk_min, pl, perr, &mask)) return fail(PFR_ERR_ARG, perr);
    std::vector<int32_t> reach_ptr[2];
    for (int w = side == 1 ? 1 : 0; w < 2; ++w)
      pfr::reach_lists(front_of_col, front_parent, pl.level_ptr, pl.level_fronts, pfr::rows_in(S, mask, rows[w]), mark, list,
                       reach_ptr[w]);
    const pfr::Schedule sc = pfr::level_schedule(S, pl, Fc, knobs, reach_ptr, &full_ptr);
    std::string bad = pfr::check_plan(S, pl, Fc);
    if (bad.empty()) bad = pfr::check_schedule(S, pl, sc);
    if (!bad.empty())
      return fail(PFR_ERR_STATE, std::string(side == 0 ? "loaded view: " : side == 1 ? "unloaded view: " : "full plan: ") + bad);
    if (dst)
      if (int rc = schedule_out(sc, dst, cap)) return rc;
  }
  return PFR_OK;
}

int pfr_solver_schedule(const pfr_solver* s, int32_t* dst, int64_t cap) {
  if (!s) return fail(PFR_ERR_ARG, "null solver");
  return schedule_out(s->sched, dst, cap);
}

int pfr_set_prune(pfr_solver* s, int32_t on) {
  if (!s) return fail(PFR_ERR_ARG, "null solver");
  HIP_TRY(hipSetDevice(s->device));
  s->prune = on != 0;
  return update_prune(s);
}

int32_t pfr_solver_active(const pfr_solver* s, int32_t* mask, int64_t cap) {
  if (!s) return -1;
  const int64_t nf = (int64_t)s->front_ns.size();
  int32_t count = 0;
  for (int64_t t = 0; t < nf; ++t) {
    const int32_t a = s->act ? s->act->active[t] != 0 : 1;
    count += a;
    if (mask && t < cap) mask[t] = a;
  }
  return s->act ? count : (int32_t)nf;
}

int pfr_solver_schedule_active(const pfr_solver* s, int32_t* dst, int64_t cap) {
  if (!s) return fail(PFR_ERR_ARG, "null solver");
  return schedule_out(s->act ? s->act->sched : s->sched, dst, cap);
}

int32_t pfr_symbolic_live(const pfr_symbolic* sym, const double* rhs, int32_t prune, int32_t n_stiff,
                          const double* stiff_host, uint32_t* live) {
  if (!sym || !rhs || !stiff_host || n_stiff <= 0 || n_stiff > 18 || !sym->S.symmetric) return -1;
  const Symbolic& S = sym->S;
  std::vector<char> mask;
  if (prune) {
    std::vector<double> rp(S.n);
    for (int p = 0; p < S.n; ++p) rp[p] = rhs[S.perm[p]];
    mask = pfr::loaded_fronts(S, rp.data());
  }
  const uint32_t l = pfr::live_stiffness(S, prune ? &mask : nullptr, pfr::stiffness_bits(stiff_host, S.nnz, n_stiff));
  if (live) *live = l;
  return __builtin_popcount(l);
}

int32_t pfr_solver_live(const pfr_solver* s, uint32_t* live, int32_t* compact) {
  if (!s) return -1;
  const SolverView& v = sweeps_pruned(s) ? *s->act : static_cast<const SolverView&>(*s);
  if (live) *live = v.live;
  if (compact) *compact = v.d_se_live != nullptr;
  return v.n_live;
}

int32_t pfr_symbolic_mass_list(const pfr_symbolic* sym, const double* rhs, int32_t prune, int32_t n_mass,
                               const double* mass_host, int32_t* list, int64_t cap, int32_t* ptr, int64_t ptr_cap,
                               int32_t* entries, int64_t entries_cap, int32_t* counts) {
  if (!sym || !mass_host || n_mass < 1 || n_mass > pfr::MASS_NM || (prune && (!rhs || !sym->S.symmetric))) return -1;
  const Symbolic& S = sym->S;
  pfr::Plan pl;
  std::string perr;
  if (pfr::build_plan(S, pfr::knobs_from_env(64).blk_min, pl, perr)) return -1;
  std::vector<char> rows;
  if (prune) {
    std::vector<double> rp(S.n);
    for (int p = 0; p < S.n; ++p) rp[p] = rhs[S.perm[p]];
    rows = pfr::front_rows(S, pfr::loaded_fronts(S, rp.data()));
  }
  const pfr::MassList L =
      pfr::mass_entries(pl.uent, pl.n_uent, S.n, prune ? &rows : nullptr, pfr::mass_on(mass_host, S.nnz, n_mass));
  const std::vector<int32_t>& l = L.list;
  if (list) std::copy(l.begin(), l.begin() + std::min<int64_t>(cap, (int64_t)l.size()), list);
  if (ptr) std::copy(L.ptr.begin(), L.ptr.begin() + std::min<int64_t>(ptr_cap, (int64_t)L.ptr.size()), ptr);
  if (entries)
    for (int64_t e = 0; e < pl.n_uent && 4 * e + 3 < entries_cap; ++e) {
      const pfr::I4& u = pl.uent[e];
      entries[4 * e] = u.x, entries[4 * e + 1] = u.y, entries[4 * e + 2] = u.z, entries[4 * e + 3] = u.w;
    }
  if (counts) counts[0] = pl.n_uent, counts[1] = (int32_t)l.size(), counts[2] = (int32_t)L.ptr.size() - 1;
  return (list && cap < (int64_t)l.size()) || (ptr && ptr_cap < (int64_t)L.ptr.size()) ? -1 : L.n_list;
}

int32_t pfr_solver_mass_list(const pfr_solver* s, int32_t* padded) {
  if (!s) return -1;
  const SolverView& v = sweeps_pruned(s) ? *s->act : static_cast<const SolverView&>(*s);
  if (padded) *padded = s->mass ? v.len_mlist : 0;
  return s->mass ? v.n_mlist : -1;
}

int pfr_set_timing(pfr_solver* s, int32_t enable) {
  if (!s) return fail(PFR_ERR_ARG, "null solver");
  ++s->gen;
  s->timing = enable == 0 ? 0 : (enable | 1);
  return PFR_OK;
}

namespace {
// The last chunk's adjoint on the unloaded trees, which a pruned sweep leaves zero (nothing it returns reads it): those
// fronts factorised from the retained chunk operator and the adjoint solved on them for the seed the sweep left in G
// (the same per-frequency coefficients), once per chunk.  The loaded rows keep what the sweep computed.
int complete_adjoint(pfr_solver* s) {
  if (!s->act || !s->last_pruned || !s->last_adj || s->comp_done) return PFR_OK;
  int rc;
  if (!s->comp) {
    std::vector<char> mask(s->act->active);
    for (char& m : mask) m = !m;
    if ((rc = make_view(s, mask, false, &s->comp))) return rc;
  }
  const int timing = s->timing;
  s->timing = 0;
  rc = factor_all(s, *s->comp, s->last_op, pfr::MAT_OPERATOR, nullptr, 0, (int)s->Fc, s->last_st);
  if (rc == PFR_OK) rc = adjoint_solve(s, *s->comp, s->last_op, rhs_vector(s->G), s->XA, s->last_st, s->last_reach);
  s->timing = timing;
  s->comp_done = true;
  s->unl_dirty = true;
  return rc;
}
}  // namespace

int pfr_debug_solution(pfr_solver* s, int32_t which, int32_t q, double* out) {
  if (!s || !out || which < 0 || which > 1 || q < 0 || q >= s->Fc) return fail(PFR_ERR_ARG, "bad debug arguments");
  HIP_TRY(hipSetDevice(s->device));
  if (which == 1)
    if (int rc = complete_adjoint(s)) return rc;
  HIP_TRY(hipDeviceSynchronize());
  std::vector<double2> col((size_t)s->n);
  const double2* src = which == 0 ? s->X : s->XA;
  HIP_TRY(hipMemcpy2D(col.data(), sizeof(double2), src + q, (size_t)s->Fc * sizeof(double2), sizeof(double2), s->n,
                      hipMemcpyDeviceToHost));
  for (int p = 0; p < s->n; ++p) {       // permuted row p holds caller row perm[p]
    out[2 * (int64_t)s->perm[p]] = col[p].x;
    out[2 * (int64_t)s->perm[p] + 1] = col[p].y;
  }
  return PFR_OK;
}

int pfr_set_refine_tol(pfr_solver* s, double tol) {
  if (!s || !(tol >= 0.0)) return fail(PFR_ERR_ARG, "bad refine tolerance");
  ++s->gen;
  s->refine_tol = tol;
  return PFR_OK;
}

int pfr_set_check(pfr_solver* s, int32_t mode, double tol, double* berr_dev) {
  if (!s || mode < 0 || mode > 31 || !(tol >= 0.0)) return fail(PFR_ERR_ARG, "bad check arguments");
  s->check_mode = mode;
  s->check_tol = tol;
  s->berr_out = berr_dev;
  return PFR_OK;
}

int pfr_last_timings(const pfr_solver* s, double* ms) {
  if (!s || !ms) return fail(PFR_ERR_ARG, "null argument");
  for (int i = 0; i < 5; ++i) ms[i] = 0.0;
  if (s->n_tev > 0) HIP_TRY(hipEventSynchronize(s->tev[s->n_tev - 1].ev[5]));
  for (int c = 0; c < s->n_tev; ++c)
    for (int i = 0; i < 5; ++i)
      if (s->tev[c].used[i]) {
        float m = 0;
        HIP_TRY(hipEventElapsedTime(&m, s->tev[c].ev[i], s->tev[c].ev[i + 1]));
        ms[i] += m;
      }
  return PFR_OK;
}

int pfr_last_kernel_timings(const pfr_solver* s, double* ms, int64_t* launches) {
  if (!s || !ms) return fail(PFR_ERR_ARG, "null argument");
  for (int i = 0; i < pfr::NKC; ++i) {
    ms[i] = 0.0;
    if (launches) launches[i] = 0;
  }
  if (!(s->timing & 2) || s->n_tev == 0) return PFR_OK;
  HIP_TRY(hipEventSynchronize(s->tev[s->n_tev - 1].ev[5]));
  const int L = (int)s->level_ptr.size() - 1;
  for (int c = 0; c < s->n_tev; ++c) {
    if (!s->tev[c].used[0]) continue;
    for (int l = 0; l < L; ++l) {
      // the records the last call's level loops launched: the loaded trees' under pruning
      const pfr::FactorLevel& r = (s->last_pruned && s->act ? s->act->sched : s->sched).factor[l];
      int work[pfr::NKC] = {r.nasm, r.nf, r.nitems, r.nblocks, r.ntiles};
      if (l == 0 && s->tev[c].f0) {   // the fused bottom level: one or two k_front0 launches, all in class 0
        work[0] = (r.f0_small > 0) + (r.nf > r.f0_small);
        for (int k = 1; k < pfr::NKC; ++k) work[k] = 0;
      }
      for (int k = 0; k < pfr::NKC; ++k) {
        float m = 0;
        HIP_TRY(hipEventElapsedTime(&m, s->tev[c].kev[(pfr::NKC + 1) * l + k], s->tev[c].kev[(pfr::NKC + 1) * l + k + 1]));
        ms[k] += m;
        if (launches) launches[k] += l == 0 && s->tev[c].f0 ? work[k] : work[k] > 0;   // empty classes launch nothing
      }
    }
  }
  return PFR_OK;
}

int pfr_solver_alg_bytes(const pfr_solver* s, int64_t* bytes) {
  if (!s || !bytes) return fail(PFR_ERR_ARG, "null argument");
  for (int i = 0; i < pfr::NKC; ++i) bytes[i] = 0;
  // what the operator-form sweeps launch under the current check mode
  const SolverView& v = sweeps_pruned(s) ? *s->act : static_cast<const SolverView&>(*s);
  for (int l = 0; l + 1 < (int)s->level_ptr.size(); ++l)
    for (int i = 0; i < pfr::NKC; ++i) bytes[i] += v.lev_bytes[l][i];
  return PFR_OK;
}

int pfr_solver_solve_bytes(const pfr_solver* s, int64_t* bytes) {
  if (!s || !bytes) return fail(PFR_ERR_ARG, "null argument");
  // factor entries each pass reads once: lower[w] = L11 + L21 of the fronts reach w holds (the
  // bottom-up pass of rhs w), upper_r[w] = U11 + U12 of those fronts, upper / lower_all = every front
  int64_t lower[2] = {0, 0}, upper_r[2] = {0, 0}, upper = 0, lower_all = 0, lower_union = 0, sup_rows = 0;
  const bool refine = (s->check_mode & PFR_CHECK_REFINE) != 0;
  const SolverView& v = sweeps_pruned(s) ? *s->act : static_cast<const SolverView&>(*s);   // the fronts the sweeps walk
  int64_t nrows = 0;
  for (size_t t = 0; t < s->front_ns.size(); ++t) {
    if (!v.active[t]) continue;
    const int64_t ns = s->front_ns[t], r = s->front_f[t] - ns;
    nrows += ns;
    const int64_t u = ns * (ns + 1) / 2 + r * ns;             // U11 + U12 (symmetric: diag(U) L^T)
    const int64_t l = ns * (ns - 1) / 2 + r * ns;             // L11 (unit diagonal) + L21
    upper += u;
    lower_all += l;
    if (v.reach_host[0][t] || v.reach_host[1][t]) lower_union += l;
    if (v.reach_host[1][t]) sup_rows += ns;
    for (int w = 0; w < 2; ++w)
      if (v.reach_host[w][t]) {
        lower[w] += l;
        upper_r[w] += u;
      }
  }
  const int64_t vec = 2 * 16 * nrows;                         // rhs in, solution out
  if (s->sym && !refine && s->fn_dot) {
    // loss sweep, functional from the bottom-up passes: ONE bottom-up chain over the rhs reach and the
    // support reach together (the support's three vectors share each L value of their fronts) + the
    // paired top-down pass over every front (each U value once for the adjoint and the forward solution)
    bytes[0] = 16 * lower_union + vec + 3 * 32 * sup_rows;
    bytes[1] = 16 * upper + 2 * vec;
  } else if (s->sym && !refine) {
    // loss sweep, paired: forward bottom-up over its reach + forward top-down over the fronts the loss
    // support reaches; adjoint bottom-up over that reach + ONE top-down pass over every front that
    // forms the adjoint and the rest of the forward solution together (each U value loaded once)
    bytes[0] = 16 * (lower[0] + upper_r[1]) + vec;
    bytes[1] = 16 * (lower[1] + upper) + 2 * vec;
  } else {
    // forward and adjoint solved one after the other; a refinement step adds a full pair each
    const int64_t ref = refine ? 16 * (lower_all + upper) + vec : 0;
    bytes[0] = 16 * (lower[0] + upper) + vec + ref;
    bytes[1] = 16 * (lower[1] + upper) + vec + ref;
  }
  return PFR_OK;
}

int pfr_set_stiffness(pfr_solver* s, int32_t n_stiff, const double* stiff_dev, const double* w) {
  if (!s || (n_stiff != 12 && n_stiff != 18) || !stiff_dev || !w)
    return fail(PFR_ERR_ARG, "bad stiffness arguments (n_stiff must be 12 or 18)");
  ++s->gen;
  s->stiff = stiff_dev;
  s->n_stiff = n_stiff;
  std::memset(&s->e, 0, sizeof(s->e));
  for (int k = 0; k < n_stiff; ++k) s->e.re[k] = w[k];
  HIP_TRY(hipSetDevice(s->device));
  if (!s->partial) {
    // written by k_contract_eg (contract_eg_parts(n_uent) parts) and by k_reduce_q (one part per 64-frequency
    // tile of the chunk: Fc / 64), 18 partials each
    const int64_t parts = std::max<int64_t>(pfr::contract_eg_parts(s->n_uent), s->Fc / 64);
    int rc = s->alloc(&s->partial, parts * 18);
    if (rc) return rc;
  }
  if (!s->d_se) {
    int rc = s->alloc(&s->d_se, (int64_t)18 * (s->n_uent + 4));
    if (rc) return rc;
  }
  // the entry-ordered copy of S the gradient contraction reads (taken now: a later change of the
  // registered buffer needs another pfr_set_stiffness, include/pfr.h)
  pfr::launch_gather_entries(s->d_uent, s->n_uent + 4, stiff_dev, n_stiff, s->d_se, nullptr);
  HIP_TRY(hipStreamSynchronize(nullptr));
  // the live matrices of the walks (the full view's and the loaded trees'), from the table's values
  s->stiff_bits.clear();
  if (s->sym) {
    std::vector<double> host((size_t)s->nnz * n_stiff);
    HIP_TRY(hipMemcpy(host.data(), stiff_dev, host.size() * 8, hipMemcpyDeviceToHost));
    s->stiff_bits = pfr::stiffness_bits(host.data(), s->nnz, n_stiff);
  }
  if (int rc = update_live(s, *s)) return rc;
  if (s->act)
    if (int rc = update_live(s, *s->act)) return rc;
  return PFR_OK;
}

int pfr_set_inertia(pfr_solver* s, int32_t n_mass, const double* mass_dev, const double* w) {
  if (!s || n_mass < 1 || n_mass > pfr::MASS_NM || !mass_dev || !w)
    return fail(PFR_ERR_ARG, "bad inertia arguments (n_mass must be 1 .. 4)");
  ++s->gen;
  HIP_TRY(hipSetDevice(s->device));
  if (!s->d_me) {
    int rc = s->alloc(&s->d_me, (int64_t)pfr::MASS_NM * (s->n_uent + 4));
    if (rc) return rc;
  }
  // the entry-ordered copy the contraction reads (taken now: a later change of the registered buffer needs another
  // pfr_set_inertia) and, from the table's values, the entries the views' lists keep
  (void)hipDeviceSynchronize();   // launches that read the copy
  pfr::launch_gather_mass(s->d_uent, s->n_uent + 4, mass_dev, n_mass, s->d_me, nullptr);
  std::vector<double> host((size_t)s->nnz * n_mass);
  HIP_TRY(hipMemcpy(host.data(), mass_dev, host.size() * 8, hipMemcpyDeviceToHost));
  s->mass_nz = pfr::mass_on(host.data(), s->nnz, n_mass);
  s->mass = mass_dev;
  s->n_mass = n_mass;
  s->mass_d = pfr::MassWeights{};
  for (int j = 0; j < n_mass; ++j) s->mass_d.d[j] = w[j];
  if (int rc = update_mass(s, *s)) return rc;
  if (s->act)
    if (int rc = update_mass(s, *s->act)) return rc;
  return PFR_OK;
}

int pfr_combine(pfr_solver* s, const double* coef, double* K_out, void* stream) {
  if (!s || !coef || !K_out) return fail(PFR_ERR_ARG, "null argument");
  if (!s->stiff) return fail(PFR_ERR_STATE, "pfr_set_stiffness not called");
  HIP_TRY(hipSetDevice(s->device));
  pfr::CoefPack c{};
  for (int k = 0; k < s->n_stiff; ++k) {
    c.re[k] = coef[2 * k];
    c.im[k] = coef[2 * k + 1];
  }
  pfr::launch_combine(s->stiff, s->n_stiff, s->nnz, c, reinterpret_cast<double2*>(K_out), (hipStream_t)stream);
  LAUNCH_TRY();
  return PFR_OK;
}

int pfr_set_operator(pfr_solver* s, const double* K_dev, const double* M_dev) {
  if (!s || !K_dev || !M_dev) return fail(PFR_ERR_ARG, "null argument");
  ++s->gen;
  s->K = reinterpret_cast<const double2*>(K_dev);
  s->M = M_dev;
  return PFR_OK;
}

int pfr_set_rhs(pfr_solver* s, const double* rhs, double beta_re, double beta_im, double mass_sum) {
  if (!s || !rhs) return fail(PFR_ERR_ARG, "null argument");
  ++s->gen;
  s->beta_re = beta_re;
  s->beta_im = beta_im;
  s->mass_sum = mass_sum;
  // the Dirichlet vector rarely changes (only the scale does, per theta): upload it
  // only when it differs from the last one (no device allocation per call)
  if (s->has_rhs && std::equal(s->rhs_host.begin(), s->rhs_host.end(), rhs)) return PFR_OK;
  HIP_TRY(hipSetDevice(s->device));
  std::vector<double> rp(s->n);
  std::vector<int32_t> sup;
  std::vector<double> val;
  for (int p = 0; p < s->n; ++p) {
    rp[p] = rhs[s->perm[p]];
    if (rp[p] != 0.0) {
      sup.push_back(p);
      val.push_back(rp[p]);
    }
  }
  int rc;
  if (!s->rhsP) {
    if ((rc = s->alloc(&s->rhsP, s->n)) || (rc = s->alloc(&s->rhs_sup, s->n)) || (rc = s->alloc(&s->rhs_val, s->n)))
      return rc;
  }
  HIP_TRY(hipMemcpy(s->rhsP, rp.data(), s->n * 8, hipMemcpyHostToDevice));
  if (!sup.empty()) {
    HIP_TRY(hipMemcpy(s->rhs_sup, sup.data(), sup.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->rhs_val, val.data(), val.size() * 8, hipMemcpyHostToDevice));
  }
  s->n_rhs_sup = (int)sup.size();
  {
    // forward reach: rhs support (+ rows coupled to Dirichlet columns in symmetric mode)
    std::vector<int32_t> rows(sup);
    std::vector<int32_t> crow(std::max(1, s->n_crow));
    if (s->sym && s->n_crow > 0) {
      HIP_TRY(hipMemcpy(crow.data(), s->d_crow, s->n_crow * 4, hipMemcpyDeviceToHost));
      rows.insert(rows.end(), crow.begin(), crow.begin() + s->n_crow);
    }
    s->reach_rows[0] = rows;
    if ((rc = set_reach(s, *s, 0, rows))) return rc;
  }
  s->rhs_host.assign(rhs, rhs + s->n);
  s->has_rhs = true;
  // the loaded trees follow the vector's support (pfr_set_prune); the same trees: the view's forward reach again
  const SolverView* before = s->act;
  if ((rc = update_prune(s))) return rc;
  if (s->act && s->act == before &&
      (rc = set_reach(s, *s->act, 0, pfr::rows_in(s->S, s->act->active, s->reach_rows[0]))))
    return rc;
  return PFR_OK;
}

int pfr_set_functional(pfr_solver* s, int32_t n_support, const int32_t* index, const double* a, double ts) {
  if (!s || n_support <= 0 || !index || !a) return fail(PFR_ERR_ARG, "bad functional arguments");
  ++s->gen;
  HIP_TRY(hipSetDevice(s->device));
  std::vector<int32_t> pidx(n_support);
  for (int i = 0; i < n_support; ++i) {
    if (index[i] < 0 || index[i] >= s->n) return fail(PFR_ERR_ARG, "functional index out of range");
    pidx[i] = s->iperm[index[i]];
  }
  std::vector<double> av(a, a + 3 * (int64_t)n_support);
  int32_t* d_idx;
  double* d_a;
  int rc;
  if ((rc = s->up(&d_idx, pidx)) || (rc = s->up(&d_a, av))) return rc;
  s->reach_rows[1] = pidx;
  if ((rc = set_reach(s, *s, 1, pidx))) return rc;    // loss adjoint reach: functional support
  // the sensor rows on unloaded trees multiply exact zeros of the forward solution: the pruned view drops them
  if (s->act && (rc = set_reach(s, *s->act, 1, pfr::rows_in(s->S, s->act->active, pidx)))) return rc;
  release_view(s, s->comp);
  s->a_perm.assign(3 * (size_t)s->n, 0.0);
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < n_support; ++i) s->a_perm[(size_t)k * s->n + pidx[i]] += av[(size_t)k * n_support + i];
  if (s->d_aP) HIP_TRY(hipMemcpy(s->d_aP, s->a_perm.data(), s->a_perm.size() * 8, hipMemcpyHostToDevice));
  s->fn.n_support = n_support;
  s->fn.pidx = d_idx;
  s->fn.a = d_a;
  s->fn.ts = ts;
  s->has_fn = true;
  return PFR_OK;
}

}  // extern "C"

namespace {
// What a sweep senses: the magnitude fr (the default) or the complex response H along a real axis (pfr_sweep_complex).
// A value of the call, never solver state: functional_args writes it into the sweep's FunctionalArgs.
struct Response {
  bool cpx = false;
  double axis[3] = {0.0, 0.0, 1.0};
};

// What one sweep call asks for: every pfr_*sweep* entry point fills one after its argument checks.
// jc != NULL (the Jacobian forms; loss_type = pfr::LOSS_UNIT, scale 1, no ref / loss / w): the reverse sweep of a unit
// cotangent per frequency whose contraction stays per frequency -- the walk's kpart (or k_contract_q's, where the walk
// has not formed it) finished by k_jac_finish into the rows of jc instead of k_reduce_q / k_contract_eg + k_reduce into w.
// jm != NULL (pfr_inertia_sweep): that sweep with the inertia rows too -- after k_jac_finish (skipped with its contraction
// when jc == NULL) k_contract_mass / k_inertia_finish contract the same x and mu with the mass components into jm.
// pop.member != NULL (pfr_population_sweep): lane group g belongs to pop.member[g] and reads the operator popK +
// pop.member[g] * pop.nnz (chunk_op).  resp.cpx (the complex sweeps): response holds complex H, loss_type is a PFR_LOSS_C*
// id, pfr::LOSS_UNIT or PFR_LOSS_NONE, and the functional kernels run in their CPX forms (seed kept in s->h0); every
// launch after them takes G, fcoef and mscale as it does for the magnitude.
// field.out != NULL (pfr_field_sweep): the forward sweep whose solution leaves the device -- after the chunk's passes
// k_field_gather writes the rows field.sel (permuted, n_sel of them) of X to field.out, frequency-major; the functional
// runs only for a caller who takes fr.  check_mask: the pfr_set_check bits the call honours (the field sweep: the
// forward check and the refinement; it has no functional to correct and no adjoint).
struct FieldOut {
  double2* out = nullptr;
  const int32_t* sel = nullptr;
  int32_t n_sel = 0;
};
// floss.ref != NULL (pfr_field_loss_sweep): the loss is on the solution's rows -- in place of the functional kernels
// launch_field_loss writes the seed into G for every selected row, so the adjoint runs unpaired over every front; the
// loss terms and the contraction then go the way of any reverse sweep without the correction.  field.out may be set too.
struct SweepSpec {
  int32_t nfreq = 0;
  const double* freqs = nullptr;
  int32_t loss_type = PFR_LOSS_NONE;
  const double* ref = nullptr;
  double scale = 1.0;
  double* response = nullptr;           // fr per frequency, or the complex H (resp.cpx)
  double *loss = nullptr, *w = nullptr;
  double2* jc = nullptr;
  double2* jm = nullptr;                // the inertia rows (pfr_inertia_sweep), beside or instead of jc
  int32_t* flags = nullptr;
  bool fresh = false;                   // the caller's outputs initialised by the first chunk (pfr_sweep_fresh)
  const double2* popK = nullptr;
  pfr::PopArgs pop;
  Response resp;
  FieldOut field;
  pfr::FieldLossArgs floss;
  int32_t check_mask = ~0;
  double* fr() const { return resp.cpx ? nullptr : response; }   // where the magnitude kernels write fr
};

// Every control-flow decision of a sweep, made once before the chunk loop (sweep_passes); the phases derive none
struct SweepPasses {
  bool reverse = false;      // a loss (or unit) cotangent is pulled back
  bool correct = false;      // functional correction: the adjoint of fr is solved in every sweep (in a loss sweep it IS
                             // the loss adjoint up to one scalar per frequency) and the forward walk adds Re(mu^T r) to fr
  bool adj = false;          // an adjoint solve runs
  bool refine = false;       // one refinement step of each solve (PFR_CHECK_REFINE)
  bool paired = false;       // one top-down pass for both solutions
  bool fwd_late = false;     // forward residual walk after the adjoint
  bool fn_fast = false;      // functional from the bottom-up passes
  bool pruned = false;       // on the loaded trees' view (sweeps_pruned)
  bool jac = false;          // the contraction stays per frequency (spec.jc)
  bool functional = true;    // the functional kernels run (a field sweep without fr: not)
  bool field = false;        // the chunk's solution rows gathered to the caller (spec.field)
  bool floss = false;        // the loss and its seed from the solution's rows (spec.floss), in place of the functional
  pfr::Reach adj_reach = pfr::REACH_SUPPORT;   // the fronts the unpaired adjoint's bottom-up pass visits
  bool cwalk = false;        // the gradient contraction rides on the forward residual walk (loss sweeps with the correction)
  bool refine_adj = false;   // selective adjoint refinement of the groups next to a resonance (PFR_CHECK_REFINE_ADJ)
  bool scorr = false;        // the solve-error scale of the cotangent (k_correct_finish): t_q = mu^T rhsP in, m_q t_q out
  // the backward-error checks: forward -- after the forward solve, on the correction walk or after the adjoint -- and adjoint
  bool check_fwd_early = false, check_fwd_walk = false, check_fwd_after = false, check_adj = false;
};

SweepPasses sweep_passes(const pfr_solver* s, const SweepSpec& sp) {
  SweepPasses p;
  const int mode = s->check_mode & sp.check_mask;
  p.reverse = sp.loss_type != PFR_LOSS_NONE;
  p.jac = sp.jc != nullptr || sp.jm != nullptr;
  p.field = sp.field.out != nullptr;
  p.floss = sp.floss.ref != nullptr;
  p.functional = p.floss || !p.field || sp.response != nullptr;
  if (p.floss) p.adj_reach = pfr::REACH_ALL;   // the seed is on any row, not on the support's reach
  p.refine = (mode & PFR_CHECK_REFINE) != 0;
  p.correct = (mode & PFR_CHECK_CORRECT) != 0;
  p.adj = p.reverse || p.correct;
  p.paired = s->sym && p.adj && !p.refine && !p.floss;
  p.fwd_late = p.paired || p.correct;
  p.fn_fast = p.paired && s->fn_dot;
  p.pruned = sweeps_pruned(s, mode);
  p.cwalk = p.reverse && p.correct && s->contract_walk && (s->n_stiff == 12 || s->n_stiff == 18);
  p.refine_adj =
      p.reverse && p.correct && p.cwalk && p.fn_fast && !sp.resp.cpx && (mode & PFR_CHECK_REFINE_ADJ);
  p.scorr = p.reverse && p.correct && s->scale_corr;
  const bool want_f = p.fwd_late && (mode & PFR_CHECK_FORWARD);
  p.check_fwd_early = !p.paired && !p.fwd_late && (mode & PFR_CHECK_FORWARD);
  p.check_fwd_walk = want_f && p.correct;
  p.check_fwd_after = want_f && !p.correct;
  p.check_adj = p.adj && (mode & PFR_CHECK_ADJOINT) != 0;
  return p;
}

// One chunk of a sweep: first frequency, count, stream, the operator's right-hand side, the functional the call asks for
struct Chunk {
  int64_t q0 = 0;
  int nv = 0;
  hipStream_t st = nullptr;
  pfr::RhsArgs rd;
  pfr::FunctionalArgs fa{};
};

pfr::FunctionalArgs functional_args(const pfr_solver* s, const SweepSpec& sp) {
  pfr::FunctionalArgs fa = s->fn;
  fa.loss_type = sp.loss_type != PFR_LOSS_NONE ? sp.loss_type : -1;
  fa.ref = reinterpret_cast<const double2*>(sp.ref);
  fa.scale = sp.scale;
  if (sp.resp.cpx) {
    fa.cpx = 1;
    std::copy(sp.resp.axis, sp.resp.axis + 3, fa.axis);
    fa.h_out = reinterpret_cast<double2*>(sp.response);
  }
  return fa;
}
// seed mode of the functional kernels: the response of this solve kept for k_correct_finish
pfr::FunctionalArgs seeded(const pfr_solver* s, pfr::FunctionalArgs f) {
  f.cpx ? (void)(f.h0 = s->h0) : (void)(f.fr0 = s->fr0);
  return f;
}

// The view a call walks, and the unloaded trees' rows of X / XA: zeroed here, kept by pruned sweeps, dirty after others
SolverView& begin_on_view(pfr_solver* s, bool pruned, hipStream_t st) {
  if (pruned && s->unl_dirty) {
    for (const auto& r : s->unl_rows) {
      pfr::launch_zero(s->X + (int64_t)r.first * s->Fc, (int64_t)(r.second - r.first) * s->Fc, st);
      pfr::launch_zero(s->XA + (int64_t)r.first * s->Fc, (int64_t)(r.second - r.first) * s->Fc, st);
    }
    s->unl_dirty = false;
  } else if (!pruned && s->act) {
    s->unl_dirty = true;
  }
  s->last_pruned = pruned;
  return pruned ? *s->act : static_cast<SolverView&>(*s);
}

// The phases of one chunk, split at the timing records.  The factorisation (paired: the operator rhs's Dirichlet move first):
int phase_factor(pfr_solver* s, SolverView& v, const pfr::ChunkOp& op, const SweepPasses& ps, const SweepSpec&,
                 const Chunk& c) {
  if (ps.paired)
    pfr::launch_dirichlet_rhs(pfr::RHS_OPERATOR, dir_desc(s, op), op.pop, s->n_crow, c.rd, nullptr, s->Bc, s->Fc, c.st);
  return factor_all(s, v, op, pfr::MAT_OPERATOR, nullptr, 0, c.nv, c.st);
}

// The forward solve.  Paired (symmetric mode with an adjoint): the bottom-up pass and the top-down pass only over the loss
// support's fronts -- one combined top-down pass follows (sym_top_down_pair); otherwise the full forward solve
int phase_forward(pfr_solver* s, SolverView& v, const pfr::ChunkOp& op, const SweepPasses& ps, const SweepSpec&,
                  const Chunk& c) {
  int rc;
  if (ps.paired) {
    const pfr::Rhs rhs = s->n_crow > 0 ? pfr::RHS_OPERATOR_DIR : pfr::RHS_OPERATOR;
    pfr::RhsArgs rf = c.rd;   // the operator's, with the Dirichlet corrections (phase_factor) in their slots
    rf.cslot = s->d_cslot;
    rf.Bc = s->Bc;
    if (ps.fn_fast) return fn_bottom_up(s, v, op, rhs, rf, c.st);
    if ((rc = solve_all(s, v, op, pfr::TRI_L, rhs, rf, nullptr, s->Y, c.st, pfr::REACH_RHS))) return rc;
    return sym_top_down_support(s, v, c.st);
  }
  if ((rc = forward_solve(s, v, op, pfr::RHS_OPERATOR, c.rd, s->X, c.st, pfr::REACH_RHS))) return rc;
  if (ps.refine) {
    // one refinement step on the same factors: r = b - A x (into G), A d = r (into XA), x += d
    run_walk(s, v, op, Walk::residual(Walk::FORWARD, pfr::RHS_OPERATOR, c.rd, s->X, s->G), c.nv, c.st);
    if ((rc = forward_solve(s, v, op, pfr::RHS_VECTOR, rhs_vector(s->G), s->XA, c.st))) return rc;
    pfr::launch_axpy_vec(s->X, s->XA, (int64_t)s->n * s->Fc, c.st);
  }
  if (ps.check_fwd_early)
    run_walk(s, v, op, Walk::checked(Walk::FORWARD, pfr::RHS_OPERATOR, c.rd, s->X, c.q0), c.nv, c.st);
  return PFR_OK;
}

void phase_functional(pfr_solver* s, SolverView& v, const pfr::ChunkOp&, const SweepPasses& ps, const SweepSpec& sp,
                      const Chunk& c) {
  const int64_t Fc = s->Fc;
  if (ps.adj) pfr::launch_zero(s->G, (int64_t)s->n * Fc, c.st);
  if (ps.floss) {
    pfr::FieldLossArgs a = sp.floss;
    a.ref += c.q0 * a.n_sel;
    pfr::launch_field_loss(a, s->X, Fc, c.nv, s->G, s->fpart, s->loss_terms, s->fseed, c.st);
  } else if (ps.fn_fast) {
    const double2* Yk[3] = {s->Y2, s->YVk, s->YVk + (int64_t)s->n * Fc};
    pfr::launch_fn_dot(v.d_fn_rows, v.n_fn_rows, s->F, s->Y, Yk, Fc, s->fn_parts, c.st);
    pfr::launch_functional_fn(ps.correct ? seeded(s, c.fa) : c.fa, s->fn_parts, Fc, c.nv, c.q0,
                              ps.correct ? nullptr : sp.fr(), ps.correct ? nullptr : s->loss_terms, s->G, s->fcoef, c.st);
  } else if (ps.correct) {   // fr of this solve kept, G = d fr / d x
    pfr::launch_functional(seeded(s, c.fa), s->X, Fc, c.nv, c.q0, nullptr, nullptr, s->G, c.st);
  } else {
    pfr::launch_functional(c.fa, s->X, Fc, c.nv, c.q0, sp.fr(), s->loss_terms, s->G, c.st);
  }
}

// the adjoint for the seed in G (ps.adj)
int phase_adjoint(pfr_solver* s, SolverView& v, const pfr::ChunkOp& op, const SweepPasses& ps, const SweepSpec&,
                  const Chunk& c) {
  int rc;
  const int64_t Fc = s->Fc;
  const pfr::RhsArgs rg = rhs_vector(s->G);
  if (ps.fn_fast) {
    double2* Yk[3] = {s->Y2, s->YVk, s->YVk + (int64_t)s->n * Fc};
    pfr::launch_fn_combine(v.d_sup_rows, v.n_sup_rows, s->fcoef, Yk, Fc, c.st);
    if ((rc = sym_top_down_pair(s, v, c.st, true))) return rc;
    pfr::launch_dirichlet_post(post_desc(s, v, op), op.pop, v.post_n, s->XA, Fc, c.st);
    // the correction fr(x) + Re(mu^T r) needs fr OF the solution x whose residual r is walked (the
    // dot product's fr has its own rounding error, which the correction does not see): fr0 from x
    if (ps.correct) pfr::launch_functional(seeded(s, c.fa), s->X, Fc, c.nv, c.q0, nullptr, nullptr, nullptr, c.st);
  } else if (ps.paired) {
    if ((rc = solve_all(s, v, op, pfr::TRI_L, pfr::RHS_VECTOR, rg, nullptr, s->Y2, c.st, pfr::REACH_SUPPORT)) ||
        (rc = sym_top_down_pair(s, v, c.st)))
      return rc;
    pfr::launch_dirichlet_post(post_desc(s, v, op), op.pop, v.post_n, s->XA, Fc, c.st);
  } else {
    if ((rc = adjoint_solve(s, v, op, rg, s->XA, c.st, ps.adj_reach))) return rc;
    if (ps.refine) {
      // l += A^{-T} (g - A^T l): residual into Y2, correction into XR
      run_walk(s, v, op, Walk::residual(Walk::ADJOINT, pfr::RHS_VECTOR, rg, s->XA, s->Y2), c.nv, c.st);
      if ((rc = adjoint_solve(s, v, op, rhs_vector(s->Y2), s->XR, c.st))) return rc;
      pfr::launch_axpy_vec(s->XA, s->XR, (int64_t)s->n * Fc, c.st);
    }
  }
  return PFR_OK;
}

// after the adjoint (ps.adj): the walks, the correction, the contraction and the finish into the caller's outputs
int phase_finish(pfr_solver* s, SolverView& v, const pfr::ChunkOp& op, const SweepPasses& ps, const SweepSpec& sp,
                 const Chunk& c) {
  int rc;
  const int64_t Fc = s->Fc, q0 = c.q0;
  const int nv = c.nv;
  hipStream_t st = c.st;
  if (ps.correct) {
    // the forward residual walk: backward error (when checked) + the correction's dot products, then the corrected
    // fr (the CPX form reads the solve's H in h0), its loss terms and the per-frequency cotangent scales
    run_walk(s, v, op, Walk::correction(c.rd, s->X, s->XA, ps.check_fwd_walk, q0, ps.cwalk), nv, st);
    if (ps.scorr) pfr::launch_rhs_dot(s->rhs_sup, s->rhs_val, s->n_rhs_sup, s->XA, Fc, s->tq, st);
    pfr::launch_correct_finish(sp.resp.cpx ? seeded(s, c.fa) : c.fa, s->fr0, s->cpart, pfr::residual_parts(s->n), Fc, nv,
                               q0, sp.fr(), s->loss_terms, s->mscale, op, st, ps.refine_adj ? s->gind : nullptr,
                               ps.scorr ? s->tq : nullptr);
  }
  if (ps.refine_adj) {
    // the listed groups (largest first-order fr error estimates above the tolerance, at most REFINE_CAP; there the
    // unrefined solves' first-order error dominates the gradient):
    // mu += A^-T (G - A^T mu) with the fr seed G = d fr / d x of THIS x (k_functional seed mode; the adjoint
    // was solved for the seed of the bottom-up dot products, whose rounding differs), then their correction
    // dot products and gradient contraction again with the refined mu, and their fr / m_q
    pfr::launch_select_groups(s->gind, (int)(Fc / 64), s->refine_tol, s->glist, st);
    if (!s->Gx) {
      if ((rc = s->alloc(&s->Gx, s->ws.nvec))) return rc;
      HIP_TRY(hipMemsetAsync(s->Gx, 0, (size_t)s->n * Fc * 16, st));   // only the support rows are ever written
    }
    pfr::launch_functional(seeded(s, c.fa), s->X, Fc, nv, q0, nullptr, nullptr, s->Gx, st);
    run_walk(s, v, op, Walk::residual(Walk::ADJOINT, pfr::RHS_VECTOR, rhs_vector(s->Gx), s->XA, s->XR).on_groups(s->glist),
             nv, st);
    if ((rc = adjoint_solve(s, v, op, rhs_vector(s->XR), s->Y2, st, pfr::REACH_ALL, s->glist))) return rc;
    pfr::launch_axpy_vec(s->XA, s->Y2, (int64_t)s->n * Fc, st, s->glist, Fc);
    run_walk(s, v, op, Walk::correction(c.rd, s->X, s->XA, false, q0, true).on_groups(s->glist), nv, st);
    if (ps.scorr) pfr::launch_rhs_dot(s->rhs_sup, s->rhs_val, s->n_rhs_sup, s->XA, Fc, s->tq, st);
    pfr::launch_correct_finish(c.fa, s->fr0, s->cpart, pfr::residual_parts(s->n), Fc, nv, q0, sp.fr(), s->loss_terms,
                               s->mscale, op, st, nullptr, ps.scorr ? s->tq : nullptr);
  }
  const double2* msc = ps.correct ? s->mscale : nullptr;
  if (ps.jac) {
    // the walk's kpart is final here (the refined groups redone above); without the walk k_contract_q forms it
    if (!ps.cwalk && sp.jc) pfr::launch_contract_q(s->d_uent, s->n_uent, s->d_se, s->n_stiff, s->XA, s->X, s->n, Fc, s->kpart, st);
  } else if (ps.cwalk)
    pfr::launch_reduce_q(s->kpart, pfr::residual_parts(s->n), s->n_stiff, msc, nv, Fc, s->partial, st);
  else if (ps.reverse)
    pfr::launch_contract_eg(s->d_uent, s->n_uent, s->d_se, s->n_stiff, s->XA, s->X, Fc, nv, s->partial, st, msc);
  // the checks as row / column walks of the original pattern (k_residual)
  if (ps.check_fwd_after) run_walk(s, v, op, Walk::checked(Walk::FORWARD, pfr::RHS_OPERATOR, c.rd, s->X, q0), nv, st);
  if (ps.check_adj)
    run_walk(s, v, op, Walk::checked(Walk::ADJOINT, pfr::RHS_VECTOR, rhs_vector(s->G), s->XA, q0), nv, st);
  if (ps.reverse) {
    if (!ps.scorr) pfr::launch_rhs_dot(s->rhs_sup, s->rhs_val, s->n_rhs_sup, s->XA, Fc, s->tq, st, msc);
    if (ps.jac && sp.jc)
      pfr::launch_jac_finish(s->kpart, ps.cwalk ? pfr::residual_parts(s->n) : pfr::contract_q_parts(s->n, s->n_uent),
                             s->n_stiff, msc, s->tq, s->e, nv, Fc, sp.jc + q0 * s->n_stiff, st);
    // the inertia rows from the same x, mu, m_q and t_q; their partials take kpart's place once it has been read
    if (ps.jac && sp.jm)
      pfr::launch_inertia_rows(v.d_mlist, v.d_mptr, s->d_uent, s->n_uent, s->d_me, s->n_mass, s->XA, s->X, s->n, Fc,
                               s->kpart, msc, s->tq, s->freqs, s->mass_d, nv, sp.jm + q0 * s->n_mass, st);
    if (!ps.jac)
      pfr::launch_reduce(s->partial, ps.cwalk ? (int)(Fc / 64) : pfr::contract_eg_parts(s->n_uent), s->n_stiff, s->tq,
                         s->e, s->loss_terms, nv, Fc, reinterpret_cast<double2*>(sp.w), sp.loss, st);
  }
  return PFR_OK;
}

// The launches of one sweep (an entry point after its checks), direct or under stream capture
int sweep_launches(pfr_solver* s, const SweepSpec& sp, hipStream_t st) {
  const SweepPasses ps = sweep_passes(s, sp);
  reset_timing(s);
  const int64_t Fc = s->Fc;
  SolverView& v = begin_on_view(s, ps.pruned, st);
  s->last_adj = ps.adj;
  s->last_reach = ps.adj_reach;
  s->last_st = st;
  int rc;
  // buffers and row lists allocated on first use (never under capture: a sweep's first run is direct)
  if (ps.fn_fast && (rc = fn_setup(s, v))) return rc;
  if (sp.resp.cpx && ps.correct && !s->h0 && (rc = s->alloc(&s->h0, Fc))) return rc;
  if ((ps.cwalk || ps.jac) && !s->kpart && (rc = s->alloc(&s->kpart, s->ws.kpart))) return rc;
  if (ps.floss && sp.floss.loss_type != PFR_LOSS_FCOTANGENT) {
    const int64_t need = pfr::field_loss_parts(sp.floss.loss_type, sp.floss.n_sel, Fc);
    if (need > s->fpart_cap) {
      // a larger request than any before: the new block first (a failure leaves the old block and its capacity in
      // place), then the old one freed once the launches that read it are done
      double* grown = nullptr;
      HIP_TRY(hipMalloc(&grown, (size_t)need * sizeof(double)));
      if (s->fpart) {
        (void)hipDeviceSynchronize();
        s->owned.erase(std::remove(s->owned.begin(), s->owned.end(), (void*)s->fpart), s->owned.end());
        (void)hipFree(s->fpart);
      }
      s->owned.push_back(grown);
      s->fpart = grown;
      s->fpart_cap = need;
    }
    if (!s->fseed && (rc = s->alloc(&s->fseed, 3 * Fc))) return rc;
  }
  const bool used[5] = {true, true, true, ps.adj, ps.adj || ps.field};
  Chunk c{.st = st, .fa = functional_args(s, sp)};
  for (c.q0 = 0; c.q0 < sp.nfreq; c.q0 += Fc) {
    c.nv = (int)std::min<int64_t>(Fc, sp.nfreq - c.q0);
    if (sp.fresh && c.q0 == 0)      // the caller's outputs initialised here (pfr_sweep_fresh)
      pfr::launch_chunk_start(s->freqs, sp.freqs + c.q0, c.nv, Fc, s->flags, st, sp.loss, sp.w,
                              ps.reverse && sp.w ? 2 * s->n_stiff : 0, sp.flags, s->berr_out, sp.nfreq);
    else
      pfr::launch_chunk_start(s->freqs, sp.freqs + c.q0, c.nv, Fc, s->flags, st);
    if ((rc = begin_chunk(s))) return rc;
    record(s, 0, st);
    const pfr::ChunkOp op = chunk_op(s, sp.popK, sp.pop.member ? &sp.pop : nullptr, c.q0);
    s->last_op = op;
    s->comp_done = false;
    c.rd = rhs_operator(op);
    if ((rc = phase_factor(s, v, op, ps, sp, c))) return rc;
    record(s, 1, st);
    if ((rc = phase_forward(s, v, op, ps, sp, c))) return rc;
    record(s, 2, st);
    if (ps.functional) phase_functional(s, v, op, ps, sp, c);
    record(s, 3, st);
    if (ps.adj && (rc = phase_adjoint(s, v, op, ps, sp, c))) return rc;
    record(s, 4, st);
    if (ps.adj && (rc = phase_finish(s, v, op, ps, sp, c))) return rc;
    // the way out of a field sweep, before the next chunk overwrites X (timed as the last phase, otherwise empty here)
    if (ps.field)
      pfr::launch_field_gather(sp.field.sel, sp.field.n_sel, s->X, Fc, c.nv, sp.field.out + c.q0 * sp.field.n_sel, st);
    record(s, 5, st);
    if (sp.flags) pfr::launch_flags_merge(s->flags, c.nv, sp.flags + c.q0, st);
    LAUNCH_TRY();
    if ((rc = finish_timing(s, used))) return rc;
  }
  return PFR_OK;
}

template <class T>
uint64_t key_bits(T v) {
  uint64_t b = 0;
  static_assert(sizeof(T) <= sizeof(b), "key word");
  std::memcpy(&b, &v, sizeof(T));
  return b;
}

// The state a sweep needs, refused in this order: the operator (own_K, a population sweep: the mass matrix alone), the
// rhs, the functional and -- no_stiff != NULL: the refusal's text -- the stiffness matrices
int sweep_ready(const pfr_solver* s, const char* no_stiff = nullptr, bool own_K = false) {
  if (!own_K && (!s->K || !s->M)) return fail(PFR_ERR_STATE, "operator not set (pfr_set_operator)");
  if (own_K && !s->M) return fail(PFR_ERR_STATE, "mass matrix not set (pfr_set_operator)");
  if (!s->has_rhs) return fail(PFR_ERR_STATE, "rhs not set (pfr_set_rhs)");
  if (!s->has_fn) return fail(PFR_ERR_STATE, "functional not set (pfr_set_functional)");
  if (no_stiff && !s->stiff) return fail(PFR_ERR_STATE, no_stiff);
  return PFR_OK;
}

// a sweep that is never captured, and the loss sweeps' graph is not replayed past it: the next loss sweep runs directly
void never_captured(pfr_solver* s) { s->drop_graph(), s->gkey_valid = false; }

int sweep_impl(pfr_solver* s, int32_t nfreq, const double* freqs_dev, int32_t loss_type, const double* ref_dev,
               double scale, double* fr_dev, double* loss_dev, double* w_dev, int32_t* flags_dev, void* stream,
               bool fresh) {
  if (!s || nfreq <= 0 || !freqs_dev) return fail(PFR_ERR_ARG, "bad sweep arguments");
  if (int rc = sweep_ready(s)) return rc;
  const bool reverse = loss_type != PFR_LOSS_NONE;
  if (reverse && (loss_type < 0 || loss_type > PFR_LOSS_COTANGENT || !ref_dev))
    return fail(PFR_ERR_ARG, "bad loss type / missing ref");
  if (reverse && (!s->stiff || !w_dev)) return fail(PFR_ERR_STATE, "reverse pass needs pfr_set_stiffness and w_dev");
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  const SweepSpec sp{.nfreq = nfreq, .freqs = freqs_dev, .loss_type = loss_type, .ref = ref_dev, .scale = scale,
                     .response = fr_dev, .loss = loss_dev, .w = w_dev, .flags = flags_dev, .fresh = fresh};
  // per-launch timing events are host work between the launches: never under a graph
  if (!s->graph_mode || s->graph_off || s->timing) return sweep_launches(s, sp, st);
  const std::array<uint64_t, 14> key = {
      s->gen * 2 + (sp.fresh ? 1 : 0), key_bits(s->check_mode), key_bits(s->check_tol), key_bits(s->berr_out),
      key_bits(sp.nfreq), key_bits(sp.freqs), key_bits(sp.loss_type), key_bits(sp.ref), key_bits(sp.scale),
      key_bits(sp.response), key_bits(sp.loss), key_bits(sp.w), key_bits(sp.flags), key_bits(st)};
  if (!s->gkey_valid || key != s->gkey) {
    // a new sweep configuration: run it directly (its first run also makes the lazy allocations and uploads,
    // which a capture must not contain); the same configuration again is captured
    s->drop_graph();
    s->gkey = key;
    s->gkey_valid = true;
    return sweep_launches(s, sp, st);
  }
  if (!s->gexec) {
    hipGraph_t g = nullptr;
    HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = sweep_launches(s, sp, st);
    const hipError_t e = hipStreamEndCapture(st, &g);
    hipGraphExec_t x = nullptr;
    if (rc == PFR_OK && e == hipSuccess && g && hipGraphInstantiate(&x, g, nullptr, nullptr, 0) == hipSuccess) {
      s->graph = g;
      s->gexec = x;
    } else {
      // nothing of the captured work ran: no graphs on this solver from now on, and this sweep directly
      if (g) (void)hipGraphDestroy(g);
      (void)hipGetLastError();
      s->graph_off = true;
      return sweep_launches(s, sp, st);
    }
  }
  s->comp_done = false;
  HIP_TRY(hipGraphLaunch(s->gexec, st));
  ++s->graph_launches;
  return PFR_OK;
}

// the argument checks the two complex sweeps share; then never captured, on the solver's device
int complex_sweep_begin(pfr_solver* s, int32_t nfreq, const double* freqs_dev, const double* axis, bool reverse,
                        Response* resp) {
  if (!s || nfreq <= 0 || !freqs_dev || !axis) return fail(PFR_ERR_ARG, "bad complex sweep arguments");
  if (!(std::isfinite(axis[0]) && std::isfinite(axis[1]) && std::isfinite(axis[2])) ||
      (axis[0] == 0.0 && axis[1] == 0.0 && axis[2] == 0.0))
    return fail(PFR_ERR_ARG, "sensing axis zero or not finite");
  if (s->check_mode & PFR_CHECK_REFINE_ADJ)
    return fail(PFR_ERR_ARG, "PFR_CHECK_REFINE_ADJ does not apply to the complex response");
  if (int rc = sweep_ready(s, reverse ? "reverse pass needs pfr_set_stiffness" : nullptr)) return rc;
  resp->cpx = true;
  std::copy(axis, axis + 3, resp->axis);
  never_captured(s);
  HIP_TRY(hipSetDevice(s->device));
  return PFR_OK;
}
}  // namespace

extern "C" {

int pfr_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev, int32_t loss_type, const double* ref_dev,
              double scale, double* fr_dev, double* loss_dev, double* w_dev, int32_t* flags_dev, void* stream) {
  return sweep_impl(s, nfreq, freqs_dev, loss_type, ref_dev, scale, fr_dev, loss_dev, w_dev, flags_dev, stream, false);
}

int pfr_sweep_fresh(pfr_solver* s, int32_t nfreq, const double* freqs_dev, int32_t loss_type, const double* ref_dev,
                    double scale, double* fr_dev, double* loss_dev, double* w_dev, int32_t* flags_dev, void* stream) {
  return sweep_impl(s, nfreq, freqs_dev, loss_type, ref_dev, scale, fr_dev, loss_dev, w_dev, flags_dev, stream, true);
}

int64_t pfr_sweep_graph_launches(const pfr_solver* s) { return s ? s->graph_launches : 0; }

int pfr_jacobian_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev, double* fr_dev, double* jc_dev,
                       int32_t* flags_dev, void* stream) {
  if (!s || nfreq <= 0 || !freqs_dev || !jc_dev) return fail(PFR_ERR_ARG, "bad jacobian sweep arguments");
  if (int rc = sweep_ready(s, "jacobian sweep needs pfr_set_stiffness")) return rc;
  never_captured(s);
  HIP_TRY(hipSetDevice(s->device));
  const SweepSpec sp{.nfreq = nfreq, .freqs = freqs_dev, .loss_type = pfr::LOSS_UNIT, .response = fr_dev,
                     .jc = reinterpret_cast<double2*>(jc_dev), .flags = flags_dev};
  return sweep_launches(s, sp, (hipStream_t)stream);
}

int pfr_sweep_complex(pfr_solver* s, int32_t nfreq, const double* freqs_dev, const double* axis, int32_t loss_type,
                      const double* ref_dev, double scale, double* h_dev, double* loss_dev, double* w_dev,
                      int32_t* flags_dev, int32_t fresh, void* stream) {
  const bool reverse = loss_type != PFR_LOSS_NONE;
  if (reverse && (loss_type < PFR_LOSS_CMSE || loss_type > PFR_LOSS_CCOTANGENT || !ref_dev))
    return fail(PFR_ERR_ARG, "bad complex loss type / missing ref");
  if (reverse && s && !w_dev) return fail(PFR_ERR_STATE, "reverse pass needs w_dev");
  Response resp;
  if (int rc = complex_sweep_begin(s, nfreq, freqs_dev, axis, reverse, &resp)) return rc;
  const SweepSpec sp{.nfreq = nfreq, .freqs = freqs_dev, .loss_type = loss_type, .ref = ref_dev, .scale = scale,
                     .response = h_dev, .loss = loss_dev, .w = w_dev, .flags = flags_dev, .fresh = fresh != 0, .resp = resp};
  return sweep_launches(s, sp, (hipStream_t)stream);
}

int pfr_jacobian_sweep_complex(pfr_solver* s, int32_t nfreq, const double* freqs_dev, const double* axis, double* h_dev,
                               double* jc_dev, int32_t* flags_dev, void* stream) {
  if (!jc_dev) return fail(PFR_ERR_ARG, "bad jacobian sweep arguments");
  Response resp;
  if (int rc = complex_sweep_begin(s, nfreq, freqs_dev, axis, true, &resp)) return rc;
  const SweepSpec sp{.nfreq = nfreq, .freqs = freqs_dev, .loss_type = pfr::LOSS_UNIT, .response = h_dev,
                     .jc = reinterpret_cast<double2*>(jc_dev), .flags = flags_dev, .resp = resp};
  return sweep_launches(s, sp, (hipStream_t)stream);
}

int pfr_inertia_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev, const double* axis, double* resp_dev,
                      double* jc_dev, double* jm_dev, int32_t* flags_dev, void* stream) {
  if (!s || nfreq <= 0 || !freqs_dev || !jm_dev) return fail(PFR_ERR_ARG, "bad inertia sweep arguments");
  Response resp;
  if (axis) {
    if (int rc = complex_sweep_begin(s, nfreq, freqs_dev, axis, jc_dev != nullptr, &resp)) return rc;
  } else if (int rc = sweep_ready(s, jc_dev ? "jacobian rows need pfr_set_stiffness" : nullptr)) {
    return rc;
  }
  if (!s->mass) return fail(PFR_ERR_STATE, "inertia sweep needs pfr_set_inertia");
  never_captured(s);
  HIP_TRY(hipSetDevice(s->device));
  const SweepSpec sp{.nfreq = nfreq, .freqs = freqs_dev, .loss_type = pfr::LOSS_UNIT, .response = resp_dev,
                     .jc = reinterpret_cast<double2*>(jc_dev), .jm = reinterpret_cast<double2*>(jm_dev),
                     .flags = flags_dev, .resp = resp};
  return sweep_launches(s, sp, (hipStream_t)stream);
}

int32_t pfr_field_tile_rows(void) { return pfr::FIELD_R; }

int pfr_field_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev, int32_t n_rows, const int32_t* rows,
                    double* out_dev, double* fr_dev, int32_t* flags_dev, void* stream) {
  if (!s || nfreq <= 0 || !freqs_dev || !out_dev) return fail(PFR_ERR_ARG, "bad field sweep arguments");
  std::vector<int32_t> sel;
  if (rows) {
    const std::string refusal = pfr::field_rows(s->iperm, n_rows, rows, sel);
    if (!refusal.empty()) return fail(PFR_ERR_ARG, refusal);
  }
  if (int rc = sweep_ready(s)) return rc;
  never_captured(s);
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  // every row: the full view's walk list is iperm, on the device already.  That holds because the solver's own view
  // covers every front (upload_view writes -1 only for rows of fronts outside a view; pruned views are s->act /
  // s->comp, never *s): a full view that skipped rows would need its own list here, the gather reads X[sel[j] * Fc + q]
  FieldOut field{.out = reinterpret_cast<double2*>(out_dev), .sel = s->d_walk, .n_sel = s->n};
  if (rows) {
    void* d_sel = nullptr;
    if (int rc = stage_upload(s, 2, sel.data(), sel.size() * sizeof(int32_t), &d_sel, st)) return rc;
    field.sel = static_cast<const int32_t*>(d_sel);
    field.n_sel = (int32_t)sel.size();
  }
  const SweepSpec sp{.nfreq = nfreq, .freqs = freqs_dev, .response = fr_dev, .flags = flags_dev, .field = field,
                     .check_mask = PFR_CHECK_FORWARD | PFR_CHECK_REFINE};
  return sweep_launches(s, sp, st);
}

int pfr_field_loss_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev, int32_t n_rows, const int32_t* rows,
                         const double* weights, int32_t loss_type, const double* ref_dev, double scale, double* out_dev,
                         double* loss_dev, double* w_dev, int32_t* flags_dev, int32_t fresh, void* stream) {
  if (!s || nfreq <= 0 || !freqs_dev || !ref_dev || !w_dev) return fail(PFR_ERR_ARG, "bad field loss sweep arguments");
  if (loss_type < PFR_LOSS_FMSE || loss_type > PFR_LOSS_FCOTANGENT) return fail(PFR_ERR_ARG, "bad field loss type");
  const bool cot = loss_type == PFR_LOSS_FCOTANGENT;
  if (!cot && !loss_dev) return fail(PFR_ERR_ARG, "field loss sweep: a loss term needs loss_dev");
  std::vector<int32_t> sel;
  const std::string refusal = pfr::field_loss_rows(s->iperm, n_rows, rows, weights, cot, sel);
  if (!refusal.empty()) return fail(PFR_ERR_ARG, refusal);
  if (int rc = sweep_ready(s, "reverse pass needs pfr_set_stiffness")) return rc;
  never_captured(s);
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  // all rows: the full view's walk list is iperm, on the device already (pfr_field_sweep)
  pfr::FieldLossArgs fl{.loss_type = loss_type, .sel = s->d_walk, .n_sel = rows ? (int32_t)sel.size() : s->n,
                        .ref = reinterpret_cast<const double2*>(ref_dev), .scale = scale};
  if (rows || weights) {
    // one staged block: the weights (8-byte entries first), then the selection
    const size_t wb = weights ? (size_t)fl.n_sel * sizeof(double) : 0, sb = sel.size() * sizeof(int32_t);
    std::vector<char> block(wb + sb);
    if (wb) std::memcpy(block.data(), weights, wb);
    if (sb) std::memcpy(block.data() + wb, sel.data(), sb);
    void* d_block = nullptr;
    if (int rc = stage_upload(s, 2, block.data(), block.size(), &d_block, st)) return rc;
    if (wb) fl.wts = static_cast<const double*>(d_block);
    if (sb) fl.sel = reinterpret_cast<const int32_t*>(static_cast<const char*>(d_block) + wb);
  }
  const FieldOut field{.out = reinterpret_cast<double2*>(out_dev), .sel = fl.sel, .n_sel = fl.n_sel};
  const SweepSpec sp{.nfreq = nfreq, .freqs = freqs_dev, .loss_type = loss_type, .scale = scale,
                     .loss = cot ? nullptr : loss_dev, .w = w_dev, .flags = flags_dev, .fresh = fresh != 0,
                     .field = field, .floss = fl,
                     .check_mask = PFR_CHECK_FORWARD | PFR_CHECK_ADJOINT | PFR_CHECK_REFINE};
  return sweep_launches(s, sp, st);
}

int pfr_combine_batch(pfr_solver* s, int32_t n_members, const double* coef, double* Kpop_dev, void* stream) {
  if (!s || n_members <= 0 || !coef || !Kpop_dev) return fail(PFR_ERR_ARG, "bad combine batch arguments");
  if (!s->stiff) return fail(PFR_ERR_STATE, "pfr_set_stiffness not called");
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  void* d_coef = nullptr;
  if (int rc = stage_upload(s, 0, coef, (size_t)n_members * s->n_stiff * 16, &d_coef, st)) return rc;
  pfr::launch_combine_batch(s->stiff, s->n_stiff, s->nnz, static_cast<const double2*>(d_coef), n_members,
                            reinterpret_cast<double2*>(Kpop_dev), st);
  LAUNCH_TRY();
  return PFR_OK;
}

int pfr_population_sweep(pfr_solver* s, int32_t nlane, const double* freqs_dev, const int32_t* member,
                         int32_t n_members, const double* Kpop_dev, const double* beta, double* fr_dev,
                         double* jc_dev, int32_t* flags_dev, void* stream) {
  if (!s || nlane <= 0 || !freqs_dev || !member || n_members <= 0 || !Kpop_dev || !beta || !fr_dev)
    return fail(PFR_ERR_ARG, "bad population sweep arguments");
  if (nlane % 64 != 0) return fail(PFR_ERR_ARG, "population sweep: nlane must be a multiple of 64");
  const int64_t ng = nlane / 64;
  for (int64_t g = 0; g < ng; ++g)
    if (member[g] < 0 || member[g] >= n_members) return fail(PFR_ERR_ARG, "population sweep: member index out of range");
  // ranks the groups of a chunk against each other: a member's result would depend on its neighbours
  if (s->check_mode & PFR_CHECK_REFINE_ADJ)
    return fail(PFR_ERR_ARG, "population sweep: PFR_CHECK_REFINE_ADJ is not supported");
  if (int rc = sweep_ready(s, jc_dev ? "population jacobian sweep needs pfr_set_stiffness" : nullptr, true)) return rc;
  never_captured(s);
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  // the group table padded to whole chunks (the lanes past nlane of a short last chunk run too, on repeated
  // frequencies: their groups take the last member), then the members' beta, 16-byte aligned
  const int64_t gc = s->Fc / 64, ngp = (ng + gc - 1) / gc * gc;
  const size_t off_beta = (size_t)((ngp * 4 + 15) / 16 * 16);
  std::vector<char> tab(off_beta + (size_t)n_members * 16, 0);
  int32_t* tm = reinterpret_cast<int32_t*>(tab.data());
  for (int64_t g = 0; g < ngp; ++g) tm[g] = member[std::min(g, ng - 1)];
  std::memcpy(tab.data() + off_beta, beta, (size_t)n_members * 16);
  void* d_tab = nullptr;
  if (int rc = stage_upload(s, 1, tab.data(), tab.size(), &d_tab, st)) return rc;
  const double2* d_beta = reinterpret_cast<const double2*>(static_cast<const char*>(d_tab) + off_beta);
  const SweepSpec sp{.nfreq = nlane, .freqs = freqs_dev, .loss_type = jc_dev ? pfr::LOSS_UNIT : PFR_LOSS_NONE,
                     .response = fr_dev, .jc = reinterpret_cast<double2*>(jc_dev), .flags = flags_dev,
                     .popK = reinterpret_cast<const double2*>(Kpop_dev),
                     .pop = {.member = static_cast<const int32_t*>(d_tab), .beta = d_beta, .nnz = s->nnz}};
  return sweep_launches(s, sp, st);
}

int pfr_stream_order(void* waiter, void* signaller) {
  // one event per (thread, device), recorded again for every ordering: a wait takes the event's state at the time
  // of the hipStreamWaitEvent call, so a later record does not move an earlier wait
  thread_local std::vector<hipEvent_t> evs;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if ((int)evs.size() <= dev) evs.resize(dev + 1, nullptr);
  if (!evs[dev]) HIP_TRY(hipEventCreateWithFlags(&evs[dev], hipEventDisableTiming));
  HIP_TRY(hipEventRecord(evs[dev], (hipStream_t)signaller));
  HIP_TRY(hipStreamWaitEvent((hipStream_t)waiter, evs[dev], 0));
  return PFR_OK;
}

int pfr_hessian_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev, int32_t loss_type, const double* ref_dev,
                      double scale, int32_t n_dir, const double* dcoef, double* loss_dev, double* w_dev,
                      double* h_dev, int32_t* flags_dev, void* stream) {
  if (!s || nfreq <= 0 || !freqs_dev || !ref_dev || !w_dev || !h_dev || n_dir <= 0 || !dcoef)
    return fail(PFR_ERR_ARG, "bad hessian sweep arguments");
  ++s->gen;
  if (loss_type < PFR_LOSS_MSE || loss_type > PFR_LOSS_MSE_LOG_AFC)
    return fail(PFR_ERR_ARG, "hessian sweep needs a loss type (MSE, RMSE, MSE_AFC, MSE_LOG_AFC)");
  if (int rc0 = sweep_ready(s, "pfr_set_stiffness not called")) return rc0;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  reset_timing(s);
  const int64_t Fc = s->Fc, n = s->n;
  // the tangent solves' right-hand sides are not the operator's: every front
  SolverView& v = begin_on_view(s, false, st);
  int rc;
  // the first-order part as the loss sweep's phases where they launch the same: unpaired, unrefined, unchecked
  const SweepSpec sp{.nfreq = nfreq, .freqs = freqs_dev, .loss_type = loss_type, .ref = ref_dev, .scale = scale,
                     .loss = loss_dev, .w = w_dev, .flags = flags_dev};
  const SweepPasses ps{.reverse = true, .correct = (s->check_mode & PFR_CHECK_CORRECT) != 0, .adj = true};
  Chunk ck{.st = st, .fa = functional_args(s, sp)};
  if (!s->DX && ((rc = s->alloc(&s->DX, n * Fc)) || (rc = s->alloc(&s->DL, n * Fc)))) return rc;
  if (s->n_kdir < n_dir) {
    if ((rc = s->alloc(&s->Kdir, (int64_t)n_dir * s->nnz))) return rc;   // previous block stays owned
    s->n_kdir = n_dir;
  }
  // tangent operators dA_i = sum_k dc_ik S_k and right-hand-side weights beta_i = sum_k dc_ik e_k
  std::vector<double2> beta(n_dir);
  pfr::CoefPack zero{};
  for (int i = 0; i < n_dir; ++i) {
    pfr::CoefPack c{};
    double br = 0, bi = 0;
    for (int k = 0; k < s->n_stiff; ++k) {
      c.re[k] = dcoef[2 * (i * s->n_stiff + k)];
      c.im[k] = dcoef[2 * (i * s->n_stiff + k) + 1];
      br += c.re[k] * s->e.re[k];
      bi += c.im[k] * s->e.re[k];
    }
    beta[i] = make_double2(br, bi);
    pfr::launch_combine(s->stiff, s->n_stiff, s->nnz, c, s->Kdir + (int64_t)i * s->nnz, st);
  }
  double2* H = reinterpret_cast<double2*>(h_dev);
  for (int64_t& q0 = ck.q0; q0 < nfreq; q0 += Fc) {
    const int nv = ck.nv = (int)std::min<int64_t>(Fc, nfreq - q0);
    pfr::launch_chunk_start(s->freqs, freqs_dev + q0, nv, Fc, s->flags, st);
    const pfr::ChunkOp op = chunk_op(s);
    ck.rd = rhs_operator(op);
    // factorisation, forward solve, loss, adjoint, gradient partials
    if ((rc = phase_factor(s, v, op, ps, sp, ck)) || (rc = phase_forward(s, v, op, ps, sp, ck))) return rc;
    HIP_TRY(hipMemsetAsync(s->G, 0, (size_t)n * Fc * 16, st));
    const pfr::RhsArgs rg = rhs_vector(s->G);
    // with the correction the seed mode, as pfr_sweep: the adjoint of fr, the corrected fr's loss terms and cotangent
    // scales, then lambda = m_q mu in place -- loss and gradient equal the corrected loss sweep's
    pfr::launch_functional(ps.correct ? seeded(s, ck.fa) : ck.fa, s->X, Fc, nv, q0, nullptr,
                           ps.correct ? nullptr : s->loss_terms, s->G, st);
    if ((rc = phase_adjoint(s, v, op, ps, sp, ck))) return rc;
    if (ps.correct) {
      run_walk(s, v, op, Walk::correction(ck.rd, s->X, s->XA, false, q0, false), nv, st);
      // the loss sweep's cotangent, solve-error scale included (k_correct_finish): its gradient is the loss sweep's
      if (s->scale_corr) pfr::launch_rhs_dot(s->rhs_sup, s->rhs_val, s->n_rhs_sup, s->XA, Fc, s->tq, st);
      pfr::launch_correct_finish(ck.fa, s->fr0, s->cpart, pfr::residual_parts(s->n), Fc, nv, q0, nullptr, s->loss_terms,
                                 s->mscale, op, st, nullptr, s->scale_corr ? s->tq : nullptr);
      pfr::launch_scale_vec(s->XA, s->mscale, s->n, Fc, st);
      // the second-order seeds G (k_functional_tangent) are formed from fa, not the seed mode
    }
    contract_rows(s, s->XA, s->X, nv, st);
    pfr::launch_rhs_dot(s->rhs_sup, s->rhs_val, s->n_rhs_sup, s->XA, Fc, s->tq, st);
    pfr::launch_reduce(s->partial, pfr::contract_eg_parts(s->n_uent), s->n_stiff, s->tq, s->e, s->loss_terms, nv, Fc,
                       reinterpret_cast<double2*>(w_dev), loss_dev, st);
    // second order, per direction i (same factors):
    //   A dx_i = db_i - dA_i x ;  A^T dl_i = dG_i(dx_i) - dA_i^T l
    //   h_ki += sum_q [ -dl_i^T S_k x + e_k dl_i^T b0 - l^T S_k dx_i ]
    for (int i = 0; i < n_dir; ++i) {
      const double2* Kd = s->Kdir + (int64_t)i * s->nnz;
      pfr::launch_tangent_spmv(s->d_rptr, s->d_ridx, s->d_rnz, (int)n, Kd, s->X, Fc, s->rhsP, beta[i], s->G, 0, st);
      if ((rc = forward_solve(s, v, op, pfr::RHS_VECTOR, rg, s->DX, st))) return rc;
      HIP_TRY(hipMemsetAsync(s->G, 0, (size_t)n * Fc * 16, st));
      pfr::launch_functional_tangent(ck.fa, s->X, s->DX, Fc, nv, q0, s->G, st);
      pfr::launch_tangent_spmv(s->d_cptr, s->d_cidx, s->d_cnz, (int)n, Kd, s->XA, Fc, nullptr, make_double2(0, 0),
                               s->G, 1, st);
      if ((rc = adjoint_solve(s, v, op, rg, s->DL, st))) return rc;
      contract_rows(s, s->DL, s->X, nv, st);
      pfr::launch_rhs_dot(s->rhs_sup, s->rhs_val, s->n_rhs_sup, s->DL, Fc, s->tq, st);
      pfr::launch_reduce(s->partial, pfr::contract_eg_parts(s->n_uent), s->n_stiff, s->tq, s->e, s->loss_terms, nv, Fc,
                         H + (int64_t)i * s->n_stiff, nullptr, st);
      contract_rows(s, s->XA, s->DX, nv, st);
      pfr::launch_reduce(s->partial, pfr::contract_eg_parts(s->n_uent), s->n_stiff, s->tq, zero, s->loss_terms, nv, Fc,
                         H + (int64_t)i * s->n_stiff, nullptr, st);
    }
    if (flags_dev) pfr::launch_flags_merge(s->flags, nv, flags_dev + q0, st);
    LAUNCH_TRY();
  }
  return PFR_OK;
}

int pfr_solve_multi(pfr_solver* s, int32_t batch, int32_t nrhs, const double* data_dev, int64_t data_stride,
                    const double* b_dev, int64_t b_stride, int64_t b_rhs_stride, double* x_dev, int64_t x_rhs_stride,
                    int32_t transpose, int32_t* flags_dev, void* stream) {
  if (!s || batch <= 0 || nrhs <= 0 || !data_dev || !b_dev || !x_dev || data_stride < 0 || b_stride < 0 ||
      b_rhs_stride < 0 || x_rhs_stride < 0)
    return fail(PFR_ERR_ARG, "bad solve arguments");
  ++s->gen;
  if (data_stride != 0 && data_stride < s->nnz) return fail(PFR_ERR_ARG, "data_stride < nnz");
  if (b_stride != 0 && b_stride < s->n) return fail(PFR_ERR_ARG, "b_stride < n");
  if (nrhs > 1 && x_rhs_stride < (int64_t)batch * s->n) return fail(PFR_ERR_ARG, "x_rhs_stride < batch * n");
  if (s->sym)
    return fail(PFR_ERR_STATE, "explicit-matrix solves need a solver on a general analysis (symmetric = 0)");
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  reset_timing(s);
  const int64_t Fc = s->Fc;
  // a caller's matrices: every front (a general analysis: no view exists; kept right should that ever change)
  SolverView& v = begin_on_view(s, false, st);
  const double2* data = reinterpret_cast<const double2*>(data_dev);
  const double2* B = reinterpret_cast<const double2*>(b_dev);
  double2* Xo = reinterpret_cast<double2*>(x_dev);
  bool used[5] = {true, !transpose, false, (bool)transpose, false};
  for (int64_t q0 = 0; q0 < batch; q0 += Fc) {
    const int nv = (int)std::min<int64_t>(Fc, batch - q0);
    HIP_TRY(hipMemsetAsync(s->flags, 0, Fc * sizeof(int32_t), st));
    if (int rc0 = begin_chunk(s)) return rc0;
    record(s, 0, st);
    // padded lanes repeat the last valid item (stride 0 broadcast handled by the kernel's clamp)
    const pfr::ChunkOp op = chunk_op(s);   // explicit matrices: K and the rhs may be unset, none of it is read
    int rc = factor_all(s, v, op, pfr::MAT_BATCH, data + q0 * data_stride, data_stride, nv, st);
    if (rc) return rc;
    record(s, 1, st);
    // every right-hand side of the chunk on the same factors (reference mode 4
    // refactorises per right-hand side, InnerState.h:289-305)
    for (int32_t r = 0; r < nrhs; ++r) {
      const pfr::RhsArgs rd{.B = B + r * b_rhs_stride + q0 * b_stride, .b_stride = b_stride, .nvalid = nv};
      const pfr::Tri up = transpose ? pfr::TRI_UT : pfr::TRI_L, down = transpose ? pfr::TRI_LT : pfr::TRI_U;
      const auto solve = [&] {   // the bottom-up and the top-down pass of the system solved: L, U or U^T, L^T
        const int e = solve_all(s, v, op, up, pfr::RHS_BATCH, rd, nullptr, s->Y, st);
        return e ? e : solve_all(s, v, op, down, pfr::RHS_BATCH, rd, s->Y, s->X, st);
      };
      if (!transpose && (rc = solve())) return rc;
      if (r == 0) {
        record(s, 2, st);
        record(s, 3, st);
      }
      if (transpose && (rc = solve())) return rc;
      const Walk::Sys which = transpose ? Walk::ADJOINT : Walk::FORWARD;
      const double2* dq = data + q0 * data_stride;
      if (s->check_mode & PFR_CHECK_REFINE) {
        // x += A^{-1} (b - A x) (or the transposed system) on the same factors
        run_walk(s, v, op, Walk::residual(which, pfr::RHS_BATCH, rd, s->X, s->G).on_batch(dq, data_stride), nv, st);
        const pfr::RhsArgs rr = rhs_vector(s->G);
        if ((rc = solve_all(s, v, op, up, pfr::RHS_VECTOR, rr, nullptr, s->Y, st))) return rc;
        if ((rc = solve_all(s, v, op, down, pfr::RHS_OPERATOR, rr, s->Y, s->XA, st))) return rc;
        pfr::launch_axpy_vec(s->X, s->XA, (int64_t)s->n * Fc, st);
      }
      if (s->check_mode & (transpose ? PFR_CHECK_ADJOINT : PFR_CHECK_FORWARD))
        run_walk(s, v, op, Walk::checked(which, pfr::RHS_BATCH, rd, s->X, r == 0 ? q0 : -1).on_batch(dq, data_stride), nv, st);
      pfr::launch_unpermute(s->P.perm, s->n, s->X, Fc, nv, Xo + r * x_rhs_stride + q0 * s->n, st);
    }
    record(s, 4, st);
    record(s, 5, st);
    if (flags_dev) pfr::launch_flags_merge(s->flags, nv, flags_dev + q0, st);
    LAUNCH_TRY();
    if ((rc = finish_timing(s, used))) return rc;
  }
  return PFR_OK;
}

int pfr_solve(pfr_solver* s, int32_t batch, const double* data_dev, int64_t data_stride, const double* b_dev,
              int64_t b_stride, double* x_dev, int32_t transpose, int32_t* flags_dev, void* stream) {
  return pfr_solve_multi(s, batch, 1, data_dev, data_stride, b_dev, b_stride, 0, x_dev, 0, transpose, flags_dev,
                         stream);
}

int pfr_matvec(pfr_solver* s, int32_t batch, const double* data_dev, int64_t data_stride, const double* x_dev,
               int64_t x_stride, double* y_dev, int32_t transpose, void* stream) {
  if (!s || batch <= 0 || !data_dev || !x_dev || !y_dev) return fail(PFR_ERR_ARG, "bad matvec arguments");
  ++s->gen;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = (hipStream_t)stream;
  if (!transpose) HIP_TRY(hipMemsetAsync(y_dev, 0, (size_t)batch * s->n * 16, st));
  pfr::launch_matvec(s->d_colptr, s->d_rowind, s->n, reinterpret_cast<const double2*>(data_dev), data_stride,
                     reinterpret_cast<const double2*>(x_dev), x_stride, reinterpret_cast<double2*>(y_dev),
                     transpose, batch, st);
  LAUNCH_TRY();
  return PFR_OK;
}

}  // extern "C"
