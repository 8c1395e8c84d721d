/*
 * pfr.h -- C ABI of the MI355X plate frequency-response solver (libpfr.so).
 *
 * Drop-in boundary for the reference's native solver path:
 *   pybind11 class InnerState (source/jax_plate_lib/src/main.cpp:6-19) bound by
 *   SolverState (source/jax_plate/Sparse.py:19-44) and called through the JAX
 *   primitives' CPU lowering (Sparse.py:150-160, 187-197).
 *
 * Plain C: opaque handles, integer status codes (no exceptions cross the ABI),
 * plain pointers and sizes.  Complex numbers are interleaved (re, im) doubles
 * (numpy complex128 / torch.complex128 memory layout).  Every *_dev pointer is
 * a device (HBM) pointer; `stream` is a hipStream_t (NULL = default stream).
 * Host pointers are only read during the call.
 */
#ifndef PFR_H
#define PFR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFR_API __attribute__((visibility("default")))

/* status codes */
#define PFR_OK 0
#define PFR_ERR_ARG 1        /* invalid argument (cf. Sparse.py:120-140 checks) */
#define PFR_ERR_SYMBOLIC 2   /* symbolic analysis failed (cf. umfpack_interface.h:10-18) */
#define PFR_ERR_HIP 3        /* HIP runtime error */
#define PFR_ERR_NOMEM 4      /* device allocation failed */
#define PFR_ERR_STATE 5      /* call out of order (e.g. operator not set) */

/* per-frequency status flags (bitwise OR into an int32 array) */
#define PFR_FLAG_BAD_PIVOT 1 /* zero / non-finite static pivot */
#define PFR_FLAG_BACKWARD_ERROR 2     /* forward solution: componentwise backward error above the tolerance */
#define PFR_FLAG_BACKWARD_ERROR_ADJ 4 /* adjoint solution: componentwise backward error above the tolerance */

/* pfr_set_check modes (bitwise OR) */
#define PFR_CHECK_FORWARD 1   /* backward error of the forward solution (A x = b) */
#define PFR_CHECK_ADJOINT 2   /* backward error of the adjoint solution (A^T l = g; loss sweeps, transposed solves) */
#define PFR_CHECK_REFINE 4    /* one step of iterative refinement of the forward (and, in loss sweeps, the
                               * adjoint) solution on the same factors, x += A^{-1} (b - A x), before the
                               * checks (UMFPACK refines by default, up to 2 steps) */
#define PFR_CHECK_CORRECT 8   /* functional correction (pfr_sweep): fr += Re(mu^T (b - A x)) with mu the adjoint
                               * of fr (A^T mu = d fr / d x) -- fr to second order in the solve's error, the
                               * accuracy the reference's refined UMFPACK solves give; the loss, its
                               * cotangent and the gradient are formed from the corrected fr; in loss sweeps
                               * the cotangent also carries the solve-error scale fr / (mu^T A x) (complex; the
                               * static-pivot solves' error next to a resonance is a complex multiple of the
                               * solution itself, which this divides out of the gradient contraction; env
                               * PFR_SCALE_CORR=0 turns it off) */

#define PFR_CHECK_REFINE_ADJ 16 /* selective adjoint refinement (loss sweeps with PFR_CHECK_CORRECT, symmetric
                               * mode): after the forward residual walk, the 64-frequency groups holding a frequency
                               * whose functional correction exceeds the tolerance (pfr_set_refine_tol; the
                               * first-order fr error estimate, large next to a resonance) get one refinement step
                               * of the fr adjoint, mu += A^-T (d fr / d x - A^T mu), and their gradient contraction
                               * and correction are redone with it (opt-in: with the solve-error scale of
                               * PFR_CHECK_CORRECT the gradient is already within the oracle's accuracy) */

/* loss types (Problem.py:948-975) */
#define PFR_LOSS_NONE -1
#define PFR_LOSS_MSE 0
#define PFR_LOSS_RMSE 1
#define PFR_LOSS_MSE_AFC 2
#define PFR_LOSS_MSE_LOG_AFC 3
#define PFR_LOSS_COTANGENT 4  /* ref holds dL/dfr (real part), loss not computed */
/* losses of the complex response H (pfr_sweep_complex only); g is the cotangent, d term = Re(g dH) */
#define PFR_LOSS_CMSE 16        /* |H - ref|^2,            g = 2 conj(H - ref) */
#define PFR_LOSS_CRMSE 17       /* |H - ref|^2 / |ref|^2,  g = 2 conj(H - ref) / |ref|^2 */
#define PFR_LOSS_CLOG 18        /* |z|^2, z = log(H / ref) on the principal branch, g = 2 conj(z) / H */
#define PFR_LOSS_CCOTANGENT 19  /* ref holds dL/dH (complex), loss not computed */
/* losses on the field (pfr_field_loss_sweep): x_j the selected rows of the solution, r_j the reference, v_j the weights;
 * d term = Re(sum_j g_j dx_j), g_j = v_j (c1 conj(x_j) + c2 conj(r_j)) */
#define PFR_LOSS_FMSE 32        /* sum v |x - r|^2,                                 c1 = 2, c2 = -2 */
#define PFR_LOSS_FRMSE 33       /* sum v |x - r|^2 / R2, R2 = sum v |r|^2,          c1 = 2 / R2, c2 = -2 / R2 */
#define PFR_LOSS_FMAC 34        /* 1 - |s|^2 / (X2 R2), s = sum v conj(r) x, X2 = sum v |x|^2 (one minus the modal
                                 * assurance criterion), c1 = 2 |s|^2 / (X2^2 R2), c2 = -2 conj(s) / (X2 R2) */
#define PFR_LOSS_FCOTANGENT 35  /* ref holds dL/dx (complex, per selected row), loss not computed */

typedef struct pfr_symbolic pfr_symbolic;
typedef struct pfr_solver pfr_solver;

typedef struct pfr_symbolic_options {
  int32_t leaf_size;   /* nested-dissection leaf size (default 10000): parts at or below it are
                        * ordered by multiple minimum degree */
  int32_t ordering;    /* 0 nested dissection + multiple-minimum-degree leaves (default), 1 natural,
                        * 2 nested dissection + exact minimum-degree leaves (the round 1-3 ordering) */
  int32_t relax_small, relax_mid, relax_big; /* supernode amalgamation (4, 8, 24) */
  double zrelax_mid, zrelax_big;             /* (0.5, 0.1) */
  /* 1: symmetric-structure analysis (default 0).  The caller guarantees that the matrices
   * factorised with it are complex symmetric (A = A^T, non-conjugate) once the Dirichlet
   * rows -- rows holding only their diagonal entry (tgv = -1 rows, pyFFInterface.py:176) --
   * and their columns are removed.  Those nodes are decoupled (their column entries move
   * to the right-hand side / the adjoint's Dirichlet rows), the rest is factorised as
   * A = L U with U = diag(U) L^T implicit: only L is formed and read. */
  int32_t symmetric;
  /* Nodes to be eliminated last, together (default none): ordered after every other node, they
   * form the root front.  The engine passes the loss functional's support, so that the adjoint's
   * bottom-up solve stays inside the root and both top-down solves run as one pass. */
  int32_t n_last;
  const int32_t* last;
  int32_t max_ns;      /* fundamental supernodes split into pieces of at most max_ns pivots (default 256;
                        * 0 = no split) */
  int32_t md_delta;    /* multiple minimum degree: each stage eliminates an independent set of the
                        * nodes of external degree <= minimum + md_delta (default 4) */
} pfr_symbolic_options;

typedef struct pfr_symbolic_stats {
  int32_t n;
  int64_t nnz;
  int32_t n_fronts;
  int32_t n_levels;
  int32_t max_front;
  int64_t total_rows;      /* sum of front sizes */
  int64_t factor_entries;  /* sum of squared front sizes (dense front storage per frequency) */
  int64_t nnz_lu;          /* entries of L + U (per frequency) */
  double factor_flops;     /* real flops of one numeric factorisation */
  int32_t symmetric;       /* analysis built with options.symmetric = 1 */
  int32_t n_dirichlet;     /* symmetric mode: decoupled Dirichlet nodes */
  int64_t n_coupling;      /* symmetric mode: entries (i, d), i not Dirichlet, d Dirichlet */
} pfr_symbolic_stats;

/* export ids for pfr_symbolic_export (int32 arrays unless noted) */
#define PFR_EXPORT_PERM 0        /* n: new -> old */
#define PFR_EXPORT_IPERM 1       /* n: old -> new */
#define PFR_EXPORT_FRONTS 2      /* n_fronts x 8 int64: ns, f, row0, col0, parent, level, off, wv */
#define PFR_EXPORT_IDX 3         /* total_rows */
#define PFR_EXPORT_RELPOS 4      /* total_rows */
#define PFR_EXPORT_ASM_PTR 5     /* total_rows + 1 */
#define PFR_EXPORT_ASM_COL 6     /* nnz */
#define PFR_EXPORT_ASM_NZ 7      /* nnz */
#define PFR_EXPORT_EA_PTR 8      /* total_rows + 1 */
#define PFR_EXPORT_EA_SRC 9      /* ea_ptr[total_rows] */
#define PFR_EXPORT_LEVEL_PTR 10  /* n_levels + 1 */
#define PFR_EXPORT_LEVEL_FRONTS 11 /* n_fronts */
#define PFR_EXPORT_DIRICHLET 12  /* n_dirichlet x 2: permuted node, CSC index of its diagonal entry */
#define PFR_EXPORT_COUPLING 13   /* n_coupling x 3: permuted row i, Dirichlet slot, CSC index; by row */

PFR_API const char* pfr_version(void);
/* Message of the last failed call on this thread ("" if none). */
PFR_API const char* pfr_last_error(void);
PFR_API void pfr_symbolic_options_default(pfr_symbolic_options* opt);

/* ---------------------------------------------------------------- symbolic (host only, no GPU)
 * Replaces InnerState::add_mat -> umfpack_zi_symbolic (InnerState.h:120-162) and
 * create_symbolic (Sparse.py:92-116).  Pattern = n x n CSC (colptr n+1, rowind nnz),
 * the union pattern of Problem.py:317-332.  opt may be NULL (defaults). */
PFR_API int pfr_symbolic_create(int32_t n, int64_t nnz, const int32_t* colptr, const int32_t* rowind,
                                const pfr_symbolic_options* opt, pfr_symbolic** out);
PFR_API int pfr_symbolic_stats_get(const pfr_symbolic* sym, pfr_symbolic_stats* out);
PFR_API int pfr_symbolic_export(const pfr_symbolic* sym, int32_t what, void* dst, int64_t capacity_bytes);
PFR_API void pfr_symbolic_destroy(pfr_symbolic* sym);

/* ---------------------------------------------------------------- device solver
 * Uploads the symbolic maps and allocates frequency-minor workspaces for up to
 * max_batch frequencies per chunk.  Keeps a copy of colptr/rowind for matvec. */
PFR_API int pfr_solver_create(const pfr_symbolic* sym, const int32_t* colptr, const int32_t* rowind,
                              int32_t device, int32_t max_batch, pfr_solver** out);
PFR_API void pfr_solver_destroy(pfr_solver* s);
/* device bytes pfr_solver_create would allocate for max_batch */
PFR_API int64_t pfr_solver_workspace_bytes(const pfr_symbolic* sym, int32_t max_batch);
PFR_API int32_t pfr_solver_max_batch(const pfr_solver* s);

/* The launch schedule: which kernel form every tree level launches in every pass, and with what shape.  The library
 * decides it once per solver, from the launch-shape environment knobs (PFR_SOLVE_WMAX, PFR_US2_NAR, ...) read at
 * pfr_solver_create, the level geometry and the right-hand-side reaches; its level loops launch exactly these records.
 * pfr_symbolic_schedule: the schedule a solver created now for max_batch would start with, every front reached (host
 * only, no device).  pfr_solver_schedule: the live schedule of a solver, with its current reaches.
 * dst receives n_levels x PFR_SCHED_COLS int32 (capacity in bytes): the six tables below one after the other, each
 * n_levels rows (level 0 first) of its column count.  In the paired, chain and unpaired tables nf = 0 (nmax = 0) means
 * the level launches nothing in that pass.
 *   factor (13): nf, maxns, fused0 (level through k_front0 in operator-form sweeps), f0_small (its fronts of <= 2
 *                pivots), lds (A11 by k_factor_sym_lds), G (lane groups per wave of k_factor_sym), waves (A11 panel),
 *                off_small, off_pu (L21: SMALL form; 3 = pipelined prefix, 2 = plain), nasm, nitems, nblocks, ntiles
 *   pair (9):    paired top-down pass.  nf, form (0 tiny4, 1 tiny8, 2 rl, 3 level_small, 4 level_big), upd (0 none,
 *                1 k_usolve2_upd, 2 k_usolve2_updc), split, waves (of the pivot-block kernel), rpl (rl), RB (updc),
 *                tiny, small (the level's classes under PFR_US2_TINY / PFR_US2_SMALL, whichever form runs)
 *   chain (11):  bottom-up chain of the loss sweeps.  nf0, nf1 (fronts of reach 0 / 1), nmax, nsum, form (0 plain,
 *                1 NAR, 2 RL), rows (0 none, 1 k_lsolve_rows_z, 2 k_lsolve_rows_zc), split, waves, rpl (RL), RB (zc),
 *                lds_bytes (NAR: dynamic LDS)
 *   solve_all, solve_reach0, solve_reach1 (5 each): the unpaired passes over all fronts / the fronts of reach 0 / 1.
 *                nf, level_w (the level's size-based wave count), waves (the launch's), split_L, split_U */
#define PFR_SCHED_FACTOR_COLS 13
#define PFR_SCHED_PAIR_COLS 9
#define PFR_SCHED_CHAIN_COLS 11
#define PFR_SCHED_SOLVE_COLS 5
#define PFR_SCHED_COLS (PFR_SCHED_FACTOR_COLS + PFR_SCHED_PAIR_COLS + PFR_SCHED_CHAIN_COLS + 3 * PFR_SCHED_SOLVE_COLS)
PFR_API int pfr_symbolic_schedule(const pfr_symbolic* sym, int32_t max_batch, int32_t* dst, int64_t capacity_bytes);
PFR_API int pfr_solver_schedule(const pfr_solver* s, int32_t* dst, int64_t capacity_bytes);

/* Pruning: factor and solve only the trees of the elimination forest that the load reaches (symmetric solvers; off
 * by default).  A tree is loaded when one of its rows has a non-zero entry of the vector given to pfr_set_rhs, or is
 * a coupled row of a Dirichlet node whose entry of that vector is non-zero; on every other tree the forward solution
 * of the operator right-hand side is exactly zero, and so is every term of the loss, the gradient, the Jacobian rows
 * and the functional correction that the tree's adjoint enters (each multiplies it by the forward solution or by the
 * load).  With pruning on, the operator-form sweeps (pfr_sweep, pfr_sweep_fresh, pfr_sweep_complex, the two Jacobian
 * sweeps, pfr_population_sweep) factorise, solve and walk the loaded trees only: a view of the plan and schedule over
 * their fronts, rebuilt when pfr_set_rhs changes which trees are loaded.  Rows of unloaded trees hold exact zeros in
 * the solution vectors, the adjoint's backward error is taken over the loaded rows, and a pivot failure inside an
 * unloaded tree no longer flags its frequency (nothing of that tree is factorised).  A solver on which every tree is
 * loaded builds nothing and launches exactly what it launches with pruning off.  pfr_hessian_sweep and the refinement
 * check modes (PFR_CHECK_REFINE, PFR_CHECK_REFINE_ADJ) keep the full plan; so do pfr_solve / pfr_solve_multi, which
 * need a general analysis, where no view is ever built.
 * pfr_debug_solution still returns the whole adjoint: it completes the unloaded trees for the last chunk on demand.
 * pfr_solver_active: the number of fronts the sweeps factorise, and per front 0 / 1 into mask (may be NULL; capacity in
 * entries).  pfr_solver_schedule_active: the schedule of the view the sweeps launch (pfr_solver_schedule's layout;
 * the full schedule while nothing is pruned).  pfr_solver_alg_bytes / pfr_solver_solve_bytes count what the sweeps
 * launch under the current check mode: the view, or the full plan under the refinement modes. */
PFR_API int pfr_set_prune(pfr_solver* s, int32_t on);
/* Host only, no device: the views pruning builds on a solver for max_batch whose right-hand side vector is rhs (caller
 * numbering, n entries) and whose functional support is index[0 .. n_support).  mask (n_fronts): 1 = the front's tree
 * is loaded.  Builds the plan and schedule of the loaded trees and of the rest (the view pfr_debug_solution completes
 * the adjoint on) and checks every index and record of both as pfr_solver_create's plan is checked (PFR_ERR_STATE and
 * pfr_last_error on a violation); sched_active / sched_rest / sched_full (may be NULL, capacity in bytes each): their
 * schedules and the full plan's with the same reaches, in pfr_symbolic_schedule's layout.  A view's records take every
 * launch-shape decision as the full plan takes it (from the whole analysis' level geometry and the full reaches;
 * fused0 from every level-0 front of the analysis: a view with a level-0 front runs it through k_front0 exactly when
 * the full plan does) and only their counts from the view: each front runs the same arithmetic in the same order with
 * pruning on and off. */
PFR_API int pfr_symbolic_prune(const pfr_symbolic* sym, int32_t max_batch, const double* rhs, int32_t n_support,
                               const int32_t* index, int32_t* mask, int32_t* sched_active, int32_t* sched_rest,
                               int32_t* sched_full, int64_t capacity_bytes);
PFR_API int32_t pfr_solver_active(const pfr_solver* s, int32_t* mask, int64_t capacity);
PFR_API int pfr_solver_schedule_active(const pfr_solver* s, int32_t* dst, int64_t capacity_bytes);
/* Live stiffness matrices: the matrices k with a non-zero value (!= 0.0) on at least one entry
 * of the rows a sweep's forward residual walk visits -- the pivot rows of the loaded trees under pruning, every row
 * otherwise.  The gradient contraction fused into that walk accumulates only those when they are 6 or 12 of more
 * (a table compacted to them is built once per view and pfr_set_stiffness; PFR_CONTRACT_LIVE=0 or any other count:
 * all n_stiff); the partials of the other matrices are written as the zeros their sums are, so every output keeps its
 * bits.
 * pfr_symbolic_live (host only, no device): the live set as a bit mask (bit k) for the stiffness table stiff_host
 * (nnz x n_stiff, entry-major, as pfr_set_stiffness takes it on the device) on a symmetric analysis whose right-hand
 * side vector is rhs (caller numbering); prune != 0: over the loaded trees' rows, else over every row.  Returns the
 * number of live matrices, or -1 on bad arguments.
 * pfr_solver_live: the same for the view the operator-form sweeps walk now (the loaded trees' under pruning);
 * *compact (may be NULL) = 1 when the walk takes the compacted table.  A solver on a general analysis keeps all. */
PFR_API int32_t pfr_symbolic_live(const pfr_symbolic* sym, const double* rhs, int32_t prune, int32_t n_stiff,
                                  const double* stiff_host, uint32_t* live);
PFR_API int32_t pfr_solver_live(const pfr_solver* s, uint32_t* live, int32_t* compact);

/* ---------------------------------------------------------------- InnerState-compatible entry points
 * pfr_solve: x[q] = A_q^{-1} b[q]  (transpose != 0: A_q^{-T} b[q], NON-conjugate, = UMFPACK_Aat,
 * InnerState.h:183-185).  A_q values on the CSC pattern: data_dev + q * data_stride (complex, nnz);
 * data_stride = 0 broadcasts one matrix (modes 0/2 of InnerState::solve, InnerState.h:192-233);
 * b_stride likewise (0 = broadcast b, mode 1).  Batch-major (batch, n) complex output.
 * Replaces InnerState::solve (InnerState.h:164-308).  flags_dev: int32 per batch item (may be NULL).
 * Needs a solver on a general analysis (options.symmetric = 0): explicit matrices carry no symmetry
 * guarantee (PFR_ERR_STATE otherwise). */
PFR_API int pfr_solve(pfr_solver* s, int32_t batch, const double* data_dev, int64_t data_stride,
                      const double* b_dev, int64_t b_stride, double* x_dev, int32_t transpose,
                      int32_t* flags_dev, void* stream);

/* Several right-hand sides per matrix on the same factors: the reference's batching mode 4
 * (data (B, nnz), b (J, B, N), Sparse.py:245-282, used by jax.hessian), which refactorises for every
 * right-hand side (InnerState.h:289-305).  b of rhs r, item q at b_dev + 2 * (r * b_rhs_stride +
 * q * b_stride) doubles (b_stride 0 = broadcast); x of rhs r at x_dev + 2 * r * x_rhs_stride
 * (items contiguous, stride n; x_rhs_stride >= batch * n when nrhs > 1). */
PFR_API int pfr_solve_multi(pfr_solver* s, int32_t batch, int32_t nrhs, const double* data_dev,
                            int64_t data_stride, const double* b_dev, int64_t b_stride, int64_t b_rhs_stride,
                            double* x_dev, int64_t x_rhs_stride, int32_t transpose, int32_t* flags_dev,
                            void* stream);
/* pfr_matvec: y[q] = A_q x[q] (or A_q^T x[q]); replaces InnerState::matvec (InnerState.h:310-470). */
PFR_API int pfr_matvec(pfr_solver* s, int32_t batch, const double* data_dev, int64_t data_stride,
                       const double* x_dev, int64_t x_stride, double* y_dev, int32_t transpose, void* stream);

/* ---------------------------------------------------------------- fused operator-form sweep
 * The hot path of Problem.getFRFunction / getLossFunction (Problem.py:432-477, 948-975) fused
 * with the reverse pass JAX derives from Sparse.py:162-222:
 *   A(omega) = K - omega^2 M,  b(omega) = rhs * (beta - omega^2 mass_sum),
 *   fr = sqrt(ts^2|aU.x|^2 + ts^2|aV.x|^2 + |aW.x|^2),
 *   loss = scale * sum_q term(fr_q, ref_q),
 *   w_k = sum_q ( -lam_q^T S_k x_q + e_k lam_q^T rhs ),   A^T lam_q = d loss / d x_q.
 * The (F, nnz) matrix batch is never materialised. */

/* K_out_dev = sum_k coef_k * S_k  (S registered by pfr_set_stiffness), complex nnz.  n_stiff is 18
 * (A, B, D coefficient matrices of Problem.py:440-445) or 12 (A and D only: the B coefficients vanish
 * for mid-plane symmetric laminates, so their matrices and gradient partials are left out).
 * pfr_set_stiffness registers stiff_dev: pfr_combine, the Hessian sweep and the gradient contraction of
 * every loss sweep (fused into the forward residual walk by default) read it at every call, so the
 * buffer must stay alive and unchanged while the solver uses it (an entry-ordered copy is also taken
 * for the k_contract_eg path; after changing the values, call pfr_set_stiffness again). */
PFR_API int pfr_set_stiffness(pfr_solver* s, int32_t n_stiff, const double* stiff_dev /* (nnz, n_stiff) */,
                              const double* rhs_weights /* host, n_stiff: e_k */);
PFR_API int pfr_combine(pfr_solver* s, const double* coef /* host complex n_stiff */, double* K_out_dev,
                        void* stream);
PFR_API int pfr_set_operator(pfr_solver* s, const double* K_dev /* complex nnz */, const double* M_dev /* real nnz */);
PFR_API int pfr_set_rhs(pfr_solver* s, const double* rhs_host /* real n, caller numbering */, double beta_re,
                        double beta_im, double mass_sum);
PFR_API int pfr_set_functional(pfr_solver* s, int32_t n_support, const int32_t* index_host /* caller numbering */,
                               const double* a_host /* 3 x n_support: aU, aV, aW */, double ts);
/* nfreq frequencies [Hz] (device).  loss_type PFR_LOSS_NONE: forward only (fr_dev).  Otherwise ref_dev
 * (complex nfreq) and the reverse pass: loss_dev[0] += sum of terms * scale ... (raw sum, unscaled),
 * w_dev (complex n_stiff) += gradient partials.  fr_dev / loss_dev / w_dev / flags_dev may be NULL. */
PFR_API int pfr_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev, int32_t loss_type,
                      const double* ref_dev, double scale, double* fr_dev, double* loss_dev, double* w_dev,
                      int32_t* flags_dev, void* stream);
/* pfr_sweep with fresh outputs: loss_dev[0], w_dev (n_stiff complex) and flags_dev[0 .. nfreq) zeroed and the
 * pfr_set_check backward-error buffer set to NaN by the sweep's first kernel, then filled as pfr_sweep accumulates
 * them -- the loss step's initialisation without separate fills before the sweep (Problem._Engine.loss_step). */
PFR_API int pfr_sweep_fresh(pfr_solver* s, int32_t nfreq, const double* freqs_dev, int32_t loss_type,
                            const double* ref_dev, double scale, double* fr_dev, double* loss_dev, double* w_dev,
                            int32_t* flags_dev, void* stream);
/* Sweeps of this solver replayed from its captured hipGraph so far.  A pfr_sweep called again with the same
 * arguments, stream and solver state (no setter called in between; pfr_set_check's mode, tolerance and berr
 * pointer are part of the arguments) is captured into a hipGraph on that second call and replayed with one
 * hipGraphLaunch afterwards -- the same kernels with the same arguments; only with PFR_GRAPH=1 (off by default).  The
 * reference's analogue is none: its sweep is a host loop of UMFPACK calls (InnerState.h:276-288). */
PFR_API int64_t pfr_sweep_graph_launches(const pfr_solver* s);
/* Per-frequency sensitivities on one factorisation per frequency: fr_dev[q] as pfr_sweep, and
 *   jc_dev[q * n_stiff + k] = -mu_q^T S_k x_q + e_k mu_q^T rhs,   A_q^T mu_q = d fr_q / d x_q
 * (complex, WRITTEN not accumulated, every row q < nfreq), in the convention of w: for any real cot,
 *   sum_q cot_q jc[q][k] = w_k of pfr_sweep(PFR_LOSS_COTANGENT, ref.re = cot, scale 1) in the same check mode,
 * so d fr_q / d theta_i = Re sum_k jc[q][k] d c_k / d theta_i.  The reverse sweep of a unit cotangent per frequency
 * with the frequency sum left out: every pfr_set_check mode applies as in a loss sweep (under PFR_CHECK_CORRECT fr is
 * the corrected response and the rows carry the solve-error scale).  Never part of the PFR_GRAPH graph; the next
 * loss sweep is bit-identical to one run without it.  The reference has no analogue: jax.jacobian of its fr function
 * solves one adjoint system per frequency and refactorises for each (InnerState.h:289-305). */
PFR_API int pfr_jacobian_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev, double* fr_dev /* may be NULL */,
                               double* jc_dev, int32_t* flags_dev /* may be NULL */, void* stream);
/* The complex response: with a real sensing axis d = (dU, dV, dW) (host, 3 doubles; read during the call),
 *   H_q = dU ts U_q + dV ts V_q + dW W_q            (complex; U, V, W and ts of pfr_set_functional)
 * -- d = (0, 0, 1) is the out-of-plane transfer function, (cos phi, sin phi, 1) a z-axis accelerometer with its
 * transverse sensitivity along phi.  H is the number the solver's x gives, with NO conjugation: a reference recorded
 * in the other time convention (e^{-i omega t} against e^{+i omega t}) must be conjugated by the caller.
 * pfr_sweep_complex: h_dev[q] = H_q (complex nfreq, may be NULL) and, with a loss (PFR_LOSS_CMSE .. PFR_LOSS_CCOTANGENT,
 * ref_dev complex nfreq), loss_dev[0] and w_dev accumulated as pfr_sweep does (fresh != 0: initialised by the sweep as
 * pfr_sweep_fresh does), with A^T lam_q = scale g_q a_d and g the loss's complex cotangent, d term = Re(g dH).
 * pfr_jacobian_sweep_complex: jc_dev[q * n_stiff + k] = -m_q mu_q^T S_k x_q + e_k t_q with A^T mu = a_d, so that
 *   dH_q = sum_k jc[q][k] dc_k     (complex, no real part taken),
 * and for any complex g, sum_q g_q jc[q][k] = w_k of a PFR_LOSS_CCOTANGENT sweep with ref = g and scale 1.
 * H is linear in x, so mu does not depend on x and the functional correction H + mu^T r (PFR_CHECK_CORRECT) is exact
 * in the forward solve's error.  Every pfr_set_check mode applies except PFR_CHECK_REFINE_ADJ (PFR_ERR_ARG).
 * PFR_ERR_ARG before any launch: a loss id outside {PFR_LOSS_NONE, 16 .. 19} (the magnitude's ids 0 .. 4 included), a
 * zero or non-finite axis, a loss without ref_dev.  Never part of the PFR_GRAPH graph; the next magnitude sweep is
 * bit-identical to one run without them.  Out of scope: the Hessian of the complex losses, complex responses in the
 * population sweep, several channels in one sweep.  The reference computes the phases and drops them
 * (Problem.py _solve: uang, vang, wang). */
PFR_API int pfr_sweep_complex(pfr_solver* s, int32_t nfreq, const double* freqs_dev, const double* axis /* host, 3 */,
                              int32_t loss_type /* PFR_LOSS_NONE or 16..19 */, const double* ref_dev /* complex nfreq */,
                              double scale, double* h_dev /* complex nfreq, may be NULL */, double* loss_dev,
                              double* w_dev, int32_t* flags_dev, int32_t fresh /* as pfr_sweep_fresh */, void* stream);
PFR_API int pfr_jacobian_sweep_complex(pfr_solver* s, int32_t nfreq, const double* freqs_dev, const double* axis,
                                       double* h_dev /* may be NULL */, double* jc_dev, int32_t* flags_dev, void* stream);
/* The inertia rows: sensitivities to the other half of the operator.  With the mass matrix split into n_mass components,
 *   A(omega) = K - omega^2 sum_j I_j G_j,   b(omega) = rhs (beta - omega^2 sum_j d_j I_j),
 * pfr_set_inertia registers the components G_j (mass_dev: (nnz, n_mass) real, entry-major like pfr_set_stiffness' table;
 * n_mass 1 .. 4) and their load weights d_j (rhs_weights, host).  It takes an entry-ordered copy of the table (after
 * changing the values, call it again), lists the pattern entries on which some component is non-zero -- under pruning
 * only those on the loaded trees' rows; the list follows pfr_set_prune and a pfr_set_rhs that changes the loaded trees --
 * and, like every setter, ends the captured graph.  It does not touch M or mass_sum: the caller keeps pfr_set_operator's
 * M = sum_j I_j G_j and pfr_set_rhs' mass_sum = sum_j d_j I_j consistent with its coefficients I_j, which the library
 * never sees.
 * pfr_inertia_sweep is pfr_jacobian_sweep (axis == NULL: resp_dev holds fr, real nfreq) or pfr_jacobian_sweep_complex
 * (axis: 3 host doubles, resp_dev holds the complex H) with one more output per frequency,
 *   jm_dev[q * n_mass + j] = omega_q^2 ( m_q mu_q^T G_j x_q - d_j t_q )        (complex, WRITTEN, every row q < nfreq),
 * m_q and t_q = m_q mu_q^T rhs the cotangent scale and load term of the rows jc, omega_q = 2 pi f_q, so that
 *   d fr_q / d I_j = Re jm[q][j]      (the complex response: d H_q / d I_j = jm[q][j], no real part taken).
 * resp_dev and jc_dev may be NULL (jc_dev NULL: the stiffness contraction is skipped and pfr_set_stiffness is not
 * needed); what they receive, the flags and the pfr_set_check backward errors are bitwise those of the Jacobian sweep
 * on the same solver state.  Two identities tie the rows together, in every check mode:
 *   homogeneity:      sum_k c_k jc[q][k] + sum_j I_j jm[q][j] = 0       (complex; scaling K, beta, M and mass_sum alike
 *                                                                         leaves x where it is)
 *   frequency slope:  d fr_q / d f = (2 / f_q) Re sum_j I_j jm[q][j]    (f in Hz; H: the same without Re)
 * Every pfr_set_check mode applies as in the Jacobian sweeps (PFR_CHECK_REFINE_ADJ: honoured for fr, PFR_ERR_ARG with
 * an axis).  Per chunk, after k_jac_finish: k_contract_mass (lane = frequency, the listed entries only, fixed order, no
 * atomics; its partials take the stiffness partials' buffer) and k_inertia_finish.  Never part of the PFR_GRAPH graph;
 * the next loss sweep is bit-identical to one run without it.
 * PFR_ERR_ARG before any launch: a null solver or jm_dev, nfreq <= 0, a zero or non-finite axis, n_mass outside 1 .. 4
 * (pfr_set_inertia).  PFR_ERR_STATE: no operator, rhs or functional, no pfr_set_inertia, jc_dev without pfr_set_stiffness.
 * Out of scope: inertia rows in pfr_population_sweep, pfr_hessian_sweep and pfr_field_loss_sweep, and across devices.
 * The reference has no analogue: its inertia constants are Python floats closed over by _solve (Problem.py).
 * pfr_symbolic_mass_list (host only, no device): the list pfr_set_inertia builds for the table mass_host on this
 * analysis -- prune != 0: for the trees loaded by rhs (caller numbering; symmetric analyses), else every row.  Returns
 * the number of listed entries (-1: bad arguments or a capacity below what is written).  The contraction's waves each
 * own a fixed range of the contraction entries, the same on every view (so that a view's rows equal the full walk's bit
 * for bit); list (may be NULL) receives the listed positions in ascending order, wave by wave, each wave's run padded
 * with -1 to whole 4-entry batches, ptr (may be NULL) the first batch of each wave's run and the end (waves + 1);
 * entries (may be NULL; capacity in int32) the contraction entries, four int32 each: permuted column, matrix entry
 * (i, j) or -1, matrix entry (j, i) or -1, permuted row; counts (may be NULL, 3): the contraction entries, the list's
 * padded length, the waves.
 * pfr_solver_mass_list: the count for the view the operator-form sweeps walk now (-1 before pfr_set_inertia), *padded
 * (may be NULL) the length on the device. */
PFR_API int pfr_set_inertia(pfr_solver* s, int32_t n_mass /* 1..4 */, const double* mass_dev /* (nnz, n_mass) */,
                            const double* rhs_weights /* host, n_mass: d_j */);
PFR_API int pfr_inertia_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev,
                              const double* axis /* host, 3, or NULL: the magnitude fr */,
                              double* resp_dev /* may be NULL */, double* jc_dev /* may be NULL */, double* jm_dev,
                              int32_t* flags_dev /* may be NULL */, void* stream);
PFR_API int32_t pfr_symbolic_mass_list(const pfr_symbolic* sym, const double* rhs, int32_t prune, int32_t n_mass,
                                       const double* mass_host, int32_t* list, int64_t capacity, int32_t* ptr,
                                       int64_t ptr_capacity, int32_t* entries, int64_t entries_capacity,
                                       int32_t* counts);
PFR_API int32_t pfr_solver_mass_list(const pfr_solver* s, int32_t* padded);
/* The field: the solution x_q of (K - omega_q^2 M) x = b itself, at every frequency, for the rows the caller selects
 * -- the operating deflection shapes over a band, and the data under the reference's Problem.getModePicture
 * (Problem.py:521-608, one UMFPACK solve per picture).
 *   out_dev[q * n_sel + j] = x_q[rows[j]]      (complex, nfreq x n_sel, frequency-major, caller numbering)
 * rows_host: n_rows int32 in the caller's numbering, repeats and any order allowed (n_sel = n_rows); NULL: all n rows
 * in order (n_sel = n, n_rows ignored).  fr_dev (may be NULL): fr as a PFR_LOSS_NONE pfr_sweep gives it without the
 * functional correction.  Per chunk the call launches what pfr_sweep(PFR_LOSS_NONE) launches with the check mode
 * reduced to its PFR_CHECK_FORWARD and PFR_CHECK_REFINE bits (the functional kernel only with fr_dev), on the view that
 * sweep runs on, then k_field_gather: a transpose of the chunk's frequency-minor, permuted solution through LDS in
 * tiles of 64 frequencies x pfr_field_tile_rows() selected rows.  PFR_CHECK_CORRECT, PFR_CHECK_ADJOINT and
 * PFR_CHECK_REFINE_ADJ are ignored, not refused: there is no functional to correct and no adjoint.  Under pruning the
 * rows of unloaded trees come out as exact +0.0, the true solution there; Dirichlet rows come out with the values the
 * solve gives them.  flags_dev (may be NULL): the bad-pivot and forward backward-error flags as in pfr_sweep; a
 * pfr_set_check berr_dev gets slot 2 q written and 2 q + 1 left alone.  Nothing is written outside out_dev's nfreq x
 * n_sel entries.  PFR_ERR_ARG before anything is launched: a null out_dev, n_rows <= 0 with a list, a row outside
 * [0, n).  The selection is uploaded once per call on the sweep's stream.  Never part of the PFR_GRAPH graph; the next
 * loss sweep is bit-identical to one run without it.  Like every sweep the call needs the operator, the right-hand side
 * and the functional set (PFR_ERR_STATE otherwise) -- pfr_set_functional too when fr_dev is NULL: the analysis' reaches
 * are set with it.
 * Out of scope: the adjoint field, a population form, a complex-axis form (pfr_sweep_complex gives H), gathering the
 * field across ranks.  No longer out of scope: gradients through the field and a loss on field data, which
 * pfr_field_loss_sweep gives. */
PFR_API int pfr_field_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev, int32_t n_rows,
                            const int32_t* rows_host, double* out_dev /* complex nfreq x n_sel */,
                            double* fr_dev /* nfreq, may be NULL */, int32_t* flags_dev /* may be NULL */, void* stream);
/* selected rows per tile of k_field_gather (the sizes at which its launch grid changes) */
PFR_API int32_t pfr_field_tile_rows(void);
/* A loss on the field and its gradient: full-field data (a scanning vibrometer's deflection shapes) fitted directly.
 * With x_j = x_q[rows[j]], r_j = ref_dev[q * n_sel + j] (the layout of pfr_field_sweep's out_dev: a field computed
 * earlier serves as data unchanged) and weights v_j (weights_host, n_sel real, NULL: all 1), per frequency q the term
 * and seed of PFR_LOSS_FMSE / FRMSE / FMAC (see the ids); the seed convention is the complex response's:
 * d term = Re(sum_j g_j dx_j), the adjoint A^T lam_q = scale g_q, non-conjugate.  Then, accumulating as pfr_sweep does
 * (fresh != 0: as pfr_sweep_fresh),
 *   loss_dev[0] += scale sum_q term_q,     w_dev[k] += sum_q (-lam_q^T S_k x_q + e_k lam_q^T rhs)   (complex n_stiff).
 * PFR_LOSS_FCOTANGENT: g_j = ref (the caller's dL/dx), no term, loss_dev left alone (may be NULL), no weights.
 * out_dev (may be NULL): the field too, bitwise pfr_field_sweep's in the same mode.
 * Per chunk: the unpaired full forward solve (refined under PFR_CHECK_REFINE), k_field_terms / k_field_finish /
 * k_field_seed (the loss's sums over tiles of 64 frequencies x pfr_field_tile_rows() rows, the term and two seed
 * coefficients per frequency, the seed scattered into the adjoint's right-hand side), the unpaired adjoint solve over
 * every front, k_contract_eg, k_rhs_dot and k_reduce.  The call honours PFR_CHECK_FORWARD, PFR_CHECK_ADJOINT and
 * PFR_CHECK_REFINE; the other bits are ignored, not refused (there is no single functional to correct), and it runs
 * pruned exactly when a sweep in that reduced mode would.  Under pruning selected rows of unloaded trees enter the
 * terms with x = +0.0 (a constant); their seed is written but nothing in w needs their adjoint, which stays +0.0 until
 * pfr_debug_solution(1, q) completes it.  A frequency with R2 = 0 (FRMSE, FMAC) or X2 = 0 (FMAC) gives a non-finite
 * term: validate the reference before the call.  Never part of the PFR_GRAPH graph; the next loss sweep is
 * bit-identical to one run without it.
 * PFR_ERR_ARG before any launch: a null ref_dev or w_dev, a null loss_dev with a loss term, a loss id outside 32 .. 35,
 * a weight that is negative or not finite, all weights zero, weights with FCOTANGENT, n_rows <= 0 with a list, a row
 * outside [0, n), a repeated row (the seed is a scatter: pfr_field_sweep allows repeats, this call does not).
 * PFR_ERR_STATE: as the reverse sweeps (no operator, rhs, functional or stiffness set).
 * Out of scope: the field Jacobian and covariance, the Hessian, population and distributed forms, a correction of the
 * field loss (near a resonance the accuracy tool is PFR_CHECK_REFINE), magnitude-only field data. */
PFR_API int pfr_field_loss_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev, int32_t n_rows,
                                 const int32_t* rows_host /* NULL: all n rows */,
                                 const double* weights_host /* n_sel, may be NULL */, int32_t loss_type /* 32..35 */,
                                 const double* ref_dev /* complex nfreq x n_sel */, double scale,
                                 double* out_dev /* complex nfreq x n_sel, may be NULL */, double* loss_dev,
                                 double* w_dev, int32_t* flags_dev /* may be NULL */, int32_t fresh, void* stream);
/* A population of parameter sets in one sweep: a lane is a (member, frequency) pair.
 * pfr_combine_batch: Kpop_dev[m * nnz + nz] = sum_k coef[m * n_stiff + k] S_k(nz) for m < n_members (member-major;
 * each row bitwise what pfr_combine gives for that member's coefficients), the stiffness read once.
 * pfr_population_sweep: nlane lanes, a positive multiple of 64; the lanes 64 g .. 64 g + 63 (group g) solve
 *   (Kpop[member[g]] - omega_q^2 M) x_q = rhs (beta[member[g]] - omega_q^2 mass_sum)
 * with rhs and mass_sum of pfr_set_rhs and M of pfr_set_operator (that call's K and pfr_set_rhs's beta are not read).
 * With jc_dev the sweep is pfr_jacobian_sweep's per lane (fr_dev[q], jc_dev[q * n_stiff + k] written); without,
 * the forward sweep (fr_dev only).  Every pfr_set_check mode applies per lane as in those sweeps, except
 * PFR_CHECK_REFINE_ADJ (it ranks the groups of a chunk against each other: PFR_ERR_ARG).  A lane's results are
 * bitwise those of pfr_jacobian_sweep over the same nlane frequencies with that member's K and beta set.  A member
 * index outside [0, n_members) or an nlane that is no multiple of 64 is PFR_ERR_ARG, checked before anything is
 * launched.  Never part of the PFR_GRAPH graph; the next loss sweep is bit-identical to one run without it.  The
 * reference evaluates a population one member at a time (scipy calling its loss function, Optimizers.py). */
PFR_API int pfr_combine_batch(pfr_solver* s, int32_t n_members, const double* coef_host /* n_members x n_stiff complex */,
                              double* Kpop_dev /* n_members x nnz complex */, void* stream);
PFR_API int pfr_population_sweep(pfr_solver* s, int32_t nlane, const double* freqs_dev /* nlane */,
                                 const int32_t* member_host /* nlane / 64 */, int32_t n_members,
                                 const double* Kpop_dev, const double* beta_host /* n_members complex */,
                                 double* fr_dev /* nlane */, double* jc_dev /* nlane x n_stiff complex, may be NULL */,
                                 int32_t* flags_dev /* may be NULL */, void* stream);
/* Stream ordering for a host that drives several solver lanes: work enqueued on `waiter` after this call starts
 * only after the work enqueued on `signaller` before it (one event of the calling thread and device, recorded on
 * signaller, waited for on waiter; both HIP stream handles of the current device).  The loss step orders each lane's
 * stream after the caller's and the caller's after every lane with it (Problem._Engine._run) -- one C call where
 * torch's Stream.wait_stream makes and destroys an event.  No reference analogue (its sweep is a host loop,
 * InnerState.h:276-288). */
PFR_API int pfr_stream_order(void* waiter, void* signaller);

/* Exact second derivatives with the factors of the sweep reused (replaces the reference's
 * forward-over-reverse Hessian, `jax.jacobian(grad)` in Optimizers.py:125-136, whose mode-4
 * batched solves refactorise per direction, InnerState.h:289-305).  Per frequency: one
 * factorisation, then x, the adjoint l, and per tangent direction i (n_dir of them, complex
 * coefficient directions dcoef[i] = d c / d theta_i, host memory, n_dir x n_stiff complex):
 *   A dx_i = db_i - dA_i x,   A^T dl_i = dG_i(dx_i) - dA_i^T l     (dA_i = sum_k dcoef_ik S_k)
 * Accumulates loss_dev[0] (may be NULL) and w_dev (n_stiff complex) as pfr_sweep, and
 *   h_dev[i * n_stiff + k] += sum_f [ -dl_i^T S_k x + e_k dl_i^T b0 - l^T S_k dx_i ]
 * so that d2L / dtheta_i dtheta_j = Re sum_k ( h_ik dc_kj + w_k d2c_k / dtheta_i dtheta_j ).
 * loss_type must be one of MSE, RMSE, MSE_AFC, MSE_LOG_AFC. */
PFR_API int pfr_hessian_sweep(pfr_solver* s, int32_t nfreq, const double* freqs_dev, int32_t loss_type,
                              const double* ref_dev, double scale, int32_t n_dir, const double* dcoef,
                              double* loss_dev, double* w_dev, double* h_dev, int32_t* flags_dev, void* stream);

/* Backward-error checks of the solves and the accuracy options (the failure detection a static pivot
 * order needs; the reference turns UMFPACK's status into an exception, umfpack_interface.h:10-18, and
 * its solves refine by default).  After each solve the componentwise (Oettli-Prager) backward error
 *   berr = max_i |b - A x|_i / (|A| |x| + |b|)_i        (|z| = |re| + |im|)
 * of the ORIGINAL system is computed on the device per frequency / batch item -- UMFPACK's sparse
 * backward error, invariant under row / column scaling -- and the item's flag
 * PFR_FLAG_BACKWARD_ERROR (forward) / PFR_FLAG_BACKWARD_ERROR_ADJ (adjoint) is set when berr > tol
 * (or not finite).  mode: PFR_CHECK_* bits (0 = off, the default).  berr_dev (device, may be NULL):
 * every later pfr_sweep / pfr_solve call writes berr_dev[2 q] (forward) and berr_dev[2 q + 1]
 * (adjoint) for its items q = 0 .. nfreq - 1 (slots of a solve that is not checked are left
 * alone), so it must hold 2 nfreq doubles of every such call.  With PFR_CHECK_REFINE a loss sweep
 * runs its forward solve, refinement and adjoint in sequence (not the paired top-down pass).
 * PFR_CHECK_CORRECT: every pfr_sweep (forward-only sweeps too) also solves for the adjoint of fr --
 * in symmetric mode inside the paired top-down pass -- and the forward residual walk (the forward
 * check) accumulates the correction; in a loss sweep that adjoint is the loss adjoint up to one
 * scalar per frequency, so the correction costs only the residual walk.  pfr_hessian_sweep applies
 * the correction to its loss and gradient (they equal pfr_sweep's), not the checks; its second-order
 * seeds (the directional derivatives of the loss cotangent) are formed from the uncorrected fr, so its
 * Hessian is that of the uncorrected functional (the two differ by the solve's first-order error). */
PFR_API int pfr_set_check(pfr_solver* s, int32_t mode, double tol, double* berr_dev);
/* PFR_CHECK_REFINE_ADJ threshold: refine the groups where |Re(mu^T r)| > tol |fr| (default 2e-8) */
PFR_API int pfr_set_refine_tol(pfr_solver* s, double tol);

/* Diagnostic: the last chunk's solution vectors of pfr_sweep for chunk lane q (which 0: the forward solution x,
 * 1: the adjoint (mu, the adjoint of fr, under PFR_CHECK_CORRECT; lambda otherwise)), caller numbering, n complex
 * into out_host.  Synchronises the device. */
PFR_API int pfr_debug_solution(pfr_solver* s, int32_t which, int32_t q, double* out_host);

/* Per-phase device times [ms] of the last pfr_sweep/pfr_solve call on this solver, measured with HIP
 * events on the call's stream (0 = factor, 1 = forward solves, 2 = functional, 3 = adjoint solves,
 * 4 = contraction; in a pfr_field_sweep: the gather).  Timing is enabled by pfr_set_timing(s, 1). */
PFR_API int pfr_set_timing(pfr_solver* s, int32_t enable);
PFR_API int pfr_last_timings(const pfr_solver* s, double* ms_out /* 5 */);

/* With pfr_set_timing(s, 3) the factorisation additionally brackets every launch with HIP events:
 * summed device times [ms] of the last call per kernel class (0 = A11 assembly, 1 = A11 LU,
 * 2 = L21/U12 rows/columns, 3 = Schur complement A22 of the large update blocks (16 x 16 LDS
 * blocks, symmetric mode), 4 = Schur complement A22 of the other fronts (4 x 4 tiles)) and their launch
 * counts (NULL allowed). */
PFR_API int pfr_last_kernel_timings(const pfr_solver* s, double* ms_out /* 5 */, int64_t* launches_out /* 5 */);

/* Algorithmic HBM bytes per frequency of one factorisation, per kernel class as above: complex
 * entries each class must store plus the entries it must read once (children's update-matrix
 * entries it gathers, factor blocks it consumes); index data, shared by all frequencies, excluded. */
PFR_API int pfr_solver_alg_bytes(const pfr_solver* s, int64_t* bytes_out /* 5 */);

/* Algorithmic HBM bytes per frequency of the triangular solves of one loss pfr_sweep under the
 * solver's current check mode: factor entries each pass must read (16 B each) plus rhs in / solution
 * out.  Symmetric mode without refinement, functional from the bottom-up passes (PFR_FN_DOT, default):
 * [0] the one bottom-up chain over the fronts the rhs or the loss support reach, [1] the paired top-down
 * pass over every front.  With PFR_FN_DOT=0 (the paired passes): [0] forward bottom-up over the fronts
 * the rhs reaches + forward top-down over the fronts the loss support reaches, [1] adjoint bottom-up
 * over that reach + the single top-down pass that reads every U value once for the adjoint and the
 * rest of the forward solution.  Otherwise [0] / [1] forward / adjoint pair (reached bottom-up + full
 * top-down; with PFR_CHECK_REFINE plus the full correction solve). */
PFR_API int pfr_solver_solve_bytes(const pfr_solver* s, int64_t* bytes_out /* 2 */);

#ifdef __cplusplus
}
#endif

#endif /* PFR_H */
