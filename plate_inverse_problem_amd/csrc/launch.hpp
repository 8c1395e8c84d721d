// Host launchers of the HIP kernels (defined in kernels.hip).
#pragma once

#include "device_types.hpp"

namespace pfr {

// The operator A = K - omega^2 M and the operator right-hand side b = rhsP (beta - omega^2 mass_sum) of the current
// chunk (device pointers; api.cpp builds one per chunk and passes it down).  pop.member != NULL (population sweep): K
// holds the members' operators (stride pop.nnz) and every 64-lane group takes K and beta of its member -- the
// launchers then pick the kernels' POP instantiations.  Explicit-matrix solves read none of K, rhsP and beta.
struct ChunkOp {
  const double2* K = nullptr;
  const double* M = nullptr;
  const double* freqs = nullptr;  // chunk frequencies (padded)
  const double* rhsP = nullptr;   // permuted Dirichlet vector
  double beta_re = 0, beta_im = 0, mass_sum = 0;
  PopArgs pop;
};

// The integer codes of the launchers by name.  The values are the kernels' template values (MODE, RHS) and the
// solver's reach indices: a launcher maps an enumerator to the instantiation, the kernels keep their int parameters.
enum Tri { TRI_L = 0, TRI_U = 1, TRI_UT = 2, TRI_LT = 3 };   // triangular pass: L, U^T bottom-up; U, L^T top-down
// right-hand-side source: the operator's, an explicit batch B, a permuted vector G, the operator's with the
// Dirichlet corrections in their slots (symmetric mode with coupled rows)
enum Rhs { RHS_OPERATOR = 0, RHS_BATCH = 1, RHS_VECTOR = 2, RHS_OPERATOR_DIR = 3 };
// the fronts a solve visits: all, the rhs reach, the functional support's reach (SolverView::d_reach)
enum Reach { REACH_ALL = -1, REACH_RHS = 0, REACH_SUPPORT = 1 };
enum Mat { MAT_OPERATOR = 0, MAT_BATCH = 1 };                // matrix source: the chunk operator, an explicit batch

// the first launch configuration refused since the last call (a kernel's dynamic LDS size), NULL: none; the
// refused launch was skipped
const char* launch_refused();

void launch_combine(const double* stiff, int n_stiff, int64_t nnz, const CoefPack& coef, double2* K, hipStream_t st);
// K[m * nnz + nz] for n_members coefficient rows (coef: device, n_members x n_stiff; n_stiff 12 or 18), each
// bitwise launch_combine's K
void launch_combine_batch(const double* stiff, int n_stiff, int64_t nnz, const double2* coef, int n_members,
                          double2* K, hipStream_t st);
// MAT_OPERATOR: the operator op (a population sweep's: every 64-lane group assembled from its member's K; so too in
// launch_front0 / launch_offdiag); MAT_BATCH: the explicit batch (data, ds, nvalid)
void launch_assemble(Mat mode, const int4* recs, int nrec, const int* xptr, const int2* xl, int ngroups, double2* F,
                     int64_t Fc, const ChunkOp& op, const double2* data, int64_t ds, int nvalid, hipStream_t st);
// The launchers of a tree level take the level's record of the solver's schedule (plan.hpp: FactorLevel, PairLevel,
// ChainLevel, SolveLevel) and only map it to a kernel instantiation, grid and block.
// A11 LU of a level: r.G lane groups per wave of the symmetric kernel, r.waves waves
void launch_factor(bool sym, const DevPattern& P, const int* lvl, const FactorLevel& r, int ngroups, double2* F, int64_t Fc,
                   int* flags, hipStream_t st);
// symmetric A11 LU with the pivot block in LDS (one front x one frequency per workgroup); r.maxns, the level's
// largest pivot block, sizes the dynamic LDS (fac_lds_bytes)
void launch_factor_lds(const DevPattern& P, const int* lvl, const FactorLevel& r, double2* F, int64_t Fc, int* flags,
                       hipStream_t st);
// the bottom level fused (k_front0, Plan::fused0): fl = level-0 fronts, the first r.f0_small with <= 2 pivots
void launch_front0(const DevPattern& P, const int* fl, const FactorLevel& r, const int* fptr, const int* fnz,
                   int ngroups, double2* F, int64_t Fc, const ChunkOp& op, int* flags, hipStream_t st);
// L21 rows (and U12 columns in general mode) of a level's items; r.off_pu 3: the software-pipelined prefix
// (operator-form launches)
void launch_offdiag(Mat mode, const DevPattern& P, const int4* items, const FactorLevel& r, const int2* orec,
                    const int* oxp, const int2* ox, int ngroups, double2* F, int64_t Fc, const ChunkOp& op,
                    const double2* data, int64_t ds, int nvalid, hipStream_t st);
// Schur complement A22 -= L21 U12 for a level's tile list (TM x TN = 4 x 4 tiles)
void launch_schur(bool sym, const DevPattern& P, const int4* tiles, int ntiles, const int* g1, const int* gxp,
                  const int2* gx, int ngroups, double2* F, int64_t Fc, hipStream_t st);
// symmetric mode, large update blocks: 16 x 16 blocks, operands staged in LDS per workgroup
void launch_schur_blk(const DevPattern& P, const int4* blocks, int nblocks, const int* bg1, const int* bgxp,
                      const int2* bgx, int ngroups, double2* F, int64_t Fc, hipStream_t st);
// r.split_L / r.split_U > 1 (L and U solves): the update part of every front (L: the update rows; U: the pivot rows'
// products with the update-row solution) runs first / last over that many workgroups of SPLIT_W waves per
// (front, frequency group) -- the top levels' few fronts otherwise pull their L21 blocks through one CU each
// glist (may be NULL): the groups to solve, REFINE_CAP of them (-1: none), indexed by grid row (pass
// ngroups = REFINE_CAP); the selective adjoint refinement's solves
// pop (the chunk operator's): a population sweep's L solve of the operator rhs (RHS_OPERATOR / _DIR) takes its POP form
void launch_solve(Tri which, Rhs rhs_mode, bool sym, const DevPattern& P, const int* lvl, const SolveLevel& r, int ngroups,
                  const double2* F, int64_t Fc, double2* WV, const RhsArgs& rd, const PopArgs& pop, const double2* Yin,
                  double2* Out, const int* reach, hipStream_t st, const int* glist = nullptr);
// nslices (<= 4) bottom-up L solves as one chain of launches (blockIdx.z = slice; slice z: the fronts
// lvl[z][0 .. r.nf0 or r.nf1), its work vectors WV[z], rhs rd[z] (RHS_OPERATOR or _DIR for every slice), solution Y[z]);
// pop (population sweep): slice 0's rhs with the member's beta
void launch_lsolve_multi(Rhs rhs_mode, const DevPattern& P, int nslices, const int* const* lvl, const ChainLevel& r,
                         int ngroups, const double2* F, int64_t Fc, double2* const* WV, const RhsArgs* rd,
                         const PopArgs& pop, double2* const* Y, const int* const* reach, hipStream_t st);
// functional from the bottom-up passes: partial dot products (FN_PARTS x 3 x Fc), the functional / loss
// / cotangent from them (fcoef: 3 x Fc, G at the support rows), and L^-1 g = sum_k c_k L^-1 a_k in Yk[0]
void launch_fn_dot(const int2* rows, int nrows, const double2* F, const double2* Yb, const double2* const* Yk, int64_t Fc,
                   double2* parts, hipStream_t st);
void launch_functional_fn(const FunctionalArgs& A, const double2* parts, int64_t Fc, int nvalid, int64_t q0,
                          double* fr_out, double* loss_terms, double2* G, double2* fcoef, hipStream_t st);
void launch_fn_combine(const int* rows, int nrows, const double2* fcoef, double2* const* Yk, int64_t Fc, hipStream_t st);
// two top-down U solves in one pass (vector 0 skipped on the fronts flagged in skip0), symmetric mode
void launch_usolve2(const DevPattern& P, const int* lvl, const PairLevel& r, int ngroups, const double2* F, int64_t Fc,
                    const double2* Y0, double2* X0, const int* reach0, const int* skip0, const double2* Y1, double2* X1,
                    const int* reach1, hipStream_t st);
// Hessian sweep: tangent right-hand sides (rows of the permuted matrix, or of its
// transpose with accumulate = 1) and the directional derivative of the loss cotangent
void launch_tangent_spmv(const int* ptr, const int* idx, const int* nzs, int nrows, const double2* Kd,
                         const double2* X, int64_t Fc, const double* rhsP, double2 beta, double2* Y, int accumulate,
                         hipStream_t st);
void launch_functional_tangent(const FunctionalArgs& A, const double2* X, const double2* DX, int64_t Fc, int nvalid,
                               int64_t q0, double2* G, hipStream_t st);
void launch_functional(const FunctionalArgs& A, const double2* X, int64_t Fc, int nvalid, int64_t q0, double* fr_out,
                       double* loss_terms, double2* G, hipStream_t st);
// gradient contraction with the frequency sum first (one partial per workgroup: contract_eg_parts of them)
// msc (may be NULL): per-frequency factor of Lam (functional correction: the loss cotangent scale)
void launch_contract_eg(const int4* ent, int nent, const double* se, int n_stiff, const double2* Lam, const double2* X,
                        int64_t Fc, int nvalid, double2* partial, hipStream_t st, const double2* msc = nullptr);
// entry-ordered copy of the stiffness matrices (se)
void launch_gather_entries(const int4* ent, int nent, const double* stiff, int ns, double* se, hipStream_t st);
// the stiffness table compacted to the nl matrices of `live` (se_live[nz * nl + i]) on the entries of the rows of a
// walk list (rows ptr / nzs: the permuted matrix by rows); *bad = 1 on a non-zero value of another matrix there
void launch_gather_live(const int* walk, int n, const int* ptr, const int* nzs, const double* stiff, int ns,
                        unsigned live, int nl, double* se_live, int* bad, hipStream_t st);
void launch_rhs_dot(const int* sup, const double* val, int n_sup, const double2* Lam, int64_t Fc, double2* t_out,
                    hipStream_t st, const double2* msc = nullptr);
// w_out[k] += -sum(partial[., k]) + e_k sum_q t_q ;  loss_out += sum_q loss_terms (q < nvalid)
void launch_reduce(const double2* partial, int nparts, int n_stiff, const double2* t_q, const CoefPack& e,
                   const double* loss_terms, int nvalid, int64_t Fc, double2* w_out, double* loss_out,
                   hipStream_t st);
// Jacobian sweep.  launch_contract_q: the per-frequency contraction in k_residual's kpart layout,
// kpart[(b n_stiff + k) Fc + q] over contract_q_parts(n, nent) workgroups b (entries and se as launch_contract_eg).
// launch_jac_finish: jc[q n_stiff + k] = -msc[q] sum_b kpart[b][k][q] + e_k t_q[q] for the chunk's rows q < nvalid
// (jc: the chunk's first row; msc NULL: 1; written, not accumulated)
void launch_contract_q(const int4* ent, int nent, const double* se, int n_stiff, const double2* Lam, const double2* X,
                       int n, int64_t Fc, double2* kpart, hipStream_t st);
void launch_jac_finish(const double2* kpart, int nparts, int n_stiff, const double2* msc, const double2* t_q,
                       const CoefPack& e, int nvalid, int64_t Fc, double2* jc, hipStream_t st);
// Inertia sweep.  launch_gather_mass: me[e MASS_NM + j] = mass[nz(e) n_mass + j], the entry-ordered copy of the n_mass
// mass components (columns j >= n_mass zero) over ent[0 .. nent).  launch_inertia_rows: k_contract_mass over a view's
// list and per-wave batch ranges (plan.hpp, mass_entries) into mpart[(b MASS_NM + j) Fc + q] over
// contract_mass_parts(n, nent) workgroups b, then k_inertia_finish:
//   jm[q n_mass + j] = omega_q^2 (msc[q] sum_b mpart[b][j][q] - d_j t_q[q])   for the chunk's rows q < nvalid
// (jm: the chunk's first row; msc NULL: 1; omega_q = 2 pi freqs[q]; written, not accumulated)
void launch_gather_mass(const int4* ent, int nent, const double* mass, int n_mass, double* me, hipStream_t st);
void launch_inertia_rows(const int* list, const int* ptr, const int4* ent, int nent, const double* me, int n_mass,
                         const double2* Lam, const double2* X, int n, int64_t Fc, double2* mpart, const double2* msc,
                         const double2* t_q, const double* freqs, const MassWeights& d, int nvalid, double2* jm,
                         hipStream_t st);
// symmetric mode: forward right-hand-side corrections (RHS_OPERATOR: operator rhs -> Bc; RHS_VECTOR: G in
// place) and the adjoint's Dirichlet rows (X in place); pop (population sweep): K and the rhs scale of the
// group's member
void launch_dirichlet_rhs(Rhs src, const DirArgs& d, const PopArgs& pop, int n_crow, const RhsArgs& rd, double2* G,
                          double2* Bc, int64_t Fc, hipStream_t st);
void launch_dirichlet_post(const DirArgs& d, const PopArgs& pop, int n_dir, double2* X, int64_t Fc, hipStream_t st,
                           const int* glist = nullptr);
// Backward-error check: the original system's rows (forward) or columns (adjoint) in the permuted
// numbering, A = K - omega^2 M (MAT_OPERATOR) or the explicit batch (MAT_BATCH); rhs RHS_OPERATOR, RHS_BATCH or
// RHS_VECTOR.  The per-frequency componentwise backward error accumulates in acc (max, zero on
// entry); acc == NULL: only the residual is written to R.
// n_stiff (12 or 18, with a.se / a.kpart; else 0): the gradient contraction fused into the forward walk (MAT_OPERATOR,
// RHS_OPERATOR, Mu != NULL) over the matrices of a.live (all n_stiff, or 6 or 12 live ones with a.se compacted to them:
// the other slots of kpart are written as zeros; any other count is refused).  unroll: entries per gather batch of
// the adjoint check walk and of the six-matrix contraction walk (4 or 8; the same bits).
// pop (population sweep, MAT_OPERATOR): K and beta of the group's member.
// Mu != NULL (MAT_OPERATOR, RHS_OPERATOR): also the functional-correction dot products sum_p Mu_p r_p, one partial
// per workgroup and frequency in cpart (residual_parts(n) x Fc), summed by launch_correct_finish
void launch_residual(Mat mode, Rhs rhs, const ResidArgs& a, int n_stiff, int unroll, const PopArgs& pop, const double2* X,
                     int64_t Fc, double2* R, double* acc, hipStream_t st, const double2* Mu = nullptr,
                     double2* cpart = nullptr);
// partial[t * n_stiff + k] = sum_{q in tile t} msc[q] sum_b kpart[b][k][q] (msc NULL: 1; tiles of 64
// frequencies): the fused walk's contraction as Fc / 64 parts
void launch_reduce_q(const double2* kpart, int nparts, int n_stiff, const double2* msc, int nvalid, int64_t Fc,
                     double2* partial, hipStream_t st);
// corrected fr (fr_out, global index; may be NULL), loss terms and cotangent scales of a chunk
// gind != NULL: per 64-frequency group its largest |correction| / |fr| (launch_select_groups picks from them)
// tq != NULL: t_q = mu^T rhsP in, m_q t_q out, and the solve-error scale in m_q (k_correct_finish) from op's
// rhs scale (population sweep: with the beta of the group's member)
void launch_correct_finish(const FunctionalArgs& A, const double* fr0, const double2* cpart, int nparts, int64_t Fc,
                           int nvalid, int64_t q0, double* fr_out, double* loss_terms, double2* mscale,
                           const ChunkOp& op, hipStream_t st, double* gind = nullptr, double2* tq = nullptr);
// One residual walk as a value: which system of the original matrix, which matrix and right-hand side, the solution X
// (permuted, frequency-minor), which groups, and exactly one of three outputs.  Built by residual, checked or
// correction (+ on_batch / on_groups); the solver maps it to launch_residual and launch_berr_finish.
struct Walk {
  enum Sys { FORWARD = 0, ADJOINT = 1 };   // A x = b over the rows; A^T l = g over the columns
  Sys sys = FORWARD;
  Mat mat = MAT_OPERATOR;                // the chunk operator, or the explicit batch (data, ds)
  const double2* data = nullptr;
  int64_t ds = 0;
  Rhs rhs = RHS_OPERATOR;                // operator, explicit B or vector G, in rd
  RhsArgs rd;
  const double2* X = nullptr;
  const int* glist = nullptr;            // the groups walked (REFINE_CAP of them; NULL: every group)
  double2* R = nullptr;                  // output 1: the residual b - A x (a refinement step); nothing is checked
  bool check = false;                    // output 2: the backward error -> the chunk's flags and (q0 >= 0) the caller's
  int64_t q0 = -1;                       //           berr slots from q0 on
  const double2* Mu = nullptr;           // output 3: the functional correction's dot products with Mu, with `check`
  bool contract = false;                 //           too if asked, and with the gradient contraction fused in
  static Walk residual(Sys sys, Rhs rhs, const RhsArgs& rd, const double2* X, double2* R) {
    return {.sys = sys, .rhs = rhs, .rd = rd, .X = X, .R = R};
  }
  static Walk checked(Sys sys, Rhs rhs, const RhsArgs& rd, const double2* X, int64_t q0) {
    return {.sys = sys, .rhs = rhs, .rd = rd, .X = X, .check = true, .q0 = q0};
  }
  // the forward walk of the operator system (rd: the operator's rhs)
  static Walk correction(const RhsArgs& rd, const double2* X, const double2* Mu, bool check, int64_t q0, bool contract) {
    return {.rd = rd, .X = X, .check = check, .q0 = q0, .Mu = Mu, .contract = contract};
  }
  Walk& on_batch(const double2* d, int64_t stride) { mat = MAT_BATCH; data = d; ds = stride; return *this; }
  Walk& on_groups(const int* g) { glist = g; return *this; }
};
// glist[0 .. REFINE_CAP): the groups with the largest indicators above tol, largest first, -1 past them
void launch_select_groups(const double* gind, int ngroups, double tol, int* glist, hipStream_t st);
// flags |= flag where acc[q] > tol (or not finite); acc cleared
void launch_berr_finish(double* acc, int64_t Fc, int nvalid, double tol, int flag, int* flags, double* berr_out,
                        int64_t q0, int which, hipStream_t st);
void launch_axpy_vec(double2* X, const double2* D, int64_t count, hipStream_t st, const int* glist = nullptr,
                     int64_t Fc = 64);
void launch_scale_vec(double2* X, const double2* m, int n, int64_t Fc, hipStream_t st);
void launch_unpermute(const int* perm, int n, const double2* X, int64_t Fc, int nvalid, double2* out, hipStream_t st);
// pfr_field_sweep's way out: out[q * n_sel + j] = X[sel[j] * Fc + q] for q < nvalid, j < n_sel (sel: permuted rows,
// each in [0, n); out: the chunk's first row of the caller's frequency-major array).  Tiles of 64 frequencies x
// FIELD_R selected rows through LDS; nothing outside [0, nvalid) x [0, n_sel) is stored.
constexpr int FIELD_R = 32;
void launch_field_gather(const int* sel, int n_sel, const double2* X, int64_t Fc, int nvalid, double2* out,
                         hipStream_t st);
// pfr_field_loss_sweep between the forward solve and the adjoint: the loss PFR_LOSS_F* on the selected rows of X against
// ref (the chunk's first row of the caller's frequency-major array; wts NULL: all 1) and its seed into G (zeroed by the
// caller): G[sel[j] * Fc + q] = scale g_j, loss_terms[q] = scale term_q (both zero for q >= nvalid).  fpart:
// field_loss_parts(loss, n_sel, Fc) doubles, fc: 3 x Fc doubles (both unused by FCOTANGENT, which writes scale * ref and
// leaves loss_terms alone).  sel must hold no row twice (the seed is a scatter).
struct FieldLossArgs {
  int32_t loss_type = 0;
  const int32_t* sel = nullptr;
  const double* wts = nullptr;
  int32_t n_sel = 0;
  const double2* ref = nullptr;
  double scale = 1.0;
};
inline int field_loss_tiles(int n_sel) { return (n_sel + FIELD_R - 1) / FIELD_R; }
// the sums a loss keeps per tile and frequency, and the partial buffer's doubles for a selection
constexpr int field_nsum(int loss) {
  return loss == PFR_LOSS_FMSE ? 1 : loss == PFR_LOSS_FRMSE ? 2 : loss == PFR_LOSS_FMAC ? 4 : 0;
}
inline int64_t field_loss_parts(int loss, int n_sel, int64_t Fc) {
  return (int64_t)field_loss_tiles(n_sel) * field_nsum(loss) * Fc;
}
void launch_field_loss(const FieldLossArgs& a, const double2* X, int64_t Fc, int nvalid, double2* G, double* fpart,
                       double* loss_terms, double* fc, hipStream_t st);
void launch_matvec(const int* colptr, const int* rowind, int n, const double2* data, int64_t ds, const double2* x,
                   int64_t xs, double2* y, int transpose, int batch, hipStream_t st);
// a chunk's frequencies (padded with the last) and its flags cleared, one kernel
void launch_chunk_start(double* freqs, const double* src, int nvalid, int64_t Fc, int* flags, hipStream_t st,
                        double* loss = nullptr, double* w = nullptr, int nw = 0, int* out_flags = nullptr,
                        double* berr = nullptr, int nfreq = 0);
// p[0 .. n) = 0 (complex entries)
void launch_zero(double2* p, int64_t n, hipStream_t st);
void launch_flags_merge(const int* chunk, int nvalid, int* out, hipStream_t st);

}  // namespace pfr
