// Types shared by the host launchers and the HIP kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pfr.h"
#include "plan.hpp"
#include "symbolic.hpp"

namespace pfr {

// Device copy of the symbolic maps (all pointers are device pointers).
struct DevPattern {
  const Front* fronts;
  const int32_t* idx;
  const int32_t* relpos;
  const int32_t* row_front;
  const int32_t* asm_ptr;
  const int32_t* asm_col;
  const int32_t* asm_nz;
  const int32_t* ea_ptr;
  const int32_t* ea_src;
  const int32_t* perm;
  const int32_t* prow;
  const int32_t* pcol;
  int32_t n;
};

constexpr int COEF_MAX = 32;
struct CoefPack {
  double re[COEF_MAX];
  double im[COEF_MAX];
};

// The load weights d_j of the mass components (pfr_set_inertia; k_inertia_finish)
struct MassWeights {
  double d[4];
};

// Population sweep (pfr_population_sweep): the 64-lane group g of the chunk belongs to member[g]; its operator is
// K + member[g] * nnz and its rhs scale beta[member[g]].  Read only by the kernels' POP instantiations.
struct PopArgs {
  const int32_t* member = nullptr;   // the chunk's group table (device, Fc / 64 entries)
  const double2* beta = nullptr;     // per member (device)
  int64_t nnz = 0;                   // stride of the members' K
};

// b = rhsP * (beta_re - omega^2 mass_sum + i beta_im) per frequency (the rhs of a sweep's solves)
struct RhsScale {
  const double* freqs = nullptr;   // chunk-local frequencies [Hz]
  double mass_sum = 0, beta_re = 0, beta_im = 0;
};

// Right-hand side of a solve, by the kernels' RHS template value (kernels.hip, "right-hand sides"); the host fills
// the fields of the form it launches
struct RhsArgs {
  const double* rhsP = nullptr;   // RHS 0: permuted Dirichlet vector
  double beta_re = 0, beta_im = 0, mass_sum = 0;
  const double* freqs = nullptr;  // chunk frequencies (padded)
  const double2* B = nullptr;     // RHS 1: explicit batch (batch-major, caller numbering)
  int64_t b_stride = 0;
  const double2* G = nullptr;     // RHS 2: permuted frequency-minor vector
  int nvalid = 1;                 // RHS 1: padded lanes repeat the last valid item
  const int* cslot = nullptr;     // RHS 3: coupled-row slot of each permuted row (or -1)
  const double2* Bc = nullptr;    // RHS 3: Dirichlet corrections, slot-major (slot * Fc + q)
};

// Dirichlet decoupling lists of a symmetric-mode solver + the operator (kernels.hip, "Dirichlet decoupling")
struct DirArgs {
  const int2* dir = nullptr;      // per Dirichlet node: (permuted node, diagonal entry)
  const int* crow = nullptr;      // coupled rows (permuted)
  const int* cptr = nullptr;      // entry range of each coupled row in ce
  const int2* ce = nullptr;       // (Dirichlet slot, entry)
  const int* dptr = nullptr;      // entry range of each Dirichlet node in de
  const int2* de = nullptr;       // (permuted row, entry)
  const double2* K = nullptr;
  const double* M = nullptr;
  const double* freqs = nullptr;
};

// The residual walk (k_residual): the original system's rows or columns in the permuted numbering, the operator
// (mode 0) or the explicit batch (mode 1), and the right-hand side (0 operator, 1 explicit B, 2 vector G)
struct ResidArgs {
  const int* ptr = nullptr;
  const int* idx = nullptr;
  const int* nzs = nullptr;
  int n = 0;
  const double2* K = nullptr;
  const double* M = nullptr;
  const double* freqs = nullptr;
  const double2* data = nullptr;
  int64_t data_stride = 0;
  int nvalid = 1;
  const double* rhsP = nullptr;
  double beta_re = 0, beta_im = 0, mass_sum = 0;
  const double2* B = nullptr;
  int64_t b_stride = 0;
  const int* perm = nullptr;
  const double2* G = nullptr;
  const int* walk = nullptr;      // rows in walk order (original numbering: mesh-local gathers of X)
  const double* se = nullptr;     // NSK > 0: stiffness values, nz-major (se[nz * NSK + i]: the i-th live matrix)
  double2* kpart = nullptr;       // NSK > 0: per (workgroup, k, frequency) sums of S_k(nz) mu_row x_col, k < nslot
  unsigned live = 0;              // NSK > 0: bit k set for the NSK matrices se holds, in order (the others: zeros out)
  int nslot = 0;                  // NSK > 0: the stiffness matrices of kpart's layout (n_stiff >= NSK)
  const int* glist = nullptr;     // the groups to walk, indexed by grid row (REFINE_CAP, -1: none; NULL: grid row = group)
};

// internal loss id of pfr_jacobian_sweep: d L / d fr_q = 1 for every frequency, no reference (never accepted from
// a caller of pfr_sweep)
constexpr int LOSS_UNIT = PFR_LOSS_COTANGENT + 1;

struct FunctionalArgs {
  // the complex response H = axis . (ts U, ts V, W) (pfr_sweep_complex; the kernels' CPX forms, which read none of
  // fr0).  In front of the magnitude's fields: k_functional_fn fetches ref .. fr0 and the kernel argument after this
  // struct with one scalar load, which fields behind fr0 would split (48 bytes here move the offsets only)
  int32_t cpx;            // != 0: the launchers take the CPX forms; loss_type PFR_LOSS_C*, LOSS_UNIT or -1
  double axis[3];         // real sensing axis (dU, dV, dW)
  double2* h_out;         // H per frequency, indexed by global frequency (may be NULL)
  double2* h0;            // != NULL: seed mode: H of the solve -> h0, G = a_d = d H / d x; k_correct_finish reads it
  int32_t n_support;
  const int32_t* pidx;    // permuted DOF index of each support entry (device)
  const double* a;        // [aU | aV | aW], 3 * n_support (device)
  double ts;              // transverse sensitivity
  int32_t loss_type;      // PFR_LOSS_* or -1 (forward only)
  const double2* ref;     // reference FR (complex) or cotangent (re), indexed by global frequency
  double scale;           // 1 / F_total (mean over the whole sweep)
  double* fr0;            // != NULL: seed mode of k_functional (functional correction): fr of the solve -> fr0,
                          // G = d fr / d x (no loss terms); k_correct_finish forms the corrected fr and the loss
};

}  // namespace pfr
