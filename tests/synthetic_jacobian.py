"""The per-frequency Jacobian rows of pfr_jacobian_sweep on the synthetic fronts of ``synthetic.py`` (test
infrastructure, not a test): the extended-precision reference rows and the errors of the fp64 multifrontal model and
of the unrefined dense LU against them, from which the GPU tests' bounds come.

    jc[q][k] = -mu_q^T S_k x_q + e_k mu_q^T rhs,   A_q^T mu_q = d fr_q / d x_q        (include/pfr.h)

i.e. ``synthetic.partials(op, mu_q, x_q)``: the w of a unit cotangent at frequency q alone.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla

import synthetic as sy


def jacobian_reference(refc: sy.Reference) -> np.ndarray:
    """Rows (nfreq, n_stiff) in extended precision from the refined x_q and the refined adjoint of fr at x_q.
    Cached on the operator."""
    op = refc.op
    key = ("jac", refc.freqs.tobytes())
    if key not in op._cache:
        rows = []
        for q in range(refc.freqs.size):
            mu = sy.refined_solve(refc.mats[q], sy.adjoint_seed(op, refc.x[q], sy.LD(1)), refc.lus[q], trans=True)[0]
            rows.append(sy.partials(op, mu, refc.x[q]))
        op._cache[key] = np.array(rows)
    return op._cache[key]


def fr_at(op: sy.Operator, freqs, coef_ld) -> np.ndarray:
    """fr (extended precision) of the operator with the coefficients ``coef_ld`` (not rounded: K = coef S and
    beta = coef e formed in extended precision) at ``freqs``: what the rows are the derivative of."""
    K = op.pat.dense(coef_ld @ op._ld("S"))
    beta = coef_ld @ op.e.astype(sy.LD)
    out = []
    for f in freqs:
        om2 = sy.LD(op.om2(f))
        A = K - om2 * op._ld("M")
        b = op.rhs.astype(sy.LD) * (beta - om2 * sy.LD(op.mass_sum))
        out.append(sy.fr_of(op, sy.refined_solve(A, b)[0])[0])
    return np.array(out)


def row_errors(rows, ref) -> float:
    """max over the rows q of max_k |row_k - ref_k| / max_k |ref_k|."""
    rows, ref = np.asarray(rows, dtype=sy.CLD), np.asarray(ref, dtype=sy.CLD)
    return float(np.max(np.max(np.abs(rows - ref), axis=1) / np.max(np.abs(ref), axis=1)))


def _rows_of(op, solve_q, freqs, sel, refc, correct, scale_corr, refine=False):
    """(fr, rows) over ``sel`` of the sweep's sequence in fp64 with ``solve_q(q)(v, transpose)``: forward solve, the
    adjoint of fr at that x; with ``correct`` fr += Re(mu^T r) (r = b - A x in extended precision rounded to fp64, as
    the compensated walk forms it) and lam = m mu with m = 1 or, with ``scale_corr``, fr / (mu^T b - mu^T r);
    ``refine`` (PFR_CHECK_REFINE): one refinement step of x and of mu (synthetic._refine_step)."""
    frs, rows = [], []
    for q in sel:
        solve = solve_q(q)
        b_ld = op.b_ld(freqs[q])
        b = b_ld.astype(np.complex128)
        x = solve(b, False)
        if refine:
            x = sy._refine_step(solve, refc.mats[q], b_ld, x, False)
        fr = sy.fr_of(op, x)[0]
        g = sy.adjoint_seed(op, x, 1.0)
        mu = solve(g, True)
        if refine:
            mu = sy._refine_step(solve, refc.mats[q], g, mu, True)
        lam = mu
        if correct:
            r = (b_ld - refc.mats[q] @ x.astype(sy.CLD)).astype(np.complex128)
            d = mu @ r
            fr = fr + d.real
            if scale_corr:
                lam = (fr / (mu @ b - d)) * mu
        frs.append(fr)
        rows.append(sy.partials(op, lam, x))
    return np.array(frs), np.array(rows)


def jacobian_model_errors(op: sy.Operator, sym, freqs, symmetric=True, correct=False, scale_corr=True, refine=False):
    """e_model and e_dense of the rows and of fr against the reference, over EVERY frequency: the same sequence in
    fp64 through the multifrontal model (synthetic._model_solver) and through the unrefined dense LU.  Returns
    (e_model, e_dense), dicts with "jc" (row_errors) and "fr" (max relative error)."""
    refc = sy.reference(op, freqs)
    ref = jacobian_reference(refc)
    sel = list(range(len(freqs)))
    out = []
    for which in ("model", "dense"):
        if which == "model":
            solve_q = lambda q: sy._model_solver(op, sym, freqs[q], symmetric)                          # noqa: E731
        else:
            solve_q = lambda q: (lambda v, tr: sla.lu_solve(refc.lus[q], v, trans=1 if tr else 0))      # noqa: E731
        frs, rows = _rows_of(op, solve_q, freqs, sel, refc, correct, scale_corr, refine)
        out.append({"jc": row_errors(rows, ref),
                    "fr": float(np.max(np.abs(frs.astype(sy.LD) / refc.fr[sel] - 1)))})
    return out[0], out[1]


def bounds(e_model, e_dense):
    """The project's rule: 10 x max(e_model, e_dense, FLOOR) per quantity."""
    return sy.bounds(e_model, e_dense)
