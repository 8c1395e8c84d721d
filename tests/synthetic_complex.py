"""The complex response sweeps (pfr_sweep_complex, pfr_jacobian_sweep_complex) on the synthetic fronts of
``synthetic.py`` (test infrastructure, not a test; mirrors ``synthetic_jacobian.py``): the extended-precision
reference and the errors of the fp64 multifrontal model and of the unrefined dense LU against it, from which the GPU
tests' bounds come.

    H_q = a_d . x_q,   a_d = ts dU aU + ts dV aV + dW aW                      (include/pfr.h; linear in x)
    term, g of the three losses (d term = Re(g dH)):
        MSE_COMPLEX      |H - ref|^2                  g = 2 conj(H - ref)
        RMSE_COMPLEX     |H - ref|^2 / |ref|^2        g = 2 conj(H - ref) / |ref|^2
        MSE_LOG_COMPLEX  |z|^2, z = log(H / ref)      g = 2 conj(z) / H      (principal branch)
        CCOTANGENT       none                         g = the caller's dL/dH
    w_k = sum_q (-lam_q^T S_k x_q + e_k lam_q^T rhs),  A^T lam_q = g_q a_d;   rows jc[q] = the same with A^T mu = a_d
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import scipy.linalg as sla

import synthetic as sy
import synthetic_jacobian as sj

AXES = ((0.0, 0.0, 1.0), (0.6, 0.8, 1.0))
LOSSES = ("MSE_COMPLEX", "RMSE_COMPLEX", "MSE_LOG_COMPLEX")
MODEL_EVERY = 6                                   # the model's sample of a sweep, as the Jacobian tests'


def a_d(op: sy.Operator, axis, ext):
    """The sensing vector (n,): ts dU aU + ts dV aV + dW aW, in extended precision or fp64."""
    a = op._ld("a") if ext else op.a_full()
    T = sy.LD if ext else np.float64
    d = [T(v) for v in axis]
    return T(op.ts) * d[0] * a[0] + T(op.ts) * d[1] * a[1] + d[2] * a[2]


def loss_c(H, ref, loss_type):
    """(term, g) of one frequency in the precision of ``H`` (extended, or fp64 as fp64 code forms them)."""
    ext = np.asarray(H).dtype == sy.CLD
    C, T = (sy.CLD, sy.LD) if ext else (np.complex128, np.float64)
    H, ref = C(H), C(ref)
    if loss_type == "MSE_COMPLEX":
        z = H - ref
        return abs(z) ** 2, 2 * np.conj(z)
    if loss_type == "RMSE_COMPLEX":
        z, r2 = H - ref, abs(ref) ** 2
        return abs(z) ** 2 / r2, 2 * np.conj(z) / r2
    if loss_type == "MSE_LOG_COMPLEX":
        p = H * np.conj(ref)
        z = C(np.log(abs(H)) - np.log(abs(ref))) + C(1j) * np.arctan2(p.imag, p.real)
        return abs(z) ** 2, 2 * np.conj(z) / H
    if loss_type == "CCOTANGENT":
        return T(0), ref
    raise ValueError(loss_type)


@dataclass(eq=False)
class ComplexReference:
    refc: sy.Reference
    axis: tuple
    H: np.ndarray             # (nfreq,) extended
    ref: np.ndarray           # (nfreq,) complex128: the sweep's reference, H * 1.02 e^{0.1i} rounded
    cot: np.ndarray           # (nfreq,) complex128: a fixed-seed complex dL/dH (PFR_LOSS_CCOTANGENT)
    mu: np.ndarray            # (nfreq, n) extended: A^T mu = a_d
    rows: np.ndarray          # (nfreq, n_stiff) extended: partials(op, mu_q, x_q)
    _loss: dict = field(default_factory=dict)

    def sweep_ref(self, loss_type):
        return None if loss_type == "NONE" else self.cot if loss_type == "CCOTANGENT" else self.ref

    def loss(self, loss_type):
        """Per-frequency terms, g, lam = refined_solve(A^T, g a_d) and partials w, in extended precision."""
        if loss_type not in self._loss:
            op, refc = self.refc.op, self.refc
            ad = a_d(op, self.axis, True)
            terms, gs, ws = [], [], []
            for q in range(refc.freqs.size):
                term, g = loss_c(self.H[q], self.sweep_ref(loss_type)[q], loss_type)
                lam = sy.refined_solve(refc.mats[q], g * ad, refc.lus[q], trans=True)[0]
                terms.append(term)
                gs.append(g)
                ws.append(sy.partials(op, lam, refc.x[q]))
            self._loss[loss_type] = {"terms": np.array(terms), "g": np.array(gs), "w": np.array(ws)}
        return self._loss[loss_type]


def reference(op: sy.Operator, freqs, axis) -> ComplexReference:
    """The complex reference of the operator-form case at ``freqs`` along ``axis`` (cached on the operator)."""
    refc = sy.reference(op, freqs)
    axis = tuple(float(v) for v in axis)
    key = ("cpx", refc.freqs.tobytes(), axis)
    if key not in op._cache:
        ad = a_d(op, axis, True)
        H = np.array([ad @ x for x in refc.x])
        ref = (H * (sy.LD(1.02) * np.exp(sy.CLD(0.1j)))).astype(np.complex128)
        rng = np.random.default_rng(6100)
        cot = (0.5 + rng.random(freqs.size)) * np.exp(2j * np.pi * rng.random(freqs.size))
        mu = np.array([sy.refined_solve(m, ad, lu, trans=True)[0] for m, lu in zip(refc.mats, refc.lus)])
        rows = np.array([sy.partials(op, mu[q], refc.x[q]) for q in range(refc.freqs.size)])
        op._cache[key] = ComplexReference(refc, axis, H, ref, cot, mu, rows)
    return op._cache[key]


def h_at(op: sy.Operator, freqs, coef_ld, axis) -> np.ndarray:
    """H (extended precision) of the operator with the coefficients ``coef_ld`` at ``freqs``, formed as
    ``synthetic_jacobian.fr_at`` forms fr (K = coef S and beta = coef e in extended precision, not rounded)."""
    K = op.pat.dense(coef_ld @ op._ld("S"))
    beta = coef_ld @ op.e.astype(sy.LD)
    ad = a_d(op, axis, True)
    out = []
    for f in freqs:
        om2 = sy.LD(op.om2(f))
        A = K - om2 * op._ld("M")
        b = op.rhs.astype(sy.LD) * (beta - om2 * sy.LD(op.mass_sum))
        out.append(ad @ sy.refined_solve(A, b)[0])
    return np.array(out)


# ----------------------------------------------------------------------------- error measures
def h_error(H, Href) -> float:
    """max_q |H_q - Href_q| / |Href_q|."""
    H, Href = np.asarray(H, dtype=sy.CLD), np.asarray(Href, dtype=sy.CLD)
    return float(np.max(np.abs(H - Href) / np.abs(Href)))


def errors(cref: ComplexReference, loss_type, sel, H=None, terms=None, w=None, rows=None, scale=1.0):
    """Errors of a candidate over the frequencies ``sel``: ``H`` (h_error), ``terms`` the relative error of the loss
    sum, ``w`` (n_stiff,) max_k |w_k - ref_k| / max_k |ref_k| as synthetic.errors, ``rows`` (len(sel), n_stiff) as
    synthetic_jacobian.row_errors.  ``w`` carries ``scale``."""
    out = {}
    if H is not None:
        out["H"] = h_error(H, cref.H[sel])
    if rows is not None:
        out["jc"] = sj.row_errors(rows, cref.rows[sel])
    if loss_type in ("NONE", None):
        return out
    L = cref.loss(loss_type)
    if terms is not None and loss_type != "CCOTANGENT":
        tot = np.sum(L["terms"][sel].astype(sy.LD))
        out["loss"] = float(abs(np.sum(np.asarray(terms, dtype=sy.LD)) / tot - 1))
    if w is not None:
        wr = scale * L["w"][sel].sum(axis=0)
        out["w"] = float(np.max(np.abs(np.asarray(w, dtype=sy.CLD) - wr)) / np.max(np.abs(wr)))
    return out


# ----------------------------------------------------------------------------- the sweep's sequence in fp64
def _sequence(op, solve_q, freqs, sel, cref, loss_types, correct, scale_corr, refine):
    """The sweep's own sequence in fp64 with ``solve_q(q)(v, transpose)`` over ``sel``: forward solve,
    mu = solve(a_d, True), one refinement step each under ``refine``; with ``correct`` H += mu @ r (r = b - A x in
    extended precision rounded to fp64) and lam = g(H) [H / (mu @ b - mu @ r)] mu (the bracket under ``scale_corr``),
    the rows with g = 1; without, lam = solve(g(H) a_d, True) and the rows from mu.  Returns (H, rows,
    {loss_type: (terms, w)})."""
    refc = cref.refc
    ad = a_d(op, cref.axis, False)
    Hs, rows = [], []
    per = {lt: ([], 0) for lt in loss_types}
    for q in sel:
        solve = solve_q(q)
        A = refc.mats[q]
        b_ld = op.b_ld(freqs[q])
        b = b_ld.astype(np.complex128)
        x = solve(b, False)
        if refine:
            x = sy._refine_step(solve, A, b_ld, x, False)
        H = ad @ x
        mu = solve(ad + 0j, True)
        if refine:
            mu = sy._refine_step(solve, A, ad, mu, True)
        fac = 1.0
        if correct:
            r = (b_ld - A @ x.astype(sy.CLD)).astype(np.complex128)
            d = mu @ r
            H = H + d
            if scale_corr:
                fac = H / (mu @ b - d)
        Hs.append(H)
        rows.append(sy.partials(op, fac * mu, x))
        for lt in loss_types:
            term, g = loss_c(H, cref.sweep_ref(lt)[q], lt)
            if correct:
                lam = (g * fac) * mu
            else:
                lam = solve(g * ad, True)
                if refine:
                    lam = sy._refine_step(solve, A, g * ad.astype(sy.CLD), lam, True)
            terms, w = per[lt]
            per[lt] = (terms + [term], w + sy.partials(op, lam, x))
    return np.array(Hs), np.array(rows), per


def model_errors(op: sy.Operator, sym, freqs, axis, loss_types=LOSSES + ("CCOTANGENT",), symmetric=True,
                 correct=False, scale_corr=True, refine=False):
    """e_model and e_dense over EVERY frequency of ``freqs`` (the caller passes its sample of the sweep): errors
    against ``reference`` of the sequence through the multifrontal model (synthetic._model_solver) and through the
    unrefined dense LU.  Returns {loss_type: (e_model, e_dense)} with the keys "H", "jc", "w" and (but for CCOTANGENT)
    "loss" in each dict."""
    cref = reference(op, freqs, axis)
    refc = cref.refc
    sel = list(range(len(freqs)))
    both = []
    for which in ("model", "dense"):
        if which == "model":
            solve_q = lambda q: sy._model_solver(op, sym, freqs[q], symmetric)                          # noqa: E731
        else:
            solve_q = lambda q: (lambda v, tr: sla.lu_solve(refc.lus[q], v, trans=1 if tr else 0))      # noqa: E731
        both.append(_sequence(op, solve_q, freqs, sel, cref, loss_types, correct, scale_corr, refine))
    out = {}
    for lt in loss_types:
        out[lt] = tuple(errors(cref, lt, sel, H=H, terms=per[lt][0], w=per[lt][1], rows=rows)
                        for H, rows, per in both)
    return out


def bounds(e_model, e_dense):
    """The project's rule: 10 x max(e_model, e_dense, FLOOR) per quantity."""
    return sy.bounds(e_model, e_dense)
