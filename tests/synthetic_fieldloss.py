"""The field-loss sweep (pfr_field_loss_sweep) on the synthetic fronts of ``synthetic.py`` (test infrastructure, not a
test; mirrors ``synthetic_complex.py``): the extended-precision reference and the errors of the fp64 multifrontal model
and of the unrefined dense LU against it, from which the GPU tests' bounds come.

    x_j = x_q[rows[j]], r_j = data[q][j], weights v_j; per frequency q (include/pfr.h):
        FIELD_MSE    sum v |x - r|^2                                  g_j = 2 v conj(x_j - r_j)
        FIELD_RMSE   sum v |x - r|^2 / R2,  R2 = sum v |r|^2          g_j = 2 v conj(x_j - r_j) / R2
        FIELD_MAC    1 - |s|^2 / (X2 R2), s = sum v conj(r) x,        g_j = v (2 |s|^2 / (X2^2 R2) conj(x_j)
                     X2 = sum v |x|^2                                          - 2 conj(s) / (X2 R2) conj(r_j))
        FCOTANGENT   none                                             g_j = the caller's dL/dx_j
    d term = Re(sum_j g_j dx_j);  A^T lam_q = g_q scattered to the rows;  w_k = sum_q (-lam_q^T S_k x_q + e_k lam_q^T rhs)

The data: the true field per row times (1 + 0.3 xi_j) e^{i phi_j}, xi_j and phi_j uniform in [-1, 1] with a fixed seed
-- an amplitude and phase error per measurement point, which keeps 1 - MAC well away from zero (the FIELD_MAC term is
then no cancellation; ``min_one_minus_mac`` measures it, the CPU test asserts >= 1e-2).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import scipy.linalg as sla

import synthetic as sy

LOSSES = ("FIELD_MSE", "FIELD_RMSE", "FIELD_MAC")
ALL = LOSSES + ("FCOTANGENT",)
LOSS_ID = {"FIELD_MSE": 32, "FIELD_RMSE": 33, "FIELD_MAC": 34, "FCOTANGENT": 35}      # include/pfr.h
MODEL_EVERY = 6                                   # the model's sample of a sweep, as the complex tests'
N_SOME = 33                                       # the partial selection: one tile and one row


def model_sample(nfreq):
    """Every MODEL_EVERY-th frequency and synthetic.three's (where the GPU tests read the adjoint back)."""
    return sorted(set(range(0, nfreq, MODEL_EVERY)) | set(sy.three(range(nfreq))))


def selection(n, some: bool, seed=0):
    """None (every row) or N_SOME distinct rows in a fixed random order (half the rows of a pattern with no more than
    N_SOME: shape F0 has 26)."""
    k = N_SOME if n > N_SOME else n // 2
    return np.random.default_rng(8100 + seed).permutation(n)[:k].astype(np.int32) if some else None


EDGE_SIZES = (1, 31, 32, 33, 65)                  # and n: around one and two tiles of 32 selected rows


def edge_selection(pat: sy.Pattern, k, seed=0):
    """``k`` distinct rows in descending order that hold the Dirichlet rows (k = 1: the loaded Dirichlet row alone;
    k >= n: every row, descending)."""
    n, d = pat.n, np.asarray(pat.dirichlet, dtype=np.int64)
    if k == 1:
        return d[:1].astype(np.int32)
    if k >= n:
        return np.arange(n, dtype=np.int32)[::-1].copy()
    rest = np.setdiff1d(np.arange(n), d)
    # 8601: with 8600 the 31-row pick of shape A has 1 - MAC = 4e-3 at one frequency (test_field_loss_cpu asserts 1e-2)
    pick = np.random.default_rng(8601 + seed + k).permutation(rest)[:k - d.size]
    return np.sort(np.concatenate([d, pick]))[::-1].astype(np.int32)


def weights(n_sel, seed=0):
    """Non-uniform weights in [0.25, 1.25), one exact zero among them (a masked point)."""
    v = 0.25 + np.random.default_rng(8200 + seed).random(n_sel)
    v[n_sel // 3] = 0.0
    return v


def terms_g(x, r, v, loss_type):
    """(term, g (n_sel,)) of one frequency in the precision of ``x`` (extended, or fp64 as fp64 code forms them);
    ``v`` None: all 1."""
    ext = np.asarray(x).dtype == sy.CLD
    C, T = (sy.CLD, sy.LD) if ext else (np.complex128, np.float64)
    x, r = np.asarray(x, dtype=C), np.asarray(r, dtype=C)
    v = np.ones(x.size, dtype=T) if v is None else np.asarray(v, dtype=T)
    if loss_type == "FCOTANGENT":
        return T(0), r
    if loss_type in ("FIELD_MSE", "FIELD_RMSE"):
        z = x - r
        den = T(1) if loss_type == "FIELD_MSE" else np.sum(v * np.abs(r) ** 2)
        return np.sum(v * np.abs(z) ** 2) / den, 2 * v * np.conj(z) / den
    if loss_type == "FIELD_MAC":
        s = np.sum(v * np.conj(r) * x)
        X2, R2 = np.sum(v * np.abs(x) ** 2), np.sum(v * np.abs(r) ** 2)
        s2 = np.abs(s) ** 2
        return 1 - s2 / (X2 * R2), v * (2 * s2 / (X2 * X2 * R2) * np.conj(x) - 2 * np.conj(s) / (X2 * R2) * np.conj(r))
    raise ValueError(loss_type)


def scatter(g, rows, n):
    """The seed as an (n,) vector: g at the selected rows, zero elsewhere."""
    if rows is None:
        return g
    out = np.zeros(n, dtype=g.dtype)
    out[rows] = g
    return out


def make_data(x_sel, seed=0):
    """The measurement of a true field ``x_sel`` (nfreq, n_sel): per row times (1 + 0.3 xi_j) e^{i phi_j}, complex128."""
    rng = np.random.default_rng(8300 + seed)
    n_sel = x_sel.shape[1]
    xi, phi = rng.uniform(-1, 1, n_sel), rng.uniform(-1, 1, n_sel)
    return (np.asarray(x_sel, dtype=sy.CLD) * ((1 + 0.3 * xi) * np.exp(1j * phi))).astype(np.complex128)


@dataclass(eq=False)
class FieldReference:
    refc: sy.Reference
    rows: np.ndarray | None   # the selection (caller numbering), None: every row
    v: np.ndarray | None      # the weights, None: all 1
    data: np.ndarray          # (nfreq, n_sel) complex128: the sweep's reference field
    cot: np.ndarray           # (nfreq, n_sel) complex128: a fixed-seed dL/dx (PFR_LOSS_FCOTANGENT)
    _loss: dict = field(default_factory=dict)

    @property
    def n_sel(self):
        return self.data.shape[1]

    def x_sel(self, q):
        x = self.refc.x[q]
        return x if self.rows is None else x[self.rows]

    def sweep_ref(self, loss_type):
        return self.cot if loss_type == "FCOTANGENT" else self.data

    def weights_for(self, loss_type):
        return None if loss_type == "FCOTANGENT" else self.v

    def loss(self, loss_type):
        """Per-frequency terms, g, lam = refined_solve(A^T, g) and partials w, in extended precision."""
        if loss_type not in self._loss:
            op, refc = self.refc.op, self.refc
            terms, gs, lams, ws = [], [], [], []
            for q in range(refc.freqs.size):
                term, g = terms_g(self.x_sel(q), self.sweep_ref(loss_type)[q], self.weights_for(loss_type), loss_type)
                lam = sy.refined_solve(refc.mats[q], scatter(g, self.rows, op.pat.n), refc.lus[q], trans=True)[0]
                terms.append(term)
                gs.append(g)
                lams.append(lam)
                ws.append(sy.partials(op, lam, refc.x[q]))
            self._loss[loss_type] = {"terms": np.array(terms), "g": np.array(gs), "lam": np.array(lams),
                                     "w": np.array(ws)}
        return self._loss[loss_type]

    def min_one_minus_mac(self):
        """The smallest FIELD_MAC term over the frequencies (extended precision; no adjoint solved)."""
        return float(min(terms_g(self.x_sel(q), self.data[q], self.v, "FIELD_MAC")[0]
                         for q in range(self.refc.freqs.size)))


def reference(op: sy.Operator, freqs, rows=None, v=None, seed=0) -> FieldReference:
    """The field-loss reference of the operator-form case at ``freqs`` (cached on the operator)."""
    refc = sy.reference(op, freqs)
    key = ("floss", refc.freqs.tobytes(), None if rows is None else np.asarray(rows).tobytes(),
           None if v is None else np.asarray(v).tobytes(), seed)
    if key not in op._cache:
        x_sel = refc.x if rows is None else refc.x[:, rows]
        rng = np.random.default_rng(8400 + seed)
        shape = x_sel.shape
        cot = (0.5 + rng.random(shape)) * np.exp(2j * np.pi * rng.random(shape))
        op._cache[key] = FieldReference(refc, None if rows is None else np.asarray(rows), v, make_data(x_sel, seed), cot)
    return op._cache[key]


def loss_at(op: sy.Operator, freqs, coef_ld, fref: FieldReference, loss_type):
    """term_q (nfreq, extended precision) of the operator with the coefficients ``coef_ld`` against ``fref``'s data,
    formed as ``synthetic_jacobian.fr_at`` forms fr (K = coef S and beta = coef e in extended precision)."""
    K = op.pat.dense(coef_ld @ op._ld("S"))
    beta = coef_ld @ op.e.astype(sy.LD)
    out = []
    for q, f in enumerate(freqs):
        om2 = sy.LD(op.om2(f))
        A = K - om2 * op._ld("M")
        b = op.rhs.astype(sy.LD) * (beta - om2 * sy.LD(op.mass_sum))
        x = sy.refined_solve(A, b)[0]
        out.append(terms_g(x if fref.rows is None else x[fref.rows], fref.data[q], fref.v, loss_type)[0])
    return np.array(out)


# ----------------------------------------------------------------------------- error measures
def errors(fref: FieldReference, loss_type, sel, terms=None, w=None, lam=None, scale=1.0):
    """Errors of a candidate over the frequencies ``sel``: ``terms`` the relative error of the loss sum, ``w``
    (n_stiff,) max_k |w_k - ref_k| / max_k |ref_k|, ``lam`` ({q: (n,)}) the largest norm-wise relative error.  ``w``
    and ``lam`` carry ``scale``, ``terms`` do not."""
    L = fref.loss(loss_type)
    out = {}
    if terms is not None and loss_type != "FCOTANGENT":
        tot = np.sum(L["terms"][sel].astype(sy.LD))
        out["loss"] = float(abs(np.sum(np.asarray(terms, dtype=sy.LD)) / tot - 1))
    if w is not None:
        wr = scale * L["w"][sel].sum(axis=0)
        out["w"] = float(np.max(np.abs(np.asarray(w, dtype=sy.CLD) - wr)) / np.max(np.abs(wr)))
    if lam is not None:
        out["lam"] = max(sy.rel(l, scale * L["lam"][q]) for q, l in lam.items())
    return out


# ----------------------------------------------------------------------------- the sweep's sequence in fp64
def _sequence(op, solve_q, fref, sel, loss_types, refine):
    """The sweep's own sequence in fp64 with ``solve_q(q)(v, transpose)`` over ``sel``: the forward solve, the term
    and seed from its rows, lam = solve(seed, True); one refinement step each under ``refine``.  Returns
    {loss_type: (terms, w, {q: lam})}."""
    refc = fref.refc
    n = op.pat.n
    per = {lt: ([], 0, {}) for lt in loss_types}
    for q in sel:
        solve = solve_q(q)
        A = refc.mats[q]
        b_ld = op.b_ld(refc.freqs[q])
        x = solve(b_ld.astype(np.complex128), False)
        if refine:
            x = sy._refine_step(solve, A, b_ld, x, False)
        xs = x if fref.rows is None else x[fref.rows]
        for lt in loss_types:
            term, g = terms_g(xs, fref.sweep_ref(lt)[q], fref.weights_for(lt), lt)
            gf = scatter(g, fref.rows, n)
            lam = solve(gf, True)
            if refine:
                lam = sy._refine_step(solve, A, gf, lam, True)
            terms, w, lams = per[lt]
            lams[q] = lam
            per[lt] = (terms + [term], w + sy.partials(op, lam, x), lams)
    return per


def model_errors(op: sy.Operator, sym, freqs, rows=None, v=None, loss_types=ALL, symmetric=True, refine=False, seed=0):
    """e_model and e_dense over EVERY frequency of ``freqs`` (the caller passes its sample of the sweep): errors
    against ``reference`` of the sequence through the multifrontal model (synthetic._model_solver) and through the
    unrefined dense LU.  Returns {loss_type: (e_model, e_dense)}, dicts with the keys "w", "lam" and (but for
    FCOTANGENT) "loss"."""
    fref = reference(op, freqs, rows, v, seed)
    refc = fref.refc
    sel = list(range(len(freqs)))
    both = []
    for which in ("model", "dense"):
        if which == "model":
            solve_q = lambda q: sy._model_solver(op, sym, freqs[q], symmetric)                          # noqa: E731
        else:
            solve_q = lambda q: (lambda v_, tr: sla.lu_solve(refc.lus[q], v_, trans=1 if tr else 0))    # noqa: E731
        both.append(_sequence(op, solve_q, fref, sel, loss_types, refine))
    return {lt: tuple(errors(fref, lt, sel, terms=per[lt][0], w=per[lt][1], lam=per[lt][2]) for per in both)
            for lt in loss_types}


def bounds(e_model, e_dense):
    """The project's rule: 10 x max(e_model, e_dense, FLOOR) per quantity."""
    return sy.bounds(e_model, e_dense)
