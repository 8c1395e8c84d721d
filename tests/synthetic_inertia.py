"""The inertia rows of pfr_inertia_sweep on the synthetic fronts of ``synthetic.py`` (test infrastructure, not a test;
mirrors ``synthetic_jacobian.py`` / ``synthetic_complex.py``): a case's mass matrix split into components, the
extended-precision reference rows and the errors of the fp64 multifrontal model and of the unrefined dense LU against
them, from which the GPU tests' bounds come.

    A(f) = K - om2 sum_j I_j G_j,   b(f) = rhs (beta - om2 sum_j d_j I_j),   om2 = (2 pi f)^2
    jm[q][j] = om2_q ( m_q mu_q^T G_j x_q - d_j m_q mu_q^T rhs ),   A_q^T mu_q = d fr_q / d x_q  (or a_d: the response H)

The split is exact: G_j and d_j are multiples of 2^-60 of at most 41 significant bits and the I_j have 4, so the fp64
sums sum_j I_j G_j and sum_j d_j I_j, in the engine's order (left to right), carry no rounding -- the operator the
solver factorises IS the one the components describe, and the homogeneity identity

    sum_k c_k jc[q][k] + sum_j I_j jm[q][j] = 0

holds for the reference to the accuracy of its extended-precision solves.
"""
from __future__ import annotations

import dataclasses

import numpy as np
import scipy.linalg as sla

import synthetic as sy
import synthetic_complex as sc
import synthetic_jacobian as sj

I_ALL = np.array([0.75, 1.25, 2.5, 0.375])          # the coefficients I_j (4 significant bits each)
SHARE = np.array([0.4, 0.3, 0.1, 0.2])               # of the load's mass_sum carried by component j
GRID = 60                                            # G_j and d_j are multiples of 2^-GRID


@dataclasses.dataclass(eq=False)
class Inertia:
    """A case with its mass split: ``op`` is the case's operator with M = sum_j I_j G_j and mass_sum = sum_j d_j I_j
    (fp64, the engine's order) and a fresh cache."""
    op: sy.Operator
    G: np.ndarray             # (n_mass, nnz) real
    I: np.ndarray             # (n_mass,)
    d: np.ndarray             # (n_mass,) load weights

    @property
    def n_mass(self):
        return int(self.I.size)

    def G_ld(self):
        if "G" not in self.op._cache:
            self.op._cache["G"] = self.G.astype(sy.LD)
        return self.op._cache["G"]


def recombine(I, G):
    """sum_j I_j G_j in fp64, left to right: Problem._Engine's expression for ``mass``."""
    out = I[0] * G[0]
    for j in range(1, len(I)):
        out = out + I[j] * G[j]
    return out


_SPLITS = {}


def split(op: sy.Operator, n_mass=4, zero=(), entries=None, seed=0) -> Inertia:
    """Split ``op.M`` into ``n_mass`` symmetric components: entry by entry random shares (the same on an entry and its
    mirror), G_j = share_j M / I_j rounded to the grid.  ``zero``: components set to zero everywhere (their share of M
    is dropped: the operator is rebuilt from the components).  ``entries`` = k: every component keeps only the diagonal
    entries of the first k loaded non-Dirichlet nodes -- the contraction's list then has exactly k entries.  Cached per
    operator: the same arguments return the same object."""
    key = (id(op), n_mass, tuple(zero), entries, seed)
    if key in _SPLITS:
        return _SPLITS[key][1]
    pat = op.pat
    rng = np.random.default_rng(8000 + seed)
    rows, cols = pat.rows.astype(np.int64), pat.cols.astype(np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    pair = lo * pat.n + hi                                      # an entry and its mirror share the key
    _, inv = np.unique(pair, return_inverse=True)
    share = 0.2 + rng.random((n_mass, int(inv.max()) + 1))
    share = (share / share.sum(axis=0))[:, inv]
    I = I_ALL[:n_mass].copy()
    G = sy._q(share * op.M[None, :] / I[:, None], GRID)
    for j in zero:
        G[j] = 0.0
    if entries is not None:
        isdir = np.zeros(pat.n, bool)
        isdir[pat.dirichlet] = True
        nodes = [int(i) for i in np.nonzero(op.rhs)[0] if not isdir[i]][:entries]
        assert len(nodes) == entries
        keep = np.zeros(pat.nnz, bool)
        keep[[int(np.nonzero((rows == i) & (cols == i))[0][0]) for i in nodes]] = True
        G[:, ~keep] = 0.0
        assert np.count_nonzero(G.any(axis=0)) == entries
    d = sy._q(op.mass_sum * SHARE[:n_mass] / SHARE[:n_mass].sum() / I, GRID)
    M = recombine(I, G)
    assert np.array_equal(M.astype(sy.LD), (I.astype(sy.LD)[:, None] * G.astype(sy.LD)).sum(axis=0)), "split not exact"
    mass_sum = float(recombine(I, d[:, None])[0])
    assert sy.LD(mass_sum) == (I.astype(sy.LD) * d.astype(sy.LD)).sum()
    new = dataclasses.replace(op, M=M, mass_sum=mass_sum, _cache={})
    out = Inertia(new, G, I, d)
    _SPLITS[key] = (op, out)                                    # op kept alive: its id is the key
    return out


# ----------------------------------------------------------------------------- rows
def mass_rows(ins: Inertia, lam, x, om2):
    """om2 (lam^T G_j x - d_j lam^T rhs) per component, in the precision of lam / x."""
    ext = np.asarray(x).dtype == sy.CLD
    T = sy.LD if ext else np.float64
    p = lam[ins.op.pat.rows] * x[ins.op.pat.cols]
    G = ins.G_ld() if ext else ins.G
    return T(om2) * (G @ p - ins.d.astype(T) * (lam @ ins.op.rhs.astype(T)))


def reference(ins: Inertia, freqs, axis=None):
    """(response, jc rows, jm rows) in extended precision at ``freqs`` from synthetic.reference's refined x and the
    refined adjoint mu (of fr at x; of the complex response along ``axis``).  Cached on the operator."""
    op = ins.op
    refc = sy.reference(op, freqs)
    key = ("inertia", refc.freqs.tobytes(), None if axis is None else tuple(float(v) for v in axis))
    if key not in op._cache:
        if axis is None:
            resp = refc.fr
            mus = [sy.refined_solve(refc.mats[q], sy.adjoint_seed(op, refc.x[q], sy.LD(1)), refc.lus[q], trans=True)[0]
                   for q in range(refc.freqs.size)]
        else:
            cref = sc.reference(op, freqs, axis)
            resp, mus = cref.H, cref.mu
        jc = np.array([sy.partials(op, mu, x) for mu, x in zip(mus, refc.x)])
        jm = np.array([mass_rows(ins, mu, x, op.om2(f)) for mu, x, f in zip(mus, refc.x, refc.freqs)])
        op._cache[key] = (resp, jc, jm)
    return op._cache[key]


def response_at(ins: Inertia, freqs, I_ld, axis=None, coef_ld=None):
    """The response (fr, or H along ``axis``) in extended precision of the operator with the inertia coefficients
    ``I_ld`` (and stiffness coefficients ``coef_ld``, default the case's) at ``freqs``, nothing rounded to fp64 on the
    way: what the rows are the derivative of."""
    op = ins.op
    coef_ld = op.coef.astype(sy.CLD) if coef_ld is None else coef_ld
    I_ld = np.asarray(I_ld, dtype=sy.LD)
    K = op.pat.dense(coef_ld @ op._ld("S"))
    M = op.pat.dense(I_ld @ ins.G_ld())
    beta = coef_ld @ op.e.astype(sy.LD)
    msum = I_ld @ ins.d.astype(sy.LD)
    ad = None if axis is None else sc.a_d(op, axis, True)
    out = []
    for f in freqs:
        f = sy.LD(f)
        om = sy.LD(6.283185307179586) * f
        om2 = om * om
        x = sy.refined_solve(K - om2 * M, op.rhs.astype(sy.LD) * (beta - om2 * msum))[0]
        out.append(sy.fr_of(op, x)[0] if axis is None else ad @ x)
    return np.array(out)


def homogeneity(ins: Inertia, jc, jm):
    """Per frequency |sum_k c_k jc_k + sum_j I_j jm_j| / max(|c_k jc_k|, |I_j jm_j|), in extended precision."""
    a = np.asarray(jc, dtype=sy.CLD) * ins.op.coef.astype(sy.CLD)[None, :]
    b = np.asarray(jm, dtype=sy.CLD) * ins.I.astype(sy.LD)[None, :]
    scale = np.maximum(np.abs(a).max(axis=1), np.abs(b).max(axis=1))
    return (np.abs(a.sum(axis=1) + b.sum(axis=1)) / scale).astype(np.float64)


def slope(ins: Inertia, freqs, jm):
    """d response / d f = (2 / f) sum_j I_j jm_j (real part for fr: the caller's), in the precision of jm."""
    jm = np.asarray(jm)
    T = sy.LD if jm.dtype == sy.CLD else np.float64
    return (T(2) / np.asarray(freqs, dtype=T)) * (jm @ ins.I.astype(T))


# ----------------------------------------------------------------------------- the sweep's sequence in fp64
def _rows_of(ins, solve_q, freqs, sel, refc, correct, scale_corr, refine=False, axis=None):
    """(response, jc rows, jm rows) over ``sel`` of the sweep's sequence in fp64 with ``solve_q(q)(v, transpose)``, as
    synthetic_jacobian._rows_of / synthetic_complex._sequence form it: forward solve, the adjoint mu (of fr at that x,
    or of a_d), one refinement step each under ``refine``; with ``correct`` the response += mu^T r (its real part for
    fr; r = b - A x in extended precision rounded to fp64) and lam = m mu with m = 1 or, with ``scale_corr``,
    response / (mu^T b - mu^T r)."""
    op = ins.op
    ad = None if axis is None else sc.a_d(op, axis, False)
    resp, jcs, jms = [], [], []
    for q in sel:
        solve = solve_q(q)
        b_ld = op.b_ld(freqs[q])
        b = b_ld.astype(np.complex128)
        x = solve(b, False)
        if refine:
            x = sy._refine_step(solve, refc.mats[q], b_ld, x, False)
        if axis is None:
            r0 = sy.fr_of(op, x)[0]
            g = sy.adjoint_seed(op, x, 1.0)
        else:
            r0 = ad @ x
            g = ad + 0j
        mu = solve(g, True)
        if refine:
            mu = sy._refine_step(solve, refc.mats[q], g, mu, True)
        lam = mu
        if correct:
            r = (b_ld - refc.mats[q] @ x.astype(sy.CLD)).astype(np.complex128)
            dd = mu @ r
            r0 = r0 + (dd.real if axis is None else dd)
            if scale_corr:
                lam = (r0 / (mu @ b - dd)) * mu
        resp.append(r0)
        jcs.append(sy.partials(op, lam, x))
        jms.append(mass_rows(ins, lam, x, op.om2(freqs[q])))
    return np.array(resp), np.array(jcs), np.array(jms)


def resp_error(resp, ref) -> float:
    """max_q |resp_q - ref_q| / |ref_q| (fr: the relative error)."""
    resp, ref = np.asarray(resp, dtype=sy.CLD), np.asarray(ref, dtype=sy.CLD)
    return float(np.max(np.abs(resp - ref) / np.abs(ref)))


def model_errors(ins: Inertia, sym, freqs, symmetric=True, correct=False, scale_corr=True, refine=False, axis=None):
    """e_model and e_dense over EVERY frequency of ``freqs`` (the caller passes its sample of the sweep): the errors
    against ``reference`` of the sequence through the multifrontal model (synthetic._model_solver) and through the
    unrefined dense LU.  Returns (e_model, e_dense), dicts with "jm", "jc" (synthetic_jacobian.row_errors), "resp" and
    "hom" (the largest homogeneity residual of the sequence's own rows)."""
    op = ins.op
    refc = sy.reference(op, freqs)
    resp, jc, jm = reference(ins, freqs, axis)
    sel = list(range(len(freqs)))
    out = []
    for which in ("model", "dense"):
        if which == "model":
            solve_q = lambda q: sy._model_solver(op, sym, freqs[q], symmetric)                          # noqa: E731
        else:
            solve_q = lambda q: (lambda v, tr: sla.lu_solve(refc.lus[q], v, trans=1 if tr else 0))      # noqa: E731
        r, c, m = _rows_of(ins, solve_q, freqs, sel, refc, correct, scale_corr, refine, axis)
        out.append({"jm": sj.row_errors(m, jm), "jc": sj.row_errors(c, jc), "resp": resp_error(r, resp),
                    "hom": float(homogeneity(ins, c, m).max())})
    return out[0], out[1]


def bounds(e_model, e_dense):
    """The project's rule: 10 x max(e_model, e_dense, FLOOR) per quantity."""
    return sy.bounds(e_model, e_dense)


# ----------------------------------------------------------------------------- the compacted list
def check_mass_list(lst, ptr, n_list, ent, on, row_on=None, batch=4):
    """The properties of the plan's compacted list ``lst`` with the waves' batch ranges ``ptr`` over the contraction
    entries ``ent`` (n_uent, 4: permuted column, nz (i, j), nz (j, i), permuted row) for the per-entry flags ``on`` (some
    component non-zero) and the visited permuted rows ``row_on`` (None: all).  Raises AssertionError naming the
    property.  Returns the wave of every listed entry."""
    lst, ptr = np.asarray(lst), np.asarray(ptr)
    assert lst.size % batch == 0 and ptr[0] == 0 and np.all(np.diff(ptr) >= 0), "whole batches, wave by wave"
    assert ptr[-1] * batch == lst.size or (n_list == 0 and ptr[-1] == 0), "the waves' runs cover the list"
    wave_of = {}
    for w in range(ptr.size - 1):
        run = lst[batch * ptr[w]:batch * ptr[w + 1]]
        k = int(np.count_nonzero(run >= 0))
        assert np.all(run[:k] >= 0) and np.all(run[k:] == -1) and run.size - k < batch, "a run: entries, then < 4 of -1"
        wave_of.update({int(e): w for e in run[:k]})
    body = lst[lst >= 0]
    assert body.size == n_list and np.all(body < ent.shape[0]), "entries in range"
    assert np.all(np.diff(body) > 0), "a subsequence of the entries' order, each once"
    assert np.all(np.diff([wave_of[int(e)] for e in body]) >= 0), "the waves own ascending ranges of the entries"
    real = (ent[:, 0] >= 0) & (ent[:, 1] >= 0)
    want = real & on[np.maximum(ent[:, 1], 0)]
    if row_on is not None:
        want &= row_on[ent[:, 3]]
    assert np.all(want[body]), "every listed entry has a non-zero component on a visited row"
    assert np.array_equal(np.nonzero(want)[0], body), "every non-zero entry on a visited row is listed"
    return wave_of
