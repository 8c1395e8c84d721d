"""Synthetic forests for the live-matrix contraction (include/pfr.h, pfr_solver_live) -- test
infrastructure, not a test.

``case(extra)``: a forest of two trees with twelve stiffness matrices.

  tree 0 (loaded)   ten nodes: the threshold graph on 0..8 (i ~ j iff i + j >= 8) and one Dirichlet node coupled into
                    node 3.  Its rows hold 1, 2, ... 9 entries (the Dirichlet row 1; nodes 0..8: 2, 3, 4, 6, 5, 6, 7, 8,
                    9), which against gather batches of 4 and 8 entries is a row shorter than a batch, exactly one batch,
                    a batch and a tail, and two batches and a tail.  Its entries carry values in the matrices LIVE only.
  tree 1 (unloaded) shape F0 of tests/synthetic.py, with values in LIVE and, on its diagonal, in the other six
                    matrices too: a walk over every row (pruning off) finds all twelve live.

The values are synthetic.make_operator's for six matrices, spread to the twelve slots: K = coef @ S and beta = e @ coef
stay exact (the other slots add exact zeros on tree 0 and multiples of 2^-8 times multiples of 2^-10 on tree 1's
diagonal; e is zero on them, so their w_k and Jacobian columns are exactly the contraction's partials).

``extra`` > 0: one visited diagonal entry of tree 0 (node 5) also gets the value ``extra`` in matrix DEAD[2] -- a
seventh live matrix, which no compact form exists for.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import synthetic as sy

LIVE = (1, 3, 4, 6, 9, 10)           # not a half in slot order: the slot map is exercised
DEAD = tuple(k for k in range(12) if k not in LIVE)
FREQS = np.linspace(40.0, 600.0, 70)   # max_batch 64: one full 64-frequency group and one clamped (6 lanes)


def loaded_tree() -> sy.Pattern:
    nodes = np.arange(9)
    pairs = [(int(i), int(j)) for i in nodes for j in nodes if i < j and i + j >= 8]
    rng = np.random.default_rng(0)
    # one leaf clique and the border both {3}: the Dirichlet node's column couples into node 3 only
    return sy._finish("threshold9+1d", 9, pairs, [np.array([3]), nodes], np.array([3]), [0], 1, rng)


@functools.lru_cache(maxsize=None)
def pattern() -> sy.Pattern:
    return sy.forest([loaded_tree(), sy.SHAPES["F0"]()], pin=0, name="live-forest")


def row_lengths(pat: sy.Pattern, nodes) -> np.ndarray:
    return np.bincount(pat.rows, minlength=pat.n)[np.asarray(nodes)]


@functools.lru_cache(maxsize=None)
def case(extra: float = 0.0):
    """(pattern, operator) -- the load and three sensor rows on tree 0, three sensor rows on tree 1."""
    pat = pattern()
    (_, _, _, rows0), (_, _, border1, rows1) = pat.components()
    support = np.sort(np.concatenate([rows0[[0, 5, 8]], border1[[0, 2, 5]]]))
    op6 = sy.make_operator(pat, n_stiff=6, support=support, load=(0,))
    S = np.zeros((12, pat.nnz))
    S[list(LIVE)] = op6.S
    diag1 = np.nonzero((pat.rows == pat.cols) & np.isin(pat.rows, rows1))[0]
    for t, k in enumerate(DEAD):
        S[k, diag1] = (t + 1) / 16.0
    if extra:
        d5 = np.nonzero((pat.rows == rows0[5]) & (pat.cols == rows0[5]))[0]
        S[DEAD[2], d5] = extra
    coef = np.zeros(12, dtype=np.complex128)
    coef[list(LIVE)] = op6.coef
    coef[list(DEAD)] = (np.arange(6) + 3) / 8.0 + 1j * (np.arange(6) + 1) / 64.0
    e = np.zeros(12)
    e[list(LIVE)] = op6.e
    K = coef @ S
    assert np.array_equal(K.astype(sy.CLD), coef.astype(sy.CLD) @ S.astype(sy.LD)), "coef @ S is not exact in fp64"
    beta = complex(e @ coef)
    assert beta == op6.beta
    op = dataclasses.replace(op6, n_stiff=12, S=S, coef=coef, e=e, K=K, beta=beta, _cache={})
    sy.check_cond([op.matrix_ld(f) for f in FREQS[::10]], "live-forest")
    return pat, op


@functools.lru_cache(maxsize=None)
def symbolic():
    from plate_inverse_problem_amd import _native
    pat = pattern()
    return _native.Symbolic(pat.n, pat.colptr, pat.rows, symmetric=True, last=pat.border)


def members(op, n_members=2, seed=0):
    """Member operators as tests/synthetic_population.py builds them: the coefficients scaled by 1 + multiples of
    2^-6 (K and beta stay exact)."""
    rng = np.random.default_rng(7000 + seed)
    out = []
    for p in range(n_members):
        d = rng.integers(-4, 5, size=(2, op.n_stiff)) / 64.0
        d[0, LIVE[0]] = (p % 4 + 1) / 64.0
        coef = op.coef.real * (1 + d[0]) + 1j * op.coef.imag * (1 + d[1])
        K = coef @ op.S
        assert np.array_equal(K.astype(sy.CLD), coef.astype(sy.CLD) @ op.S.astype(sy.LD))
        m = dataclasses.replace(op, coef=coef, K=K, beta=complex(op.e @ coef), _cache={})
        sy.check_cond([m.matrix_ld(f) for f in FREQS[::10]], f"live-forest member {p}")
        out.append(m)
    return tuple(out)
