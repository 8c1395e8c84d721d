"""Host side of the live-matrix contraction (include/pfr.h, pfr_symbolic_live; csrc/plan.cpp live_stiffness): which
stiffness matrices hold a non-zero value on an entry of the rows a sweep's forward walk visits -- decided by value from
the stiffness table, without a device, as tests/test_prune_cpu.py checks the views."""
import numpy as np
import pytest

import synthetic as sy
import synthetic_live as sl
from helpers import make_problem
from plate_inverse_problem_amd import _native
from test_prune_cpu import _engine_pattern

MPS = np.r_[0:6, 12:18]          # the engine's stiffness matrices of a mid-plane-symmetric material: A and D


def _brute(pat_rows, stiff, visited_nodes):
    """The same set straight from the definition: k with a non-zero value on an entry whose row is visited."""
    on = np.isin(pat_rows, visited_nodes)
    return sorted(np.nonzero((stiff[on] != 0).any(0))[0].tolist())


def test_plate_ny6_pruned_six_of_twelve_full_twelve():
    p = make_problem("orthotropic", ny=6)
    rows, cols, colptr, vals = _engine_pattern(p)
    sym = _native.Symbolic(p.mat_size, colptr, rows, leaf_size=200, symmetric=True)
    stiff = np.ascontiguousarray(vals[MPS].T)                      # (nnz, 12), as Problem._Engine registers it
    assert sym.live(p.vec, stiff, prune=True) == list(range(6, 12))   # the bending rows: the six D matrices
    assert sym.live(p.vec, stiff, prune=False) == list(range(12))
    mask = sym.prune(128, p.vec)[0].astype(bool)
    perm, fr = sym.export("PERM"), sym.export("FRONTS")
    visited = np.concatenate([perm[c0:c0 + ns] for (ns, f, r0, c0, *_r), m in zip(fr, mask) if m])
    assert _brute(rows, stiff, visited) == list(range(6, 12))


def test_general_laminate_eighteen_of_eighteen():
    p = make_problem("sol", ny=6)                                  # B != 0: one tree, every row loaded
    rows, cols, colptr, vals = _engine_pattern(p)
    sym = _native.Symbolic(p.mat_size, colptr, rows, leaf_size=200, symmetric=True)
    stiff = np.ascontiguousarray(vals[:18].T)
    for prune in (True, False):
        assert sym.live(p.vec, stiff, prune=prune) == list(range(18))
    assert _brute(rows, stiff, np.arange(p.mat_size)) == list(range(18))


@pytest.mark.parametrize("extra,want", [(0.0, sorted(sl.LIVE)), (0.25, sorted(sl.LIVE + (sl.DEAD[2],)))])
def test_forest(extra, want):
    pat, op = sl.case(extra)
    sym = sl.symbolic()
    stiff = np.ascontiguousarray(op.S.T)
    rows0 = pat.components()[0][3]
    assert sym.live(op.rhs, stiff, prune=True) == want == _brute(pat.rows, stiff, rows0)
    assert sym.live(op.rhs, stiff, prune=False) == list(range(12))
    # the load on both trees: nothing is pruned, every row is visited
    rhs = op.rhs.copy()
    rhs[pat.components()[1][3][0]] = 1.0
    assert sym.live(rhs, stiff, prune=True) == list(range(12))


def test_value_decides_not_the_slot():
    """A negative zero is a zero; one non-zero value anywhere on a visited row makes its matrix live."""
    pat, op = sl.case()
    sym = sl.symbolic()
    stiff = np.ascontiguousarray(op.S.T).copy()
    rows0 = pat.components()[0][3]
    e = np.nonzero(np.isin(pat.rows, rows0))[0]
    stiff[e[0], sl.DEAD[0]] = -0.0
    assert sym.live(op.rhs, stiff, prune=True) == sorted(sl.LIVE)
    stiff[e[-1], sl.DEAD[0]] = 2.0 ** -40
    assert sym.live(op.rhs, stiff, prune=True) == sorted(sl.LIVE + (sl.DEAD[0],))


def test_single_tree_all_live():
    _, op = sy.case("F0")
    assert sy.symbolic("F0").live(op.rhs, np.ascontiguousarray(op.S.T), prune=True) == list(range(12))


def test_needs_a_symmetric_analysis():
    pat, op = sl.case()
    gen = _native.Symbolic(pat.n, pat.colptr, pat.rows, symmetric=False)
    with pytest.raises(_native.NativeError):
        gen.live(op.rhs, np.ascontiguousarray(op.S.T))
