"""GPU: the forward walk's gradient contraction over the live stiffness matrices only (include/pfr.h, pfr_solver_live;
csrc/kernels.hip k_residual with NSK < n_stiff) against the full n_stiff form (PFR_CONTRACT_LIVE=0) and against
pruning off, bit for bit, on the forests of tests/synthetic_live.py: a loaded tree whose rows hold 1 .. 9 entries (a
row shorter than a gather batch of 4 or 8, exactly one batch, a batch and a tail, two batches and a tail) with values
in six of twelve matrices, and an unloaded tree with values in all twelve.  70 frequencies at max_batch 64: one full
64-frequency group and one clamped.  No tolerance anywhere: a dropped accumulator only ever held fma(0.0, finite, +0.0).
Against pruning off the adjoint's backward error alone may differ: pruning takes it over the loaded rows (include/pfr.h).
"""
import numpy as np
import pytest

import synthetic as sy
import synthetic_live as sl
import synthetic_population as sp
from test_gpu_synthetic import DEFAULT, _t, make_solver, run_sweep
from test_gpu_synthetic_jacobian import run_jacobian

pytestmark = pytest.mark.gpu
SWEEP_KEYS = ("fr", "loss", "w", "flags", "berr")
UNROLLS = ("4", "8")


def _eq(name, a, b, keys):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (name, k)


def _run(monkeypatch, op, sym, *, live, prune, unroll="4", population=True):
    """pfr_sweep, pfr_jacobian_sweep and one population sweep of two members on ONE solver created under the knobs."""
    monkeypatch.setenv("PFR_CONTRACT_LIVE", "1" if live else "0")
    monkeypatch.setenv("PFR_LIVE_UNROLL", unroll)          # read in pfr_solver_create, as every launch knob
    solver = make_solver(op, sym, prune=prune)
    out = {"live": solver[0].live(), "mask": solver[0].active_fronts()}
    out["sweep"] = run_sweep(op, sym, sl.FREQS, mode=DEFAULT, solver=solver, vectors=False)
    out["jac"] = run_jacobian(op, sym, sl.FREQS, mode=DEFAULT, solver=solver)
    if population:
        f, member, valid = sp.lanes(2, sl.FREQS[:64])
        out["pop"] = sp.run_population(op, sl.members(op), sym, f, member, max_batch=64, mode=DEFAULT,
                                       make_solver=make_solver, t=_t, jac=True, solver=solver)
    return out


def _same_outputs(name, a, b, pruning_differs=False):
    """``pruning_differs``: ``b`` ran with pruning off -- its adjoint backward error is taken over every row, the
    pruned one over the loaded rows (tests/test_gpu_synthetic_prune.py::_compare_on_off): forward column equal, adjoint
    column not above; everything else equal as between two pruned runs."""
    for what, keys in (("sweep", SWEEP_KEYS), ("jac", ("fr", "jc", "flags", "berr")), ("pop", ("fr", "jc", "flags", "berr"))):
        if what not in a or what not in b:
            continue
        _eq(name, a[what], b[what], [k for k in keys if k != "berr" or not pruning_differs])
        if pruning_differs:
            assert np.array_equal(a[what]["berr"][:, 0], b[what]["berr"][:, 0], equal_nan=True), (name, what)
            assert np.all(a[what]["berr"][:, 1] <= b[what]["berr"][:, 1]), (name, what)


def _clean(out):
    assert np.all(out["sweep"]["flags"] == 0) and np.all(out["jac"]["flags"] == 0)
    be = out["sweep"]["berr"]
    assert np.all(np.isfinite(be)) and be.max() <= sy.BERR_MAX


def test_rows_cover_every_batch_case():
    pat, _ = sl.case()
    rows0 = pat.components()[0][3]
    assert sorted(set(sl.row_lengths(pat, rows0).tolist())) == list(range(1, 10))


@pytest.mark.parametrize("unroll", UNROLLS)
def test_six_live_of_twelve(unroll, monkeypatch):
    """The loaded tree's walk finds six live matrices and takes the compact form; the full form and pruning off give the
    same loss, w (all twelve), fr, Jacobian rows, population rows, backward errors and flags; the dropped slots are 0."""
    pat, op = sl.case()
    sym = sl.symbolic()
    on = _run(monkeypatch, op, sym, live=True, prune=True, unroll=unroll)
    full = _run(monkeypatch, op, sym, live=False, prune=True, unroll=unroll)
    unpruned = _run(monkeypatch, op, sym, live=True, prune=False, unroll=unroll)
    assert 0 < on["mask"].sum() < on["mask"].size and unpruned["mask"].all()
    assert on["live"] == (list(sl.LIVE), True)
    assert full["live"] == (list(sl.LIVE), False)                    # the same list, no compact table
    assert unpruned["live"] == (list(range(12)), False)              # every row: tree 1's diagonal holds all twelve
    _same_outputs("live-vs-full", on, full)
    _same_outputs("live-vs-unpruned", on, unpruned, pruning_differs=True)
    _clean(on)
    dead = list(sl.DEAD)
    nf = sl.FREQS.size
    for out in (on, full, unpruned):
        assert np.all(out["sweep"]["w"][dead] == 0) and np.all(out["sweep"]["w"][list(sl.LIVE)] != 0)
        assert np.all(out["jac"]["jc"][:nf, dead] == 0) and np.all(out["jac"]["jc"][:nf][:, list(sl.LIVE)] != 0)
        sel = np.isfinite(out["pop"]["jc"][:-1, 0].real)
        assert sel.sum() == 2 * 64 and np.all(out["pop"]["jc"][:-1][sel][:, dead] == 0)


@pytest.mark.parametrize("unroll", UNROLLS)
def test_a_seventh_live_matrix_falls_back(unroll, monkeypatch):
    """One visited entry with a non-zero value in a seventh matrix: the list grows, no compact form is taken (only 6
    and 12 exist), and the outputs are the full form's and the unpruned sweep's."""
    pat, op = sl.case(extra=0.25)
    sym = sl.symbolic()
    seven = sorted(sl.LIVE + (sl.DEAD[2],))
    on = _run(monkeypatch, op, sym, live=True, prune=True, unroll=unroll)
    full = _run(monkeypatch, op, sym, live=False, prune=True, unroll=unroll)
    unpruned = _run(monkeypatch, op, sym, live=True, prune=False, unroll=unroll)
    assert on["live"] == (seven, False) and full["live"] == (seven, False)
    _same_outputs("seven-vs-full", on, full)
    _same_outputs("seven-vs-unpruned", on, unpruned, pruning_differs=True)
    _clean(on)
    nf = sl.FREQS.size
    assert np.all(on["jac"]["jc"][:nf, sl.DEAD[2]] != 0)                       # the seventh is contracted
    still_dead = [k for k in sl.DEAD if k != sl.DEAD[2]]
    assert np.all(on["jac"]["jc"][:nf, still_dead] == 0) and np.all(on["sweep"]["w"][still_dead] == 0)
    base = _run(monkeypatch, sl.case()[1], sym, live=True, prune=True, unroll=unroll, population=False)
    assert not np.array_equal(base["sweep"]["fr"], on["sweep"]["fr"])          # the value is in K


def test_all_live_builds_nothing(monkeypatch):
    """A single tree with values in every matrix: twelve live, no compact table, the outputs those of
    PFR_CONTRACT_LIVE=0."""
    _, op = sy.case("F0")
    sym = sy.symbolic("F0")
    on = _run(monkeypatch, op, sym, live=True, prune=True, population=False)
    full = _run(monkeypatch, op, sym, live=False, prune=True, population=False)
    assert on["live"] == (list(range(12)), False) and full["live"] == on["live"]
    assert on["mask"].all()
    _same_outputs("all-live", on, full)
    _clean(on)
