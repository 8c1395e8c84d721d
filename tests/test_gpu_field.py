"""GPU: the field sweep on the plate -- ``Problem.solveForwardField`` / ``solveForwardShapes`` / ``getModePicture``
(pfr_field_sweep under the engine's lanes) against the oracle's system, as tests/test_gpu_debug_solution.py checks the
accessor's vectors: the componentwise backward error of A x = b below 1e-12 and fr recomputed on the host from the
returned field within 5e-9 of the oracle's (the project's small-mesh tolerances from that test).  The engine is
forced to two lanes (PFR_LANE_FREQS = 64 at 70 frequencies: blocks of 64 and 6), so `out` is cut into lane blocks."""
import numpy as np
import pytest
import torch

from helpers import make_problem, oracle_for
from plate_inverse_problem_amd import _native

pytestmark = pytest.mark.gpu
FREQS = np.linspace(40.0, 600.0, 70)
PICKS = (0, 37, 63, 64, 69)                      # both lanes' blocks, and both sides of the cut


def _problem(material, monkeypatch, prune="1"):
    monkeypatch.setenv("PFR_LANE_FREQS", "64")   # read when the engine is built
    monkeypatch.setenv("PFR_LANES", "2")
    monkeypatch.setenv("PFR_PRUNE", prune)
    p = make_problem(material, ny=4, device="cuda:0")
    eng = p.engine(FREQS.size)
    assert eng.n_lanes == 2 and [hi - lo for lo, hi in eng._split(FREQS.size)] == [64, 6]
    return p


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _dirichlet_rows(A):
    """Rows of the oracle's matrix that hold only their diagonal entry."""
    R = A.tocsr()
    R.eliminate_zeros()
    return np.nonzero(np.diff(R.indptr) == 1)[0]


@pytest.mark.parametrize("material", ["orthotropic", "sol"])
def test_field_solves_the_oracle_system(material, monkeypatch):
    p = _problem(material, monkeypatch)
    orc = oracle_for(p)
    theta = p.parameters * 1.03
    x, fr = p.solveForwardField(FREQS, theta, return_fr=True)
    n = p.mat_size
    assert x.shape == (FREQS.size, n) and x.dtype == np.complex128 and fr.shape == (FREQS.size,)
    eng = p.engine()
    assert np.all(eng.last_flags == 0)
    berr = eng.last_berr.cpu().numpy()
    assert berr[:, 0].max() < 1e-12 and np.all(np.isnan(berr[:, 1]))
    c = orc.coefficients(theta)
    aU, aV, aW = orc.averaging_vectors()
    ts2 = orc.acc_ts ** 2
    fr_o = orc.fr(FREQS, theta)
    for q in PICKS:
        A = orc.matrix(FREQS[q], c).tocsc()
        b = orc.rhs_vec * orc.rhs_scale(FREQS[q], c)
        r = b - A @ x[q]
        den = abs(A) @ np.abs(x[q]) + np.abs(b)
        assert np.max(np.abs(r)[den > 0] / den[den > 0]) < 1e-12, q
        U, V, W = aU @ x[q], aV @ x[q], aW @ x[q]
        fr_h = np.sqrt(ts2 * abs(U) ** 2 + ts2 * abs(V) ** 2 + abs(W) ** 2)
        assert abs(fr_h / fr_o[q] - 1) < 5e-9, (q, fr_h, fr_o[q])
        assert abs(fr[q] / fr_o[q] - 1) < 5e-9, (q, fr[q], fr_o[q])
    # return_fr: solveForward's fr in the check mode the field sweep runs in (forward check, no correction)
    mode = eng.check_mode
    eng.set_check(mode & (_native.PFR_CHECK_FORWARD | _native.PFR_CHECK_REFINE))
    try:
        assert np.array_equal(_bits(p.solveForward(FREQS, theta)), _bits(fr))
    finally:
        eng.set_check(mode)
    # a selection equals those columns of the full result; so does the same call again (nothing accumulates)
    vr = p.vertex_rows()
    assert np.array_equal(_bits(p.solveForwardField(FREQS, theta, dofs=vr[2])), _bits(x[:, vr[2]]))
    pick = np.r_[vr[1][::-1], vr[0][:3], vr[0][:3], n - 1]
    assert np.array_equal(_bits(p.solveForwardField(FREQS, theta, dofs=pick)), _bits(x[:, pick]))
    # a loss step after the field sweeps is unharmed: the response again, bit for bit
    eng.set_check(mode & (_native.PFR_CHECK_FORWARD | _native.PFR_CHECK_REFINE))
    try:
        assert np.array_equal(_bits(p.solveForward(FREQS, theta)), _bits(fr))
    finally:
        eng.set_check(mode)


def test_shapes_and_mode_picture(monkeypatch):
    p = _problem("orthotropic", monkeypatch)
    orc = oracle_for(p)
    theta = p.parameters
    vr = p.vertex_rows()
    V = vr.shape[1]
    x = p.solveForwardField(FREQS, theta)
    shapes = p.solveForwardShapes(FREQS, theta)
    assert sorted(shapes) == ["u", "v", "w"]
    for k, name in enumerate("uvw"):
        assert shapes[name].shape == (FREQS.size, V) and shapes[name].dtype == np.complex128
        assert np.array_equal(_bits(shapes[name]), _bits(x[:, vr[k]]))
    # the boundary values of the clamped side, from the oracle's Dirichlet rows: x_d = b_d / A_dd
    c = orc.coefficients(theta)
    for q in (3, 66):
        A = orc.matrix(FREQS[q], c).tocsc()
        b = orc.rhs_vec * orc.rhs_scale(FREQS[q], c)
        d = _dirichlet_rows(A)
        want = b[d] / A.diagonal()[d]
        zero = want == 0
        assert zero.any() and (~zero).any()
        assert np.all(x[q][d[zero]] == 0)
        assert np.allclose(x[q][d[~zero]], want[~zero], rtol=1e-12, atol=0)
        for k, name in enumerate("uvw"):
            on = np.isin(vr[k], d)
            assert on.any()
            expect = b[vr[k][on]] / A.diagonal()[vr[k][on]]
            got = shapes[name][q][on]
            assert np.all(got[expect == 0] == 0) and np.allclose(got[expect != 0], expect[expect != 0], rtol=1e-12, atol=0)
        # the clamped w rows with a zero Dirichlet value are the edge normal derivatives, no vertex row
        assert np.all(p.vec[vr[2][np.isin(vr[2], d)]] != 0)
    f = float(FREQS[17])
    mesh, values = p.getModePicture(f, params=theta, plot=False)
    assert mesh is p.mesh and values.shape == (V,) and values.dtype == np.float64
    one = p.solveForwardField([f], theta, dofs=vr[2])[0]
    assert np.array_equal(values, np.abs(one))
    assert np.allclose(values, np.abs(x[17][vr[2]]), rtol=1e-9, atol=0)   # one frequency alone or lane 17 of 70
    with pytest.raises(NotImplementedError):
        p.getModePicture(f, use_freefem=True)


@pytest.mark.parametrize("prune", ["1", "0"])
def test_symmetric_laminate_has_no_in_plane_field(prune, monkeypatch):
    p = _problem("orthotropic", monkeypatch, prune=prune)
    assert p.material.is_mps
    x = p.solveForwardField(FREQS)
    L = p.Lh_size
    eng = p.engine()
    active = eng.solver.active_fronts()
    if prune == "1":
        assert 0 < active.sum() < active.size                          # the in-plane trees are not factorised
        assert np.all(_bits(x[:, :2 * L]) == 0)                         # exact +0.0
    else:
        assert active.all()
        # the in-plane block has no load: its solution is zero to the solve's backward error
        berr = eng.last_berr.cpu().numpy()[:, 0].max()
        assert berr < 1e-12
        assert np.abs(x[:, :2 * L]).max() <= 1e-12 * np.abs(x[:, 2 * L:]).max()
    assert np.abs(x[:, 2 * L:]).max() > 0


def test_oversize_request_is_refused_on_the_host(monkeypatch):
    p = _problem("orthotropic", monkeypatch)
    eng = p.engine()
    n, F = p.mat_size, FREQS.size
    need = F * (16 * n + 28)
    calls = []

    def no_sweep(*a, **k):
        calls.append(a)
        raise AssertionError("the device was touched")

    monkeypatch.setattr(eng, "field_sweep", no_sweep)
    monkeypatch.setattr(eng, "set_coefficients", no_sweep)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (int(need / 0.85) - 4096, 1 << 40))
    with pytest.raises(ValueError, match=f"{need:,}"):
        p.solveForwardField(FREQS)
    assert not calls
    # a selection that fits the same free memory is not refused by the size check
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (int(need / 0.85) + 4096, 1 << 40))
    with pytest.raises(AssertionError, match="the device was touched"):
        p.solveForwardField(FREQS)
    assert len(calls) == 1
