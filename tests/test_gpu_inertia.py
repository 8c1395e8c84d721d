"""GPU: the inertia sweep through the Python interface (the ``extra`` parameters rho, h and acc_mass of
Problem.getFRJacobianFunction and what is built on it, Problem.solveForwardSlope), against the CPU oracle's adjoint
rows at the parity tolerances of tests/test_gpu_parity.py."""
import dataclasses

import numpy as np
import pytest
import torch

from helpers import make_problem, oracle_for, report
from test_gpu_jacobian import _col_err
from test_gpu_parity import FR_RTOL, GRAD_RTOL
from test_inertia_cpu import _oracle_rows

pytestmark = pytest.mark.gpu

EXTRA = ("rho", "h", "acc_mass")
CASES = [("orthotropic", 5, 48), ("sol", 4, 32)]
MOVED = np.array([1.03, 0.98, 1.1])                      # rho x 1.03, h x 0.98, acc_mass x 1.1

_P = {}


def _problem(material, ny):
    """One Problem (and engine) per case for the whole module."""
    if (material, ny) not in _P:
        _P[material, ny] = make_problem(material, ny=ny, device="cuda:0")
    return _P[material, ny]


def _oracle(p, freqs, ext):
    """(fr, J (F, n_mat + 3), slope) of the oracle at the extended vector ``ext``: the material columns from its
    adjoint rows and the 4th-order differences of its transform at the thickness in ``ext``, the extra columns and
    the frequency slope from the same rows by the inertia formula (test_inertia_cpu._oracle_rows)."""
    from oracle.plate_oracle import coeffs18_jacobian, inertia
    acc = p.accelerometer
    theta, (rho, h, m) = ext[:-3], ext[-3:]
    orc = dataclasses.replace(oracle_for(p), I=inertia(h, rho, m, acc.radius, acc.height), h=h)
    fr, rows, jc = _oracle_rows(orc, acc, rho, freqs, theta, acc_mass=m)
    Jc = coeffs18_jacobian(orc.atype, h, theta, orc.angles)
    return fr, np.concatenate([np.real(jc @ Jc), rows[:, :3]], axis=1), rows[:, 3]


@pytest.mark.parametrize("moved", [False, True], ids=["own", "moved"])
@pytest.mark.parametrize("material,ny,nfreq", CASES)
def test_extended_jacobian_against_the_oracle(material, ny, nfreq, moved):
    p = _problem(material, ny)
    freqs = np.linspace(40.0, 600.0, nfreq)
    n_mat = p.parameters.size
    before = p.solveForward(freqs)
    fr0, J0 = p.solveForwardJacobian(freqs)
    ext = p.extendedParameters(EXTRA)
    if moved:
        ext[n_mat:] *= MOVED
    fr, J = p.solveForwardJacobian(freqs, ext, extra=EXTRA)
    assert fr.shape == (nfreq,) and J.shape == (nfreq, n_mat + 3)
    fro, Jo, _ = _oracle(p, freqs, ext)
    efr, ecol = float(np.max(np.abs(fr - fro) / np.abs(fro))), _col_err(J, Jo)
    print(f"{material} {'moved' if moved else 'own'}: fr {efr:.2e}, J columns {ecol}")
    report(f"inertia {material} {'moved' if moved else 'own'}", fr_rel=efr, col_rel=list(ecol))
    assert efr < FR_RTOL
    assert np.all(ecol < GRAD_RTOL), ecol
    assert np.all(p.engine().last_flags == 0)
    if not moved:
        # at the problem's own values: fr and the material columns are the bits of the call without extra
        assert np.array_equal(fr, fr0) and np.array_equal(J[:, :n_mat], J0)
    else:
        assert not np.array_equal(fr, fr0)
    # the problem's own values are back: the earlier bits again, on every path
    assert p.engine().inertia == p.engine().own_inertia
    assert np.array_equal(p.solveForward(freqs), before)
    fr1, J1 = p.solveForwardJacobian(freqs)
    assert np.array_equal(fr1, fr0) and np.array_equal(J1, J0)


def test_subset_and_scaling():
    """extra=('h',) alone, with scaling_params over the whole vector: J is with respect to the scaled parameters."""
    p = _problem("orthotropic", 5)
    freqs = np.linspace(40.0, 600.0, 48)
    ext = p.extendedParameters(("h",))
    fr, J = p.solveForwardJacobian(freqs, ext, extra=("h",))
    frs, Js = p.getFRJacobianFunction(scaling_params=ext, extra=("h",))(freqs, np.ones(ext.size))
    full = p.solveForwardJacobian(freqs, p.extendedParameters(EXTRA), extra=EXTRA)[1]
    np.testing.assert_allclose(J[:, -1], full[:, -2], rtol=1e-12)
    assert np.array_equal(frs.cpu().numpy(), fr)
    np.testing.assert_allclose(Js.cpu().numpy(), J * ext[None, :], rtol=1e-12)
    with pytest.raises(ValueError):
        p.getFRJacobianFunction(extra=("thickness",))


@pytest.mark.parametrize("material,ny,nfreq", CASES)
def test_frequency_slope(material, ny, nfreq):
    p = _problem(material, ny)
    freqs = np.linspace(40.0, 600.0, nfreq)
    fr, slope = p.solveForwardSlope(freqs)
    fro, _, so = _oracle(p, freqs, p.extendedParameters(EXTRA))
    err = float(np.max(np.abs(slope - so)) / np.max(np.abs(so)))
    print(f"{material}: slope {err:.2e}")
    report(f"inertia slope {material}", slope_rel=err)
    assert np.max(np.abs(fr - fro) / np.abs(fro)) < FR_RTOL and err < GRAD_RTOL
    assert np.array_equal(fr, p.solveForwardJacobian(freqs)[0])      # the Jacobian sweep's fr, to the bit


def test_complex_response_columns():
    """getTFJacobianFunction(extra=...): H and the material columns are the bits of the call without extra; the
    density column (complex, no real part taken) predicts H at a density 1e-4 higher to second order."""
    p = _problem("orthotropic", 5)
    freqs = np.linspace(40.0, 600.0, 48)
    ext = p.extendedParameters(EXTRA)
    H0, dH0 = p.getTFJacobianFunction()(freqs, p.parameters)
    H, dH = p.getTFJacobianFunction(extra=EXTRA)(freqs, ext)
    assert torch.equal(H, H0) and torch.equal(dH[:, :p.parameters.size], dH0)
    assert dH.shape == (48, ext.size) and dH.dtype == torch.complex128
    ext2 = ext.copy()
    ext2[-3] *= 1.0001
    H2, _ = p.getTFJacobianFunction(extra=EXTRA)(freqs, ext2)
    lin = H + dH[:, -3] * (ext2[-3] - ext[-3])
    assert float((H2 - lin).abs().max() / (H2 - H).abs().max()) < 2e-2


@pytest.mark.parametrize("func_type", ["MSE_LOG_AFC", "RMSE"])
def test_residual_and_loss(func_type):
    """getResidualFunction(extra=...): shapes; 2 Jr^T r / F is getLossFunction(extra=...)'s gradient; the loss matches
    the oracle's at the moved values."""
    from oracle.plate_oracle import inertia, loss as oracle_loss
    p = _problem("orthotropic", 5)
    freqs = np.linspace(40.0, 600.0, 48)
    ref = p.solveForward(freqs) * 1.01 * np.exp(0.05j)
    ext = p.extendedParameters(EXTRA)
    ext[-3:] *= MOVED
    r, Jr, const = p.getResidualFunction(freqs, ref, func_type, extra=EXTRA)(ext)
    assert r.shape == (48,) and Jr.shape == (48, ext.size)
    x = torch.tensor(ext, requires_grad=True)
    val = p.getLossFunction(freqs, ref, func_type, extra=EXTRA)(x)
    val.backward()
    np.testing.assert_allclose(val.item(), (r @ r + const) / 48, rtol=1e-13)
    np.testing.assert_allclose(x.grad.numpy(), 2 * Jr.T @ r / 48, rtol=1e-12)
    acc = p.accelerometer
    orc = dataclasses.replace(oracle_for(p), I=inertia(ext[-2], ext[-3], ext[-1], acc.radius, acc.height), h=ext[-2])
    lo = oracle_loss(orc, freqs, ref, func_type, ext[:-3])
    print(f"{func_type}: loss {val.item():.6e} oracle {lo:.6e}")
    assert abs(val.item() - lo) <= FR_RTOL * abs(lo)
    with pytest.raises(NotImplementedError):
        p.getLossFunction(freqs, ref, func_type, extra=EXTRA, distributed=True)


def test_out_of_scope_paths_say_so():
    p = _problem("orthotropic", 5)
    freqs = np.linspace(40.0, 600.0, 8)
    ref = np.ones(8, dtype=complex)
    for make in (lambda: p.getLossHessianFunction(freqs, ref, "MSE", extra=("rho",)),
                 lambda: p.getPopulationLossFunction(freqs, ref, "MSE", extra=("rho",)),
                 lambda: p.getFieldLossFunction(freqs, np.ones((8, 2), dtype=complex), "FIELD_MSE", dofs=[0, 1],
                                                extra=("rho",)),
                 lambda: p.solveInverse([0.0] * 6, "MSE", "tr", ref_fr=[freqs, ref], extra=("rho",), log=False,
                                        report=False)):
        with pytest.raises(NotImplementedError, match="inertia"):
            make()


def test_covariance_with_density():
    """parameterCovariance(extra=('rho',)): (p + 1, p + 1), symmetric; rho's correlation with each modulus is reported."""
    p = _problem("orthotropic", 5)
    freqs = np.linspace(40.0, 600.0, 48)
    rng = np.random.default_rng(0)
    ref = p.solveForward(freqs) * (1 + 0.01 * rng.standard_normal(48))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # a singular Jr^T Jr is the verdict, not a failure
        cov, std = p.parameterCovariance(freqs, ref, "MSE_LOG_AFC", extra=("rho",))
    n = p.parameters.size + 1
    assert cov.shape == (n, n) and std.shape == (n,) and np.array_equal(cov, cov.T)
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = cov[-1, :-1] / (std[-1] * std[:-1])
    print("rho: std / value", std[-1] / p.rho, "correlation with the material parameters", corr)
    report("inertia covariance rho", rho_rel_std=float(std[-1] / p.rho), corr=[float(c) for c in np.nan_to_num(corr)])


def test_lm_recovers_the_accelerometer_mass():
    """solveInverse(..., 'lm', extra=('acc_mass',)): data from the GPU's own forward at a known mass, the start 10 %
    off with the material at truth: the loss history decreases strictly and the mass ends closer than it began."""
    p = _problem("orthotropic", 5)
    freqs = np.linspace(40.0, 600.0, 48)
    truth = p.extendedParameters(("acc_mass",))
    truth[-1] *= 1.2
    data, _ = p.solveForwardJacobian(freqs, truth, extra=("acc_mass",))
    start = truth.copy()
    start[-1] *= 1.1
    res = p.solveInverse(start, "MSE_LOG_AFC", "lm", ref_fr=[freqs, data.astype(complex)], use_scaling=True,
                         extra=("acc_mass",), log=False, report=False, N_steps=8)
    hist = list(res.f_history)
    print("loss history", hist, "mass error", abs(res.x[-1] / truth[-1] - 1), "from 0.1")
    report("inertia lm acc_mass", first=hist[0], last=hist[-1], mass_err=float(abs(res.x[-1] / truth[-1] - 1)))
    assert len(hist) >= 2 and all(b < a for a, b in zip(hist, hist[1:]))
    assert abs(res.x[-1] / truth[-1] - 1) < 0.1
    assert p.engine().inertia == p.engine().own_inertia
