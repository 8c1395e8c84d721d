"""GPU: the per-frequency Jacobian through the Python interface (Problem.getFRJacobianFunction and what is built on
it: the least-squares residual, Levenberg-Marquardt in solveInverse, the parameter covariance), against the CPU
oracle's adjoint Jacobian at the parity tolerances of tests/test_gpu_parity.py."""
import numpy as np
import pytest
import torch

from helpers import make_problem, oracle_for, report
from test_gpu_parity import FR_RTOL, GRAD_RTOL

pytestmark = pytest.mark.gpu

LOSSES = ("MSE", "RMSE", "MSE_AFC", "MSE_LOG_AFC")
START = [0.03, -0.03, 0.04, 0.02, 0.1]          # tests/test_gpu_inverse.py::test_lbfgs_recovers_parameters


def _oracle_jacobian(p, freqs, theta):
    """(fr, J) of the oracle: one adjoint solve per frequency -- frequency_partials with MSE and a zero reference has
    the term fr^2, so its w is that of the cotangent 2 fr and the row is Re(w J_c) / (2 fr)."""
    from oracle.plate_oracle import coeffs18_jacobian, frequency_partials
    orc = oracle_for(p)
    Jc = coeffs18_jacobian(orc.atype, orc.h, np.asarray(theta, dtype=np.float64), orc.angles)
    fr, rows = [], []
    for f in freqs:
        lsum, w = frequency_partials(orc, [f], np.zeros(1, dtype=complex), "MSE", theta, n_total=1)
        fr.append(np.sqrt(lsum))
        rows.append(np.real(w @ Jc) / (2 * fr[-1]))
    return np.array(fr), np.array(rows)


def _col_err(J, Jo):
    """max_q |dJ| / max_q |J| per parameter column."""
    return np.max(np.abs(J - Jo), axis=0) / np.max(np.abs(Jo), axis=0)


@pytest.mark.parametrize("material,ny,nfreq", [("orthotropic", 5, 48), ("sol", 4, 32)])
def test_jacobian_against_the_oracle(material, ny, nfreq):
    p = make_problem(material, ny=ny, device="cuda:0")
    freqs = np.linspace(40.0, 600.0, nfreq)
    fr, J = p.solveForwardJacobian(freqs)
    assert fr.shape == (nfreq,) and J.shape == (nfreq, p.parameters.size)
    assert p.engine().n_stiff == (18 if material == "sol" else 12)
    fro, Jo = _oracle_jacobian(p, freqs, p.parameters)
    efr, ecol = float(np.max(np.abs(fr - fro) / np.abs(fro))), _col_err(J, Jo)
    print(f"{material}: fr {efr:.2e}, J columns {ecol}")
    report("jacobian " + material, fr_rel=efr, col_rel=list(ecol))
    assert efr < FR_RTOL
    assert np.all(ecol < GRAD_RTOL), ecol
    assert np.all(p.engine().last_flags == 0)


def test_rows_against_autograd_over_chunks():
    """151 frequencies through 64-frequency chunks (the last padded): three rows against torch.autograd.grad of
    getFRFunction's fr[q] (one cotangent sweep each).  Both are within GRAD_RTOL of the exact row."""
    p = make_problem("isotropic", ny=4, device="cuda:0", max_batch=64)
    freqs = np.linspace(40.0, 600.0, 151)
    fr, J = p.solveForwardJacobian(freqs)
    fn = p.getFRFunction()
    errs = []
    for q in (0, 64, 150):
        x = torch.tensor(p.parameters, requires_grad=True)
        out = fn(freqs, x)
        (g,) = torch.autograd.grad(out[q], x)
        assert abs(out[q].item() - fr[q]) <= FR_RTOL * abs(fr[q])
        errs.append(float(np.max(np.abs(J[q] - g.numpy()) / np.max(np.abs(J[:, :]), axis=0))))
    print("rows against autograd:", errs)
    report("jacobian rows vs autograd", rel=errs)
    assert max(errs) < 2 * GRAD_RTOL, errs


def test_scaling_params():
    p = make_problem("orthotropic", ny=4, device="cuda:0")
    freqs = np.linspace(60.0, 580.0, 24)
    s = p.parameters
    x = np.array([1.02, 0.97, 1.05, 1.0, 1.1])
    fr0, J0 = p.getFRJacobianFunction()(freqs, x * s)
    fr1, J1 = p.getFRJacobianFunction(scaling_params=s)(freqs, x)
    assert fr1.is_cuda and J1.is_cuda and fr1.dtype == J1.dtype == torch.float64
    J0, J1 = J0.cpu().numpy(), J1.cpu().numpy()
    assert np.array_equal(fr0.cpu().numpy(), fr1.cpu().numpy())
    assert np.max(np.abs(J1 - J0 * s) / np.max(np.abs(J0 * s), axis=0)) < 1e-14


@pytest.mark.parametrize("loss_type", LOSSES)
def test_residual_function_matches_the_loss(loss_type):
    p = make_problem("orthotropic", ny=5, device="cuda:0")
    freqs = np.linspace(40.0, 600.0, 48)
    ref = p.solveForward(freqs) * np.exp(1j * 0.1)
    theta = p.parameters * (1 + np.array([0.1, 0.1, 0.2, 0.1, 0.1]))
    x = torch.tensor(theta, requires_grad=True)
    val = p.getLossFunction(freqs, ref, loss_type)(x)
    val.backward()
    r, Jr, const = p.getResidualFunction(freqs, ref, loss_type)(theta)
    F = freqs.size
    assert r.shape == (F,) and Jr.shape == (F, theta.size)
    el = abs((r @ r + const) / F - val.item()) / abs(val.item())
    g = 2.0 / F * Jr.T @ r
    eg = float(np.max(np.abs(g - x.grad.numpy())) / np.max(np.abs(x.grad.numpy())))
    print(f"{loss_type}: loss {el:.2e}, gradient {eg:.2e}")
    report("residual " + loss_type, loss_rel=el, grad_rel=eg)
    assert el < FR_RTOL
    assert eg < 2 * GRAD_RTOL


def test_lm_through_solve_inverse():
    """solveInverse(..., 'lm') on the problem and start of test_lbfgs_recovers_parameters.  Measured on an MI355X
    (DESIGN.md section 5.1): 20 accepted iterates, f / f_0 = 1.9e-7, relative errors E1 3.6e-2, G12 3.3e-3.  The
    loss clears the L-BFGS test's 1e-5 by 50 x, E1 and G12 do not clear its 1e-3 (the steps move along the E1 / E2 /
    nu12 valley of D11), so only the strict decrease is asserted."""
    p = make_problem("orthotropic", ny=4, device="cuda:0")
    freq = np.linspace(40, 600, 256)
    fr = p.solveForward(freq)
    res = p.solveInverse(START, 'MSE_LOG_AFC', 'lm', ref_fr=[freq, fr], use_rel=True, use_scaling=True, log=False,
                         report=False, N_steps=20)
    rel = np.abs(res.x - p.parameters) / p.parameters
    ratio = res.f / res.f_history[0]
    print(f"lm: f / f0 = {ratio:.3e} after {len(res.f_history)} accepted iterates ({res.status}); rel {rel}")
    report("lm inverse", f_ratio=ratio, rel=list(rel), accepted=len(res.f_history))
    assert all(a > b for a, b in zip(res.f_history, res.f_history[1:]))
    assert res.f < res.f_history[0]
    with pytest.raises(NotImplementedError):
        p.solveInverse(START, 'MSE_LOG_AFC', 'lm', ref_fr=[freq, fr], use_rel=True, distributed=True, log=False,
                       report=False)


def test_parameter_covariance():
    """At the L-BFGS test's start in scaled parameters (std relative to the true moduli): symmetric, the numpy
    formula on getResidualFunction's output, and the identifiability statement of that test -- E1 and G12 are
    determined better than E2."""
    p = make_problem("orthotropic", ny=4, device="cuda:0")
    freq = np.linspace(40, 600, 256)
    ref = p.solveForward(freq)
    s, x = p.parameters, 1 + np.array(START)
    cov, std = p.parameterCovariance(freq, ref, 'MSE_LOG_AFC', params=x, scaling_params=s)
    r, Jr, const = p.getResidualFunction(freq, ref, 'MSE_LOG_AFC', scaling_params=s)(x)
    # the numpy formula, the normal matrix scaled to a unit diagonal before it is inverted (E1, E2 and nu12 enter the
    # strip's bending stiffness almost only through D11: the matrix is close to singular); two inversions of a
    # matrix of condition c agree to ~c eps each, hence the tolerance
    N = Jr.T @ Jr
    d = np.sqrt(np.diag(N))
    Ns = N / np.outer(d, d)
    c = float(np.linalg.cond(Ns))
    want = (r @ r + const) / (freq.size - x.size) * np.linalg.inv(Ns) / np.outer(d, d)
    diff = float(np.max(np.abs(cov - want) / np.sqrt(np.outer(np.diag(want), np.diag(want)))))
    print("relative std (E1, E2, G12, nu12, beta):", std, f"cond {c:.2e}, against numpy {diff:.2e}")
    report("parameter covariance", std=list(std), cond=c, diff=diff)
    assert cov.shape == (5, 5) and np.array_equal(cov, cov.T)
    assert diff <= 100 * c * np.finfo(float).eps, (diff, c)
    np.testing.assert_allclose(std, np.sqrt(np.diag(cov)))
    # measured on an MI355X: 218, 1269, 0.66, 18822, ...: G12 by three orders, E1 by 5.8 x
    assert std[0] < std[1] and std[2] < std[1], std
