"""GPU: the complex response through the Python interface (Problem.getTFFunction and what is built on it: the three
complex losses, the per-frequency Jacobian, the least-squares residual, solveInverse, the parameter covariance, the
distributed loss) on the plate, against the CPU oracle's own primitives at the parity tolerances of
tests/test_gpu_parity.py (the small-mesh tolerances)."""
import os

import numpy as np
import pytest
import torch

import synthetic_complex as sc
from helpers import make_problem, oracle_for, report
from test_gpu_parity import FR_RTOL, GRAD_RTOL, _rel

pytestmark = pytest.mark.gpu

CASES = [("orthotropic", 4), ("sol", 4)]
FREQS = np.linspace(40.0, 600.0, 70)
AXIS = (0.6, 0.8, 1.0)
START = [0.03, -0.03, 0.04, 0.02, 0.1]          # tests/test_gpu_inverse.py::test_lbfgs_recovers_parameters


def _oracle_h(orc, sols, axis):
    ts = orc.acc_ts
    return np.array([axis[0] * ts * U + axis[1] * ts * V + axis[2] * W for U, V, W in map(orc.uvw, sols)])


def _h_err(H, Ho):
    return float(np.max(np.abs(H - Ho) / np.maximum(np.abs(Ho), 1e-3 * np.max(np.abs(Ho)))))


@pytest.mark.parametrize("material,ny", CASES)
@pytest.mark.parametrize("axis", [(0, 0, 1), AXIS], ids=["z", "tilted"])
def test_forward_against_the_oracle(material, ny, axis):
    p = make_problem(material, ny=ny, device="cuda:0")
    H = p.solveForwardComplex(FREQS, axis=axis)
    assert H.shape == (FREQS.size,) and H.dtype == np.complex128
    orc = oracle_for(p)
    Ho = _oracle_h(orc, orc.solutions(FREQS, p.parameters), axis)
    err = _h_err(H, Ho)
    print(f"{material} axis={axis}: H {err:.2e}")
    report(f"complex forward {material} {axis}", h_rel=err, ratio=err / FR_RTOL)
    assert err <= FR_RTOL
    assert np.all(p.engine().last_flags == 0)


def _oracle_loss_grad(orc, freqs, ref, loss_type, theta, axis):
    """(loss, gradient) by the adjoint method from the oracle's own primitives: per frequency one sparse LU, the
    refined forward solve, H and the loss's cotangent g, the refined transposed solve with g a_d, the partials
    w_k = -lam^T S_k x + e_k lam^T rhs; then Re(w J) with the oracle's coefficient Jacobian."""
    from oracle.plate_oracle import RHS_WEIGHTS_D, coeffs18_jacobian, refined_solve, sparse_lu
    c = orc.coefficients(theta)
    aU, aV, aW = orc.averaging_vectors()
    ts = orc.acc_ts
    ad = axis[0] * ts * aU + axis[1] * ts * aV + axis[2] * aW
    e = np.concatenate([np.zeros(12), RHS_WEIGHTS_D])
    w = np.zeros(18, dtype=complex)
    total = 0.0
    for f, r in zip(freqs, ref):
        A = orc.matrix(f, c)
        lu = sparse_lu(A)
        x = refined_solve(lu, A, orc.rhs_vec * orc.rhs_scale(f, c))
        term, g = sc.loss_c(np.complex128(ad @ x), r, loss_type)
        total += float(term)
        lam = refined_solve(lu, A, (g / freqs.size) * ad, trans=True)
        w += -(orc.mats[:18] @ (lam[orc.rows] * x[orc.cols])) + e * (lam @ orc.rhs_vec)
    J = coeffs18_jacobian(orc.atype, orc.h, np.asarray(theta, dtype=np.float64), orc.angles)
    return total / freqs.size, np.real(w @ J)


@pytest.mark.parametrize("material,ny", CASES)
@pytest.mark.parametrize("loss_type", sc.LOSSES)
def test_loss_and_gradient_against_the_oracle(loss_type, material, ny):
    p = make_problem(material, ny=ny, device="cuda:0")
    ref = p.solveForwardComplex(FREQS, axis=AXIS) * 1.03 * np.exp(0.05j)
    theta = p.parameters * 1.05
    x = torch.tensor(theta, requires_grad=True)
    val = p.getLossFunction(FREQS, ref, loss_type, axis=AXIS)(x)
    val.backward()
    lo, go = _oracle_loss_grad(oracle_for(p), FREQS, ref, loss_type, theta, AXIS)
    el, eg = abs(val.item() - lo) / abs(lo), _rel(x.grad.numpy(), go)
    print(f"{material} {loss_type}: loss {el:.2e}, gradient {eg:.2e}")
    report(f"complex loss {material} {loss_type}", loss_rel=el, grad_rel=eg, loss_ratio=el / FR_RTOL,
           grad_ratio=eg / GRAD_RTOL)
    assert el <= FR_RTOL
    assert eg <= GRAD_RTOL
    assert np.all(p.engine().last_flags == 0)


@pytest.mark.parametrize("material,ny", CASES)
def test_autograd_through_the_transfer_function(material, ny):
    """torch.autograd.grad through getTFFunction with a fixed complex cotangent (one PFR_LOSS_CCOTANGENT sweep)
    against Re(conj(cot) @ dH) from getTFJacobianFunction: both are within GRAD_RTOL of the exact gradient."""
    p = make_problem(material, ny=ny, device="cuda:0")
    rng = np.random.default_rng(21)
    cot = (0.5 + rng.random(FREQS.size)) * np.exp(2j * np.pi * rng.random(FREQS.size))
    theta = p.parameters * 1.05
    x = torch.tensor(theta, requires_grad=True)
    H = p.getTFFunction(AXIS)(FREQS, x)
    assert H.is_cuda and H.dtype == torch.complex128
    (g,) = torch.autograd.grad(H, x, grad_outputs=torch.as_tensor(cot, device=H.device))
    Hj, dH = p.getTFJacobianFunction(axis=AXIS)(FREQS, theta)
    assert dH.shape == (FREQS.size, theta.size) and dH.dtype == torch.complex128
    want = np.real(np.conj(cot) @ dH.cpu().numpy())
    eh, eg = _h_err(Hj.cpu().numpy(), H.detach().cpu().numpy()), _rel(g.numpy(), want)
    print(f"{material}: H of the two sweeps {eh:.2e}, autograd against the rows {eg:.2e}")
    report(f"complex autograd {material}", h_rel=eh, grad_rel=eg, grad_ratio=eg / (2 * GRAD_RTOL))
    assert eh <= 2 * FR_RTOL
    assert eg <= 2 * GRAD_RTOL


@pytest.mark.parametrize("loss_type", sc.LOSSES)
def test_residual_function_matches_the_loss(loss_type):
    p = make_problem("orthotropic", ny=4, device="cuda:0")
    ref = p.solveForwardComplex(FREQS, axis=AXIS) * 1.03 * np.exp(0.05j)
    theta = p.parameters * 1.05
    x = torch.tensor(theta, requires_grad=True)
    val = p.getLossFunction(FREQS, ref, loss_type, axis=AXIS)(x)
    val.backward()
    r, Jr, const = p.getResidualFunction(FREQS, ref, loss_type, axis=AXIS)(theta)
    F = FREQS.size
    assert r.shape == (2 * F,) and Jr.shape == (2 * F, theta.size) and const == 0.0
    el = abs(r @ r / F - val.item()) / abs(val.item())
    eg = _rel(2.0 / F * Jr.T @ r, x.grad.numpy())
    print(f"{loss_type}: loss {el:.2e}, gradient {eg:.2e}")
    report("complex residual " + loss_type, loss_rel=el, grad_rel=eg)
    assert el <= FR_RTOL
    assert eg <= 2 * GRAD_RTOL


@pytest.mark.parametrize("optimizer,steps", [("lm", 20), ("lbfgs", 40)])
def test_solve_inverse_decreases_the_complex_loss(optimizer, steps):
    """solveInverse(..., 'MSE_LOG_COMPLEX', ...) from the start of test_lm_through_solve_inverse: the loss strictly
    decreases over the accepted iterates (all that test asserts)."""
    p = make_problem("orthotropic", ny=4, device="cuda:0")
    freq = np.linspace(40, 600, 256)
    H = p.solveForwardComplex(freq)
    res = p.solveInverse(START, 'MSE_LOG_COMPLEX', optimizer, ref_fr=[freq, H], use_rel=True, use_scaling=True,
                         log=False, report=False, N_steps=steps)
    rel = np.abs(res.x - p.parameters) / p.parameters
    ratio = res.f / res.f_history[0]
    print(f"{optimizer}: f / f0 = {ratio:.3e} after {len(res.f_history)} iterates ({res.status}); rel {rel}")
    report("complex inverse " + optimizer, f_ratio=ratio, rel=list(rel), accepted=len(res.f_history))
    assert res.f < res.f_history[0]
    if optimizer == "lm":
        assert all(a > b for a, b in zip(res.f_history, res.f_history[1:]))


def test_parameter_covariance():
    p = make_problem("orthotropic", ny=4, device="cuda:0")
    freq = np.linspace(40, 600, 256)
    ref = p.solveForwardComplex(freq)
    s, x = p.parameters, 1 + np.array(START)
    cov, std = p.parameterCovariance(freq, ref, 'MSE_LOG_COMPLEX', params=x, scaling_params=s)
    print("relative std (E1, E2, G12, nu12, beta):", std)
    report("complex parameter covariance", std=list(std))
    assert cov.shape == (5, 5) and np.all(np.isfinite(cov)) and np.array_equal(cov, cov.T)
    assert np.all(np.isfinite(std)) and np.all(std > 0)


def test_unsupported_paths_raise():
    p = make_problem("orthotropic", ny=4, device="cuda:0")
    ref = np.ones(FREQS.size, dtype=complex)
    for name in sc.LOSSES:
        with pytest.raises(ValueError):
            p.getLossHessianFunction(FREQS, ref, name)
        with pytest.raises(ValueError):
            p.getPopulationLossFunction(FREQS, ref, name)
    with pytest.raises(ValueError):
        p.getLossFunction(FREQS, ref, "MSE_LOG_AFC", axis=AXIS)
    with pytest.raises(ValueError):
        p.getTFFunction((0, 0, 0))


def test_distributed_loss_at_world_size_one(tmp_path):
    """getLossFunction(..., distributed=True) in a one-rank gloo group (the packed loss / w all-reduce runs) equals
    the plain loss to the bits."""
    import torch.distributed as dist
    from plate_inverse_problem_amd import distributed as pdist
    p = make_problem("orthotropic", ny=4, device="cuda:0")
    ref = p.solveForwardComplex(FREQS, axis=AXIS) * 1.03 * np.exp(0.05j)
    theta = p.parameters * 1.05
    y = torch.tensor(theta, requires_grad=True)
    plain = p.getLossFunction(FREQS, ref, "MSE_LOG_COMPLEX", axis=AXIS)(y)
    plain.backward()
    dist.init_process_group("gloo", store=dist.FileStore(os.path.join(tmp_path, "store"), 1), rank=0, world_size=1)
    try:
        n0 = pdist.N_COLLECTIVES
        x = torch.tensor(theta, requires_grad=True)
        v = p.getLossFunction(FREQS, ref, "MSE_LOG_COMPLEX", axis=AXIS, distributed=True)(x)
        v.backward()
        assert pdist.N_COLLECTIVES == n0 + 1
    finally:
        dist.destroy_process_group()
    eg = _rel(x.grad.numpy(), y.grad.numpy())
    print(f"distributed against plain: loss {v.item()!r} / {plain.item()!r}, gradient {eg:.2e}")
    assert v.item() == plain.item()
    assert eg <= 1e-12
