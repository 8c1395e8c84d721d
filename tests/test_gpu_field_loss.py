"""GPU: the field loss on the plate -- ``Problem.getFieldLossFunction`` / ``getFieldFunction`` / ``solveInverse`` with a
FIELD_* loss (pfr_field_loss_sweep under the engine's lanes) against a CPU adjoint built from the oracle's own matrices
and refined solves (tests/field_loss_oracle.py, checked against finite differences in tests/test_field_loss_cpu.py).
The engine is forced to two lanes (PFR_LANE_FREQS = 64 at 70 frequencies: blocks of 64 and 6), so the reference field
is cut into lane blocks.

Tolerances: the project's small-mesh ones of tests/test_gpu_parity.py -- the loss within 5e-9, the gradient within 1e-7
of its largest entry (two backward-stable fp64 solvers of these badly scaled systems differ by that much near the first
resonance).  The measured values are printed and go to $PFR_TEST_REPORT; on an MI355X: loss 7e-14 .. 6.2e-11, gradient
2.8e-11 .. 1.7e-9 over the two materials, two selections and three losses; L-BFGS on FIELD_MAC f / f_0 = 2.2e-10 after
39 iterations, parameter errors 5.1e-4, 4.8e-3, 3.6e-6, 4.3e-2, 2.5e-5 (E1, E2, G12, nu12, beta)."""
import numpy as np
import pytest
import torch

import field_loss_oracle as fo
import synthetic_fieldloss as sf
from helpers import make_problem, oracle_for, report

pytestmark = pytest.mark.gpu
FREQS = np.linspace(40.0, 600.0, 70)
LOSS_RTOL = 5e-9
GRAD_RTOL = 1e-7


def _problem(material, monkeypatch):
    monkeypatch.setenv("PFR_LANE_FREQS", "64")   # read when the engine is built
    monkeypatch.setenv("PFR_LANES", "2")
    p = make_problem(material, ny=4, device="cuda:0")
    eng = p.engine(FREQS.size)
    assert eng.n_lanes == 2 and [hi - lo for lo, hi in eng._split(FREQS.size)] == [64, 6]
    return p


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _theta(p):
    return p.parameters * (1 + 0.05 * np.linspace(-1, 1, p.parameters.size))


@pytest.mark.parametrize("every_row", [False, True], ids=["w-vertices", "all-rows"])
@pytest.mark.parametrize("material", ["orthotropic", "sol"])
def test_loss_and_gradient_against_the_oracle_adjoint(material, every_row, monkeypatch):
    p = _problem(material, monkeypatch)
    orc = oracle_for(p)
    rows = None if every_row else p.vertex_rows()[2]
    n_sel = p.mat_size if every_row else rows.size
    v = sf.weights(n_sel)
    # the data: the field at the true parameters with an amplitude and phase error per point
    x_true = orc.solutions(FREQS, p.parameters)
    data = sf.make_data(x_true if every_row else x_true[:, rows])
    theta = _theta(p)
    for lt in sf.LOSSES:
        loss_fn = p.getFieldLossFunction(FREQS, data, lt, dofs=rows, weights=v)
        t = torch.tensor(theta, requires_grad=True)
        val = loss_fn(t)
        val.backward()
        eng = p.engine()
        assert np.all(eng.last_flags == 0)
        berr = eng.last_berr.cpu().numpy()
        assert berr.shape == (FREQS.size, 2) and np.nanmax(berr) < 1e-12 and not np.any(np.isnan(berr))
        lo, go = fo.field_loss_and_grad(orc, FREQS, data, lt, theta, rows, v)
        e_loss, e_grad = abs(val.item() - lo) / abs(lo), _rel(t.grad.numpy(), go)
        print(f"{material} {'all rows' if every_row else 'w vertices'} {lt}: loss {val.item():.6e} rel {e_loss:.2e}, "
              f"grad rel {e_grad:.2e}")
        report(f"field loss {material} {n_sel} {lt}", loss_rel=e_loss, grad_rel=e_grad)
        assert e_loss < LOSS_RTOL
        assert e_grad < GRAD_RTOL


def test_autograd_through_the_field(monkeypatch):
    """FIELD_MSE written in torch on ``getFieldFunction``'s field: the value and gradient of ``getFieldLossFunction``
    (the same forward solves; the backward is one FCOTANGENT sweep with conj(grad_out))."""
    p = _problem("orthotropic", monkeypatch)
    rows = p.vertex_rows()[2]
    v = sf.weights(rows.size)
    theta = _theta(p)
    data = sf.make_data(p.solveForwardField(FREQS, dofs=rows))
    t1 = torch.tensor(theta, requires_grad=True)
    l1 = p.getFieldLossFunction(FREQS, data, "FIELD_MSE", dofs=rows, weights=v)(t1)
    l1.backward()
    t2 = torch.tensor(theta, requires_grad=True)
    x = p.getFieldFunction(dofs=rows)(FREQS, t2)
    assert x.shape == (FREQS.size, rows.size) and x.dtype == torch.complex128 and x.is_cuda
    d = x - torch.as_tensor(data, device=x.device)
    l2 = (torch.as_tensor(v, device=x.device) * (d.real ** 2 + d.imag ** 2)).sum() / FREQS.size
    l2.backward()
    e_loss, e_grad = abs(l2.item() - l1.item()) / abs(l1.item()), _rel(t2.grad.numpy(), t1.grad.numpy())
    print(f"autograd through the field: loss rel {e_loss:.2e}, grad rel {e_grad:.2e}")
    report("field autograd", loss_rel=e_loss, grad_rel=e_grad)
    # the same x to the bit; the sums in another order, the adjoint solved for the seed torch formed
    assert e_loss < 1e-13
    assert e_grad < GRAD_RTOL
    assert np.all(p.engine().last_flags == 0)


def test_lbfgs_on_the_mac_of_the_true_field():
    """solveInverse(FIELD_MAC, lbfgs) from the start of test_gpu_inverse.test_lbfgs_recovers_parameters, on the w
    vertex field at the true parameters: the accepted iterates decrease strictly.  f / f_0 and the parameter errors
    are reported; no recovery threshold is asserted (none has been measured)."""
    p = make_problem("orthotropic", ny=4, device="cuda:0")
    freq = np.linspace(40, 600, 256)
    rows = p.vertex_rows()[2]
    field = p.solveForwardField(freq, dofs=rows)
    res = p.solveInverse([0.03, -0.03, 0.04, 0.02, 0.1], 'FIELD_MAC', 'lbfgs', ref_field=(freq, field),
                         field_dofs=rows, use_rel=True, use_scaling=True, log=False, report=False, N_steps=40)
    f = np.array(list(res.f_history) + [res.f])
    rel = np.abs(res.x - p.parameters) / p.parameters
    print(f"lbfgs FIELD_MAC: f / f_0 = {f[-1] / f[0]:.3e} after {res.niter} iterations ({res.status}); "
          f"parameter errors {np.array2string(rel, precision=3)}")
    report("field mac lbfgs", f_ratio=float(f[-1] / f[0]), **{f"rel{i}": float(r) for i, r in enumerate(rel)})
    accepted = np.array(res.f_history)
    assert accepted.size >= 2 and np.all(np.isfinite(f))
    assert np.all(np.diff(accepted) < 0)
    assert f[-1] <= accepted[-1]
