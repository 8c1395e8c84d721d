"""GPU: the population sweep through the Python interface (Problem.solveForwardPopulation,
Problem.getPopulationLossFunction, solveInverse(..., 'de', vectorized=True)) on the plate: every member against the
CPU oracle at the small-mesh parity tolerances (tests/test_gpu_parity.py: fr / loss 5e-9 relative, gradient 1e-7 of
its largest component) and against the sequential getLossFunction calls at twice those -- both sides are within the
tolerance of the exact value, and the sequential calls run narrower sweeps on other launch forms, so that comparison
is not bitwise."""
import numpy as np
import pytest
import torch

from helpers import make_problem, oracle_for, report
from test_gpu_parity import FR_RTOL, GRAD_RTOL, _rel

pytestmark = pytest.mark.gpu

LOSSES = ("MSE_LOG_AFC", "MSE")
DELTA = np.array([[0.0, 0.0, 0.0, 0.0, 0.0], [0.1, 0.1, 0.1, 0.1, 0.1], [-0.1, 0.05, -0.05, 0.1, -0.1],
                  [0.03, -0.03, 0.04, 0.02, 0.1], [-0.07, -0.1, 0.1, -0.02, 0.06]])      # |delta| <= 0.1


class _Case:
    """One problem, its population and the oracle's values, computed once for the module."""

    def __init__(self, material, ny, members, nfreq, losses):
        from oracle.plate_oracle import loss_and_grad
        self.p = make_problem(material, ny=ny, device="cuda:0")
        self.freqs = np.linspace(40.0, 600.0, nfreq)
        t0 = self.p.parameters
        d = DELTA[:members, :t0.size] if t0.size <= 5 else np.pad(DELTA[:members], ((0, 0), (0, t0.size - 5)))
        self.thetas = t0 * (1 + d)
        orc = oracle_for(self.p)
        self.ref = orc.fr(self.freqs, t0 * 1.02) * np.exp(1j * 0.1)            # a complex reference no member fits
        self.fr = np.stack([orc.fr(self.freqs, t) for t in self.thetas])
        self.lg = {lt: [loss_and_grad(orc, self.freqs, self.ref, lt, t) for t in self.thetas] for lt in losses}


@pytest.fixture(scope="module")
def ortho():
    return _Case("orthotropic", 4, 5, 70, LOSSES)                              # Fpad 128: 640 lanes


@pytest.fixture(scope="module")
def sol():
    return _Case("sol", 4, 3, 40, LOSSES[:1])                                  # B != 0: all 18 matrices


def test_forward_population_against_the_oracle(ortho):
    fr = ortho.p.solveForwardPopulation(ortho.freqs, ortho.thetas)
    assert fr.shape == ortho.fr.shape
    err = np.max(np.abs(fr - ortho.fr) / np.abs(ortho.fr), axis=1)
    print("fr per member:", err)
    report("population forward", fr_rel=list(err))
    assert ortho.p.engine().n_stiff == 12
    assert np.all(err < FR_RTOL), err
    assert np.all(ortho.p.engine().last_flags == 0)


def _check(c, lt, name):
    losses, grads = c.p.getPopulationLossFunction(c.freqs, c.ref, lt, with_grad=True)(c.thetas)
    only = c.p.getPopulationLossFunction(c.freqs, c.ref, lt)(c.thetas)
    P = c.thetas.shape[0]
    assert losses.shape == only.shape == (P,) and grads.shape == c.thetas.shape
    seq = c.p.getLossFunction(c.freqs, c.ref, lt)
    el, eg, sl, sg, fl = [], [], [], [], []
    for i in range(P):
        lo, go = c.lg[lt][i]
        el.append(abs(losses[i] - lo) / abs(lo))
        fl.append(abs(only[i] - lo) / abs(lo))
        eg.append(_rel(grads[i], go))
        x = torch.tensor(c.thetas[i], requires_grad=True)
        val = seq(x)
        val.backward()
        sl.append(abs(losses[i] - val.item()) / abs(val.item()))
        sg.append(_rel(grads[i], x.grad.numpy()))
    print(f"{name} {lt}: loss {max(el):.2e} (forward-only {max(fl):.2e}), gradient {max(eg):.2e}; against the "
          f"sequential calls loss {max(sl):.2e}, gradient {max(sg):.2e}")
    report(f"population {name} {lt}", loss_rel=el, loss_fwd_rel=fl, grad_rel=eg, seq_loss_rel=sl, seq_grad_rel=sg)
    assert max(el) < FR_RTOL and max(fl) < FR_RTOL, (el, fl)
    assert max(eg) < GRAD_RTOL, eg
    assert max(sl) < 2 * FR_RTOL, sl
    assert max(sg) < 2 * GRAD_RTOL, sg


@pytest.mark.parametrize("lt", LOSSES)
def test_loss_and_gradient(ortho, lt):
    _check(ortho, lt, "orthotropic")


def test_coupled_laminate(sol):
    """'sol' with angles (0, 90): B != 0, so the sweep contracts all 18 matrices."""
    fr = sol.p.solveForwardPopulation(sol.freqs, sol.thetas)
    err = np.max(np.abs(fr - sol.fr) / np.abs(sol.fr), axis=1)
    assert sol.p.engine().n_stiff == 18
    assert np.all(err < FR_RTOL), err
    _check(sol, "MSE_LOG_AFC", "sol")


def test_vectorized_differential_evolution(ortho):
    """Two generations of a 15-member population (popsize 3 x 5 parameters), 70 frequencies.  The returned loss is
    that member's value in a 15-member sweep; re-evaluated alone it runs on other launch forms, and both are within
    FR_RTOL of the exact loss, hence 2 FR_RTOL.  The truth lies at a corner of the bounds, 8 % from their centre in
    every parameter."""
    p = ortho.p
    t0 = p.parameters
    truth = t0 * (1 + 0.08 * np.array([1, -1, 1, -1, 1]))
    ref = p.solveForward(ortho.freqs, truth)
    bounds = np.stack([0.9 * t0, 1.1 * t0], axis=1)
    res = p.solveInverse(bounds, 'MSE_LOG_AFC', 'de', ref_fr=[ortho.freqs, ref], vectorized=True, seed=5, maxiter=2,
                         popsize=3, polish=False, tol=0.0, log=False, report=False)
    pop_loss = p.getPopulationLossFunction(ortho.freqs, ref, 'MSE_LOG_AFC')
    again = pop_loss(np.asarray(res.x)[None, :])[0]
    centre = pop_loss(t0[None, :])[0]
    print(f"de: fun {res.fun:.6e}, re-evaluated {again:.6e}, centre {centre:.6e}, nfev {res.nfev}")
    report("population de", fun=res.fun, again=again, centre=centre)
    assert np.all(res.x >= bounds[:, 0]) and np.all(res.x <= bounds[:, 1])
    assert abs(res.fun - again) <= 2 * FR_RTOL * abs(again)
    assert res.fun <= centre
    with pytest.raises(NotImplementedError):
        p.getPopulationLossFunction(ortho.freqs, ref, 'MSE_LOG_AFC', distributed=True)
