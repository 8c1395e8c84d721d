"""CPU: the population sweep's interface, its lane layout, the host step from (fr, jc, dc, ref) to (loss, grad) and
the vectorised differential-evolution path of solve_inverse (no GPU)."""
import numpy as np
import pytest
import torch

import synthetic as sy
import synthetic_jacobian as sj
import synthetic_population as sp
from oracle.plate_oracle import loss_term_derivative, loss_terms
from plate_inverse_problem_amd import _native, inverse
from plate_inverse_problem_amd.Problem import Problem, _Engine, population_layout, population_loss_grad, residual_terms

LOSSES = ("MSE", "RMSE", "MSE_AFC", "MSE_LOG_AFC")


# ----------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_bound_and_exported():
    for name in ("pfr_combine_batch", "pfr_population_sweep"):
        assert name in _native.header_symbols()
        assert name in _native._PROTOS
        assert hasattr(_native.lib(), name)
    assert set(_native.header_symbols()) == set(_native._PROTOS)
    for name in ("combine_batch", "population_sweep"):
        assert callable(getattr(_native.Solver, name))
    assert callable(_Engine.population_sweep)
    for name in ("solveForwardPopulation", "getPopulationLossFunction"):
        assert callable(getattr(Problem, name))


def test_null_solver_is_an_argument_error():
    L = _native.lib()
    assert L.pfr_population_sweep(None, 64, None, None, 1, None, None, None, None, None, None) == 1   # PFR_ERR_ARG
    assert b"population" in L.pfr_last_error()
    assert L.pfr_combine_batch(None, 1, None, None, None) == 1
    assert b"combine batch" in L.pfr_last_error()


# ----------------------------------------------------------------------------- lane layout
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("F", [1, 63, 64, 65, 130])
def test_lane_layout(F, P):
    index, member, valid = population_layout(P, F)
    fpad = -(-F // 64) * 64
    assert index.shape == valid.shape == (P * fpad,) and member.shape == (P * fpad // 64,)
    assert member.dtype == np.int32 and valid.dtype == bool
    assert (P * fpad) % 64 == 0
    for p in range(P):
        blk = slice(p * fpad, (p + 1) * fpad)
        assert np.array_equal(index[blk][:F], np.arange(F))                  # the member's frequencies, in order
        assert np.all(index[blk][F:] == F - 1)                               # padded lanes repeat the last one
        assert valid[blk][:F].all() and not valid[blk][F:].any()
        assert np.all(member[p * fpad // 64:(p + 1) * fpad // 64] == p)      # every 64-lane group has one member
    assert valid.sum() == P * F


def test_lane_layout_rejects_empty():
    with pytest.raises(ValueError):
        population_layout(0, 4)
    with pytest.raises(ValueError):
        population_layout(2, 0)


def test_synthetic_members_are_exact_and_well_conditioned():
    """The members of the GPU tests (asserted inside sp.members: coef @ S and e @ coef exact in fp64, cond_2 <=
    COND_MAX of every member's matrices), for every shape the GPU tests and the issue's table use."""
    for shape in ("A", "B", "D", "T", "F0"):
        base, ops = sp.members(shape, 3)
        conds = [sy.check_cond([m.matrix_ld(f) for f in sy.FREQS[::sp.COND_EVERY]], shape).max() for m in ops]
        print(shape, "cond <=", max(conds))
        assert len(ops) == 3 and max(conds) <= sy.COND_MAX
        assert all(not np.array_equal(m.coef, base.coef) for m in ops)
        assert len({m.coef.tobytes() for m in ops}) == 3


# ----------------------------------------------------------------------------- (fr, jc, dc, ref) -> (loss, grad)
@pytest.mark.parametrize("loss_type", LOSSES)
def test_loss_and_gradient_against_the_oracle_terms(loss_type):
    rng = np.random.default_rng(21)
    P, F, K, n = 3, 37, 12, 4
    fr = 0.1 + rng.random((P, F))
    ref = fr[0] * (1 + 0.1 * rng.standard_normal(F)) * np.exp(0.3j * rng.standard_normal(F))
    jc = rng.standard_normal((P, F, K)) + 1j * rng.standard_normal((P, F, K))
    dc = rng.standard_normal((P, K, n)) + 1j * rng.standard_normal((P, K, n))
    loss, grad = population_loss_grad(fr, jc, dc, ref, loss_type)
    assert loss.shape == (P,) and grad.shape == (P, n)
    for p in range(P):
        np.testing.assert_allclose(loss[p], np.mean(loss_terms(fr[p], ref, loss_type)), rtol=1e-14)
        J = np.real(jc[p] @ dc[p])
        want = loss_term_derivative(fr[p], ref, loss_type) @ J / F
        np.testing.assert_allclose(grad[p], want, rtol=1e-12, atol=1e-14 * np.abs(want).max())
    only, none = population_loss_grad(fr, None, None, ref, loss_type)
    assert none is None and np.array_equal(only, loss)


@pytest.mark.parametrize("loss_type", LOSSES)
def test_gradient_against_finite_differences_on_synthetic_rows(loss_type):
    """Two members (the base operator of shape A and one scaled copy), 4 frequencies, 3 parameters moving the
    coefficients along fixed complex directions d: the gradient from the reference rows against central
    differences (t = 1e-7, extended precision) of the loss of fr.  The rows themselves match such differences to 1e-9
    of max|J| (test_jacobian_cpu.py); the gradient is a sum of F = 4 of them weighted by 2 r dr/dfr / F, so the
    bound is 1e-9 of (2 / F) sum_q |r_q dr_q/dfr| max|J| -- no cancellation is credited."""
    base, ops = sp.members("A", 1)
    freqs = np.linspace(40.0, 600.0, 4)
    d = sy.direction(3, 12).astype(sy.CLD)
    t = sy.LD(1e-7)
    members = [base, ops[0]]
    refs = [sy.reference(m, freqs) for m in members]
    ref = refs[0].ref
    fr = np.stack([r.fr.astype(np.float64) for r in refs])
    jc = np.stack([sj.jacobian_reference(r).astype(np.complex128) for r in refs])
    dc = np.stack([d.T.astype(np.complex128)] * 2)
    loss, grad = population_loss_grad(fr, jc, dc, ref, loss_type)

    def loss_at(m, coef):
        r, _, const = residual_terms(sj.fr_at(m, freqs, coef).astype(np.float64), ref, loss_type)
        return (sy.LD(0) + np.sum(r.astype(sy.LD) ** 2) + const) / 4

    for p, m in enumerate(members):
        c = m.coef.astype(sy.CLD)
        # the loss in extended precision along each direction (fr_at's fr rounded to fp64 would lose 1e-16 / 1e-7)
        def ld_loss(coef):
            f_ld = sj.fr_at(m, freqs, coef)
            if loss_type == "MSE":
                r = f_ld - ref.real
            elif loss_type == "RMSE":
                r = (f_ld - ref.real) / np.abs(ref)
            elif loss_type == "MSE_AFC":
                r = f_ld - np.abs(ref)
            else:
                r = np.log(f_ld) - np.log(np.abs(ref).astype(sy.LD))
            return np.sum(r * r) / 4
        fd = np.array([float((ld_loss(c + t * d[i]) - ld_loss(c - t * d[i])) / (2 * t)) for i in range(3)])
        r, drdfr, _ = residual_terms(fr[p], ref, loss_type)
        scale = 2.0 / 4 * np.sum(np.abs(r * drdfr)) * np.max(np.abs(np.real(jc[p] @ dc[p])))
        err = float(np.max(np.abs(grad[p] - fd)) / scale)
        print(f"{loss_type} member {p}: |grad - fd| / scale = {err:.1e}")
        assert err <= 1e-9
        np.testing.assert_allclose(loss[p], float(loss_at(m, c)), rtol=1e-13)


# ----------------------------------------------------------------------------- solve_inverse
class _StubProblem:
    """Counts which loss solve_inverse reaches: a quadratic bowl around (1, 2)."""
    parameters = np.array([1.0, 2.0])
    accelerometer = material = geometry = "stub"

    def __init__(self):
        self.scalar_calls, self.population_calls = 0, []

    def getLossFunction(self, f, fr, loss_type, scaling, distributed=False):
        def loss(x):
            self.scalar_calls += 1
            return torch.sum((x - torch.tensor([1.0, 2.0], dtype=torch.float64)) ** 2)
        return loss

    def getPopulationLossFunction(self, f, fr, loss_type, scaling_params=None, with_grad=False):
        assert not with_grad

        def fn(params):
            params = np.asarray(params)
            assert params.ndim == 2 and params.shape[1] == 2
            self.population_calls.append(params.shape[0])
            return np.sum((params - np.array([1.0, 2.0])) ** 2, axis=1)
        return fn


_DE = dict(ref_fr=(np.linspace(1.0, 2.0, 5), np.ones(5)), report=False, log=False, seed=3, maxiter=3, popsize=6,
           polish=False, tol=0.0)
_BOUNDS = np.array([[0.0, 3.0], [0.0, 4.0]])


def test_solve_inverse_reaches_the_vectorised_path_only_when_asked():
    plain = _StubProblem()
    r0 = inverse.solve_inverse(plain, _BOUNDS, "MSE", "de", **_DE)
    assert plain.scalar_calls > 0 and plain.population_calls == []
    vec = _StubProblem()
    r1 = inverse.solve_inverse(vec, _BOUNDS, "MSE", "de", vectorized=True, **_DE)
    assert vec.scalar_calls == 0
    assert len(vec.population_calls) == 1 + 3 and all(s == 12 for s in vec.population_calls)   # S = popsize x n_par
    assert np.isfinite(r0.f) and np.isfinite(r1.f) and r1.f <= 1.0
    off = _StubProblem()
    inverse.solve_inverse(off, _BOUNDS, "MSE", "de", vectorized=False, **_DE)
    assert off.scalar_calls > 0 and off.population_calls == []


def test_vectorised_differential_evolution_is_not_distributed():
    with pytest.raises(NotImplementedError):
        inverse.solve_inverse(_StubProblem(), _BOUNDS, "MSE", "de", vectorized=True, distributed=True, **_DE)
