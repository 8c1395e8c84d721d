"""CPU: the per-frequency Jacobian sweep's interface, its reference rows, the least-squares algebra of the four
losses, the Levenberg-Marquardt optimiser and the covariance formula (no GPU)."""
import warnings

import numpy as np
import pytest

import synthetic as sy
import synthetic_jacobian as sj
from oracle.plate_oracle import loss_term_derivative, loss_terms
from plate_inverse_problem_amd import Optimizers as opt
from plate_inverse_problem_amd import _native
from plate_inverse_problem_amd.Problem import covariance_from_residual, residual_terms

LOSSES = ("MSE", "RMSE", "MSE_AFC", "MSE_LOG_AFC")


# ----------------------------------------------------------------------------- the C ABI
def test_entry_point_is_declared_bound_and_exported():
    assert "pfr_jacobian_sweep" in _native.header_symbols()
    assert "pfr_jacobian_sweep" in _native._PROTOS
    assert hasattr(_native.lib(), "pfr_jacobian_sweep")
    assert set(_native.header_symbols()) == set(_native._PROTOS)


def test_null_solver_is_an_argument_error():
    L = _native.lib()
    assert L.pfr_jacobian_sweep(None, 4, None, None, None, None, None) == 1          # PFR_ERR_ARG
    assert b"jacobian" in L.pfr_last_error()


# ----------------------------------------------------------------------------- the reference rows
FD = [("A", 12), ("F0", 12), ("T", 18)]


@pytest.mark.parametrize("shape,n_stiff", FD)
def test_jacobian_reference_matches_finite_differences(shape, n_stiff):
    """Re sum_k row_k d_k against central differences (t = 1e-7, extended precision) of fr along three complex
    coefficient directions d, 4 frequencies; the bound 1e-9 of test_hessian_reference_matches_finite_differences for
    the same construction (it covers the O(t^2) truncation).  And the rows are w / cot of the COTANGENT reference."""
    _, op = sy.case(shape, n_stiff=n_stiff)
    freqs = np.linspace(40.0, 600.0, 4)
    refc = sy.reference(op, freqs)
    rows = sj.jacobian_reference(refc)
    d = sy.direction(3, n_stiff).astype(sy.CLD)
    t = sy.LD(1e-7)
    coef = op.coef.astype(sy.CLD)
    J = (rows @ d.T).real                                                     # (4, 3)
    Jfd = np.stack([(sj.fr_at(op, freqs, coef + t * d[i]) - sj.fr_at(op, freqs, coef - t * d[i])) / (2 * t)
                    for i in range(3)], axis=1)
    err = float(np.max(np.abs(J - Jfd)) / np.max(np.abs(J)))
    wc = refc.loss("COTANGENT")["w"] / refc.cot.astype(sy.LD)[:, None]
    same = sj.row_errors(rows, wc)
    print(f"{shape} n_stiff={n_stiff}: |J - J_fd| / max|J| = {err:.1e}; rows against w / cot {same:.1e}")
    assert err <= 1e-9
    assert same <= 1e-16


def test_model_rows_sit_at_rounding_level():
    """jacobian_model_errors on A, both analyses, raw and corrected: the fp64 sequences agree with the reference to
    rounding (the bounds of the GPU tests are 10 x these)."""
    _, op = sy.case("A")
    freqs = sy.FREQS[sy.three(sy.FREQS)]
    for symmetric in (True, False):
        for correct in (False, True):
            em, ed = sj.jacobian_model_errors(op, sy.symbolic("A", symmetric=symmetric), freqs, symmetric=symmetric,
                                              correct=correct)
            print(f"A symmetric={symmetric} correct={correct}: e_model {em} e_dense {ed}")
            assert max(em["jc"], ed["jc"], em["fr"], ed["fr"]) < 1e-11


# ----------------------------------------------------------------------------- least-squares form of the losses
@pytest.mark.parametrize("loss_type", LOSSES)
def test_residual_algebra(loss_type):
    rng = np.random.default_rng(11)
    fr = 0.1 + rng.random(37)
    ref = fr * (1 + 0.1 * rng.standard_normal(37)) * np.exp(0.3j * rng.standard_normal(37))
    r, drdfr, const = residual_terms(fr, ref, loss_type)
    assert r.shape == drdfr.shape == (37,)
    np.testing.assert_allclose((r @ r + const) / 37, np.mean(loss_terms(fr, ref, loss_type)), rtol=1e-14)
    np.testing.assert_allclose(2 * r * drdfr, loss_term_derivative(fr, ref, loss_type), rtol=1e-13, atol=1e-300)
    if loss_type in ("MSE_AFC", "MSE_LOG_AFC"):
        assert const == 0.0


def test_residual_terms_rejects_unknown_loss():
    with pytest.raises(ValueError):
        residual_terms(np.ones(3), np.ones(3), "HUBER")


# ----------------------------------------------------------------------------- optimize_lm
def _res(fun, jac, const=0.0):
    calls = []

    def res(x):
        calls.append(np.array(x, dtype=np.float64))
        return fun(x), jac(x), const
    res.calls = calls
    return res


def test_lm_linear_least_squares_in_one_accepted_step():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((20, 4))
    b = rng.standard_normal(20)
    xs = np.linalg.lstsq(A, b, rcond=None)[0]
    res = _res(lambda x: A @ x - b, lambda x: A)
    out = opt.optimize_lm(res, np.zeros(4), N_steps=2, lam0=1e-12)
    np.testing.assert_array_equal(res.calls[1], out.x_history[1])            # the first trial step was accepted ...
    np.testing.assert_allclose(out.x_history[1], xs, rtol=1e-9)               # ... and is the minimiser
    np.testing.assert_allclose(out.x, xs, rtol=1e-9)
    fmin = float(np.sum((A @ xs - b) ** 2)) / 20
    assert abs(out.f - fmin) <= 1e-12 * fmin and out.f < out.f_history[0]


def test_lm_rosenbrock():
    res = _res(lambda x: np.array([10.0 * (x[1] - x[0] ** 2), 1.0 - x[0]]),
               lambda x: np.array([[-20.0 * x[0], 10.0], [-1.0, 0.0]]))
    out = opt.optimize_lm(res, np.array([-1.2, 1.0]), N_steps=100)
    np.testing.assert_allclose(out.x, [1.0, 1.0], atol=1e-7)
    assert out.status.startswith("Converged") and out.f <= 1e-16
    assert all(a > b for a, b in zip(out.f_history, out.f_history[1:]))       # accepted iterates only
    assert len(out.f_history) == len(out.x_history) == len(out.grad_history)


def test_lm_exponential_fit():
    t = np.linspace(0.0, 2.0, 25)
    truth = np.array([2.0, -1.3])
    y = truth[0] * np.exp(truth[1] * t)
    res = _res(lambda x: x[0] * np.exp(x[1] * t) - y,
               lambda x: np.stack([np.exp(x[1] * t), x[0] * t * np.exp(x[1] * t)], axis=1))
    out = opt.optimize_lm(res, np.array([1.0, 0.0]), N_steps=60)
    np.testing.assert_allclose(out.x, truth, rtol=1e-7)
    assert out.f < 1e-14 * out.f_history[0]


def test_lm_const_is_part_of_the_loss():
    res = _res(lambda x: x - 1.0, lambda x: np.eye(2), const=6.0)
    out = opt.optimize_lm(res, np.zeros(2), N_steps=5, f_min=0.0)
    assert out.f_history[0] == (2.0 + 6.0) / 2 and abs(out.f - 3.0) < 1e-12


def test_lm_rejected_step_keeps_x_and_raises_lam():
    """A residual whose every trial point is worse than the start: x never moves, and each rejected trial is a
    shorter step of the same model (lam raised, no evaluation at x again) until the damping limit."""
    x0 = np.array([0.5, -0.25])

    def fun(x):
        return np.array([1.0, 1.0]) + 10.0 * np.linalg.norm(np.asarray(x) - x0)      # minimal AT x0, model says move
    res = _res(fun, lambda x: np.eye(2))
    out = opt.optimize_lm(res, x0, N_steps=5, lam0=1e-3, lam_up=4.0, lam_max=1e3)
    assert np.array_equal(out.x, x0) and out.status == "Damping limit reached"
    assert out.f_history == [1.0] and len(out.x_history) == 1
    steps = [np.linalg.norm(c - x0) for c in res.calls[1:]]
    assert len(steps) == 10                                                  # lam 1e-3 * 4^j <= 1e3: j = 0 .. 9
    assert all(b < a for a, b in zip(steps, steps[1:]))
    np.testing.assert_allclose(steps[0] / steps[1], (1 + 4e-3) / (1 + 1e-3), rtol=1e-12)
    assert not any(np.array_equal(c, x0) for c in res.calls[1:])


def test_lm_step_is_marquardt_scaled():
    """The step is invariant under a rescaling of the parameters (diag(J^T J) damping, not the identity)."""
    rng = np.random.default_rng(5)
    J = rng.standard_normal((12, 3))
    r = rng.standard_normal(12)
    s = np.array([1.0, 1e6, 1e-4])
    np.testing.assert_allclose(opt.lm_step(J * s, r, 0.1) * s, opt.lm_step(J, r, 0.1), rtol=1e-9)


# ----------------------------------------------------------------------------- covariance
def test_covariance_algebra():
    rng = np.random.default_rng(7)
    Jr = rng.standard_normal((40, 3)) * np.array([1.0, 1e3, 1e-3])
    r = 0.01 * rng.standard_normal(40)
    cov, std = covariance_from_residual(r, Jr, const=0.5)
    want = (r @ r + 0.5) / (40 - 3) * np.linalg.inv(Jr.T @ Jr)
    np.testing.assert_allclose(cov, want, rtol=1e-9)
    np.testing.assert_allclose(std, np.sqrt(np.diag(want)), rtol=1e-9)
    assert np.array_equal(cov, cov.T)


def test_covariance_warns_when_singular():
    rng = np.random.default_rng(8)
    J2 = rng.standard_normal((30, 2))
    Jr = np.column_stack([J2, J2[:, 0] + J2[:, 1]])              # rank 2
    with pytest.warns(RuntimeWarning, match="singular"):
        cov, std = covariance_from_residual(rng.standard_normal(30), Jr)
    assert np.all(np.isfinite(cov)) and np.linalg.matrix_rank(cov, tol=1e-9 * np.abs(cov).max()) == 2
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        covariance_from_residual(rng.standard_normal(30), J2)
    with pytest.raises(ValueError):
        covariance_from_residual(np.zeros(2), np.zeros((2, 3)))


def test_lm_names_reach_solve_inverse():
    from plate_inverse_problem_amd import inverse
    assert any("lm" in names and "levenberg_marquardt" in names and fn is opt.optimize_lm
               for names, fn in inverse._LOCAL.items())
