"""CPU: the complex response sweeps' interface, the least-squares algebra of their three losses, the test
reference's own consistency (tests/synthetic_complex.py) and the conditions on the inputs of the GPU tests (no GPU)."""
import numpy as np
import pytest

import synthetic as sy
import synthetic_complex as sc
from plate_inverse_problem_amd import _native
from plate_inverse_problem_amd.Problem import complex_residual_terms


# ----------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_bound_and_exported():
    for name in ("pfr_sweep_complex", "pfr_jacobian_sweep_complex"):
        assert name in _native.header_symbols()
        assert name in _native._PROTOS
        assert hasattr(_native.lib(), name)
    assert (_native.LOSS_CMSE, _native.LOSS_CRMSE, _native.LOSS_CLOG, _native.LOSS_CCOTANGENT) == (16, 17, 18, 19)
    assert _native.COMPLEX_LOSS_IDS == {"MSE_COMPLEX": 16, "RMSE_COMPLEX": 17, "MSE_LOG_COMPLEX": 18}
    assert not set(_native.COMPLEX_LOSS_IDS) & set(_native.LOSS_IDS)
    with open(_native.HEADER_PATH) as f:
        txt = f.read()
    for name, val in (("CMSE", 16), ("CRMSE", 17), ("CLOG", 18), ("CCOTANGENT", 19)):
        assert f"#define PFR_LOSS_{name} {val}" in txt


def test_null_solver_is_an_argument_error():
    L = _native.lib()
    axis = (np.ctypeslib.ctypes.c_double * 3)(0.0, 0.0, 1.0)
    assert L.pfr_sweep_complex(None, 4, None, axis, -1, None, 1.0, None, None, None, None, 0, None) == 1
    assert L.pfr_jacobian_sweep_complex(None, 4, None, axis, None, None, None, None) == 1


# ----------------------------------------------------------------------------- least-squares form of the losses
def _sample():
    rng = np.random.default_rng(12)
    H = (0.1 + rng.random(37)) * np.exp(2j * np.pi * rng.random(37))
    ref = H * (1 + 0.1 * rng.standard_normal(37)) * np.exp(0.3j * rng.standard_normal(37))
    return H, ref


@pytest.mark.parametrize("loss_type", sc.LOSSES)
def test_complex_residual_algebra(loss_type):
    H, ref = _sample()
    r, dz, const = complex_residual_terms(H, ref, loss_type)
    assert r.shape == (74,) and dz.shape == (37,) and dz.dtype == np.complex128 and const == 0.0
    terms = np.array([sc.loss_c(h, q, loss_type)[0] for h, q in zip(H, ref)])
    np.testing.assert_allclose(r @ r / 37, np.mean(terms), rtol=1e-14)
    # z is holomorphic in H: the same derivative along 1 and along i, by central differences
    z = lambda h: (lambda v: v[:37] + 1j * v[37:])(complex_residual_terms(h, ref, loss_type)[0])    # noqa: E731
    t = 1e-6
    for step in (t, 1j * t):
        fd = (z(H + step) - z(H - step)) / (2 * step)
        np.testing.assert_allclose(dz, fd, rtol=1e-8)
    # and d term = Re(g dH) with g = 2 conj(z) dz/dH: the kernels' cotangent
    g = np.array([sc.loss_c(h, q, loss_type)[1] for h, q in zip(H, ref)])
    np.testing.assert_allclose(2 * np.conj(z(H)) * dz, g, rtol=1e-12)


def test_complex_residual_terms_rejects_unknown_loss():
    for name in ("HUBER", "MSE", "MSE_LOG_AFC"):
        with pytest.raises(ValueError):
            complex_residual_terms(np.ones(3) + 0j, np.ones(3) + 0j, name)


# ----------------------------------------------------------------------------- the reference checks itself
@pytest.mark.parametrize("axis", sc.AXES, ids=["z", "tilted"])
def test_reference_gradient_matches_finite_differences(axis):
    """Re sum_k w_qk d_k of each loss against central differences of the extended-precision loss terms along a fixed
    complex coefficient direction d, per frequency; step t = 1e-7, 4 frequencies and the bound 1e-9 of
    test_jacobian_cpu.test_jacobian_reference_matches_finite_differences for the same construction.  And the rows
    contract to the CCOTANGENT reference."""
    _, op = sy.case("T", n_stiff=12)
    freqs = np.linspace(40.0, 600.0, 4)
    cref = sc.reference(op, freqs, axis)
    d = sy.direction(1, 12)[0].astype(sy.CLD)
    t = sy.LD(1e-7)
    coef = op.coef.astype(sy.CLD)
    Hp, Hm = sc.h_at(op, freqs, coef + t * d, axis), sc.h_at(op, freqs, coef - t * d, axis)
    for lt in sc.LOSSES:
        L = cref.loss(lt)
        J = (L["w"] @ d).real                                                # (4,)
        tp = np.array([sc.loss_c(h, r, lt)[0] for h, r in zip(Hp, cref.ref)])
        tm = np.array([sc.loss_c(h, r, lt)[0] for h, r in zip(Hm, cref.ref)])
        Jfd = (tp - tm) / (2 * t)
        err = float(np.max(np.abs(J - Jfd)) / np.max(np.abs(J)))
        print(f"T axis={axis} {lt}: |J - J_fd| / max|J| = {err:.1e}")
        assert err <= 1e-9
    dH = cref.rows @ d
    dHfd = (Hp - Hm) / (2 * t)
    assert float(np.max(np.abs(dH - dHfd)) / np.max(np.abs(dH))) <= 1e-9     # complex: no real part taken
    wc = cref.loss("CCOTANGENT")["w"]
    assert sc.sj.row_errors(wc, cref.cot.astype(sy.CLD)[:, None] * cref.rows) <= 1e-16


def test_model_sits_at_rounding_level():
    """model_errors on A, raw and corrected: the fp64 sequences agree with the reference to rounding (the bounds of
    the GPU tests are 10 x these)."""
    _, op = sy.case("A")
    freqs = sy.FREQS[sy.three(sy.FREQS)]
    for correct in (False, True):
        out = sc.model_errors(op, sy.symbolic("A"), freqs, sc.AXES[1], correct=correct)
        for lt, (em, ed) in out.items():
            print(f"A correct={correct} {lt}: e_model {em} e_dense {ed}")
            assert max(*em.values(), *ed.values()) < 1e-11


# ----------------------------------------------------------------------------- conditions on the GPU tests' inputs
GPU_CASES = [("F0", {}), ("A", {}), ("T", {}), ("A4", {}), ("T", {"n_stiff": 18}), ("T", {"spread": True})]


@pytest.mark.parametrize("shape,kw", GPU_CASES, ids=[s + "".join(f"-{k}" for k in kw) for s, kw in GPU_CASES])
def test_gpu_inputs_are_well_conditioned(shape, kw):
    """Over sy.FREQS, both axes: H never falls below 1e-6 of its peak (its relative error stays meaningful and
    2 conj(z) / H bounded) and log(Href / ref) is far from the branch cut -- so a GPU failure cannot hide behind the
    inputs."""
    _, op = sy.case(shape, **kw)
    for axis in sc.AXES:
        cref = sc.reference(op, sy.FREQS, axis)
        a = np.abs(cref.H).astype(np.float64)
        print(f"{shape} {kw} axis={axis}: min|H| / max|H| = {a.min() / a.max():.2e}")
        assert a.min() >= 1e-6 * a.max()
        z = np.log((cref.H / cref.ref.astype(sy.CLD)).astype(np.complex128))
        assert np.max(np.abs(z.imag)) <= 1.0
