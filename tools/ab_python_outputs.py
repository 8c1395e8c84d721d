"""What every Python sweep path of ``Problem`` returns, and ``last_berr`` / ``last_flags`` after each call, at ny=4 ->
an .npz (A/B of two trees' host Python on the same library for bit-for-bit equality: run once per tree with PFR_LIB
naming one libpfr.so, then compare with --compare A.npz B.npz).  Three sweep widths: 512 frequencies (two lanes), 100
(one lane, a ragged last group) and 200 under PFR_LANE_FREQS=64 (three lanes asked for, two with ragged blocks).  Four
problems: orthotropic (mid-plane symmetric: 12 contracted matrices, ``expand``), sol (18), isotropic, and the
isotropic material under a type name the jet transform does not know -- every material type of Material.py takes the
jet branch of ``_coeffs`` / ``_coeffs_jacobian``, so the autograd branch needs such a stand-in.

Usage: python tools/ab_python_outputs.py OUT.npz | --compare A.npz B.npz
"""
import os
import sys
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AXIS = (0.3, 0.2, 1.0)
CASES = ((512, None), (100, None), (200, "64"))         # (frequencies, PFR_LANE_FREQS)


def problems():
    from plate_inverse_problem_amd.Material import Isotropic
    from plate_inverse_problem_amd.Problem import Problem
    from tests.helpers import MATERIALS, make_geometry, make_problem

    class AutogradIsotropic(Isotropic):
        atype = "isotropic_autograd"                     # not one of Problem._JET_TYPES

    def autograd_isotropic():
        geom, acc = make_geometry(4)
        rho, kw = MATERIALS["isotropic"]
        return Problem(geom, AutogradIsotropic(rho, **kw), acc, device="cuda:0")
    for name in ("orthotropic", "sol", "isotropic"):
        yield name, lambda name=name: make_problem(name, ny=4, device="cuda:0")
    yield "isotropic_autograd", autograd_isotropic


def run_case(res, tag, p, n):
    import torch
    from plate_inverse_problem_amd import _native
    from plate_inverse_problem_amd.Problem import _SweepLoss

    def put(key, *arrays):
        """The call's outputs, then the engine's last_berr / last_flags and the RuntimeWarnings the call raised."""
        for i, a in enumerate(arrays):
            res[f"{tag}.{key}.{i}"] = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        eng = p.engine()
        b, fl = eng.last_berr, eng.last_flags
        res[f"{tag}.{key}.last_berr"] = np.zeros(0) if b is None else b.detach().cpu().numpy()
        res[f"{tag}.{key}.last_flags"] = np.full(1, -1, np.int32) if fl is None else np.asarray(fl)
        res[f"{tag}.{key}.warnings"] = np.array(sum(issubclass(w.category, RuntimeWarning) for w in caught))
        caught.clear()

    freqs = np.linspace(40.0, 600.0, n)
    th0 = np.asarray(p.parameters, dtype=np.float64)
    scal = th0.copy()                                    # the functions below are of params * scal
    unit = 1.0 + 0.03 * np.cos(np.arange(th0.size))
    theta = th0 * unit
    wts = torch.as_tensor(np.cos(0.1 * np.arange(n)), device="cuda:0")
    cwts = torch.as_tensor(np.exp(0.07j * np.arange(n)), device="cuda:0")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        # the response functions and their backward sweeps
        fr0 = p.solveForward(freqs)
        h0 = p.solveForwardComplex(freqs, axis=AXIS)
        put("solveForward", fr0, h0)
        ref, cref = fr0 * 1.01, h0 * (1.01 + 0.01j)
        x = torch.tensor(theta, requires_grad=True)
        fr = p.getFRFunction()(freqs, x)
        put("fr", fr)
        (fr * wts).sum().backward()
        put("fr_backward", x.grad)
        x = torch.tensor(theta, requires_grad=True)
        h = p.getTFFunction(AXIS)(freqs, x)
        put("tf", h)
        torch.real(h * cwts).sum().backward()
        put("tf_backward", x.grad)
        # the losses: the single-process step, and the all-reduce path with an identity reduction
        for name, r, axis in (("MSE_LOG_AFC", ref, None), ("MSE_LOG_COMPLEX", cref, AXIS)):
            fn = p.getLossFunction(freqs, r, name, scaling_params=scal, axis=axis)
            for step in range(2):                        # the second step on the cached buffers and views
                x = torch.tensor(unit, requires_grad=True)
                v = fn(x)
                v.backward()
                put(f"loss_{name}_{step}", v, x.grad)
            x = torch.tensor(theta, requires_grad=True)
            c = p._coeffs(p._transform(), x)
            ids = {**_native.LOSS_IDS, **_native.COMPLEX_LOSS_IDS}
            v = _SweepLoss.apply(c, p.engine(n), p._freqs(freqs),
                                 torch.as_tensor(np.asarray(r).astype(np.complex128), device=p.device), ids[name], n,
                                 lambda t: t, None if axis is None else np.asarray(axis, dtype=np.float64))
            v.backward()
            put(f"loss_reduce_{name}", v, x.grad)
        put("hessian", *p.getLossHessianFunction(freqs, ref, "MSE_LOG_AFC", scaling_params=scal)(unit))
        # the Jacobian sweeps and the least-squares forms on them
        put("fr_jacobian", *p.getFRJacobianFunction(scal)(freqs, unit))
        put("tf_jacobian", *p.getTFJacobianFunction(scal, AXIS)(freqs, unit))
        put("residual", *p.getResidualFunction(freqs, ref, "MSE_LOG_AFC", scal)(unit))
        put("residual_complex", *p.getResidualFunction(freqs, cref, "RMSE_COMPLEX", scal, AXIS)(unit))
        # checked forward sweeps (before the population re-sizes the engine)
        put("checked_refine", *p.solveForwardChecked(freqs, theta, refine=True))
        put("checked_uncorrected", *p.solveForwardChecked(freqs, theta, correct=False))
        # a population of 3
        pop = np.stack([unit, unit * 1.02, unit * 0.97])
        put("population_forward", p.solveForwardPopulation(freqs, pop * scal))
        put("population_loss", *p.getPopulationLossFunction(freqs, ref, "MSE_LOG_AFC", scal, with_grad=True)(pop))
        put("lanes", np.array(p.engine().n_lanes))


def run(out):
    import torch
    res = {}
    for n, lane_freqs in CASES:
        os.environ.pop("PFR_LANE_FREQS", None)
        if lane_freqs is not None:
            os.environ["PFR_LANE_FREQS"] = lane_freqs        # read when the engine is made
        for name, make in problems():
            p = make()
            run_case(res, f"{name}.{n}", p, n)
            p._engine = None
            del p
            torch.cuda.empty_cache()
    np.savez(out, **res)
    print("saved", out, len(res), "arrays;", os.environ.get("PFR_LIB", "default library"))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    same = sorted(A.files) == sorted(B.files)
    if not same:
        print("DIFFERENT KEYS:", sorted(set(A.files) ^ set(B.files)))
    n_eq = 0
    for k in A.files:
        if k not in B.files:
            continue
        x, y = A[k], B[k]
        eq = x.dtype == y.dtype and x.shape == y.shape and \
            np.array_equal(x, y, equal_nan=x.dtype.kind in "fc")        # NaN (a backward error not checked) = NaN
        n_eq += eq
        if not eq or k.endswith((".0", ".lanes.0")) and ".512." in k:
            print(f"{k:64s} {str(x.dtype):10s} {str(x.shape):14s} bitwise {'equal' if eq else 'DIFFERENT'}")
        same &= bool(eq)
    print(f"{n_eq} of {len(A.files)} arrays bitwise equal (the rows above: the 512-frequency runs' first outputs and "
          "every difference)")
    print("ALL EQUAL" if same else "DIFFERENCES")
    return 0 if same else 1


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run(sys.argv[1])
