"""Time of the complex response's sweeps against the magnitude's of the same build, in one process, alternating (C3:
ny = 25, 19,353 DOF, one lane, one chunk of 2,048 frequencies by default; check mode 11): the complex loss + gradient
step (MSE_LOG_COMPLEX) against the magnitude loss step (MSE_LOG_AFC), and pfr_jacobian_sweep_complex against
pfr_jacobian_sweep.  Each sample is a host clock around a call that ends in a device synchronise.  The complex forms
run the same passes with other functional kernels, so ratios near 1 are expected.

    python tools/complex_time.py [--nfreq 2048] [--reps 12] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _stats(t):
    return {"median": 1e3 * float(np.median(t)), "min": 1e3 * min(t), "max": 1e3 * max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, default=25)
    ap.add_argument("--nfreq", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--lanes", type=int, default=1, help="solver lanes (1: the whole sweep is one chunk)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["PFR_LANES"] = str(a.lanes)          # read when the engine is built
    if not torch.cuda.is_available():
        raise SystemExit("complex_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    p = bench.build_problem(a.ny, dev, max_batch=a.nfreq)
    th0 = p.parameters.copy()
    freqs = np.linspace(40.0, 600.0, a.nfreq)
    axis = (0.0, 0.0, 1.0)
    ref = p.solveForward(freqs, th0)
    ref_c = p.solveForwardComplex(freqs, th0, axis)
    theta = th0 * (1 + np.array([0.1, 0.1, 0.2, 0.1, 0.1]))
    steps = {
        "loss_step": p.getLossFunction(freqs, ref, "MSE_LOG_AFC"),
        "complex_loss_step": p.getLossFunction(freqs, ref_c, "MSE_LOG_COMPLEX", axis=axis),
    }
    jacs = {"jacobian": p.getFRJacobianFunction(), "complex_jacobian": p.getTFJacobianFunction(axis=axis)}
    f_dev = p._freqs(freqs)

    def run(name):
        if name in steps:
            x = torch.tensor(theta, requires_grad=True)
            steps[name](x).backward()
        else:
            jacs[name](f_dev, theta)
        torch.cuda.synchronize()

    order = ("loss_step", "complex_loss_step", "jacobian", "complex_jacobian")
    for _ in range(2):                       # every shape of the timed window warmed up
        for name in order:
            run(name)
    t = {name: [] for name in order}
    for _ in range(a.reps):
        for name in order:
            t0 = time.perf_counter()
            run(name)
            t[name].append(time.perf_counter() - t0)
    eng = p.engine()
    out = {"ny": a.ny, "dof": int(p.mat_size), "nfreq": a.nfreq, "lanes": eng.n_lanes, "max_batch": eng.max_batch,
           "check_mode": eng.check_mode, "reps": a.reps, "axis": list(axis)}
    for name in order:
        out[name + "_ms"] = _stats(t[name])
    out["loss_ratio_median"] = float(np.median(t["complex_loss_step"]) / np.median(t["loss_step"]))
    out["jacobian_ratio_median"] = float(np.median(t["complex_jacobian"]) / np.median(t["jacobian"]))
    eng.set_timing(True)
    try:
        for name in order:
            run(name)
            out[name + "_phases_ms"] = [float(v) for v in eng.last_timings()]
    finally:
        eng.set_timing(False)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
