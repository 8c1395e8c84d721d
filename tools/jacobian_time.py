"""Time of a per-frequency Jacobian sweep against the loss + gradient step of the same build, in one process,
alternating (C3: ny = 25, 19,353 DOF, one chunk of 2,048 frequencies by default; check mode 11).  Each sample is a
host clock around a call that ends in a device synchronise.  Then, with the checks off (mode 0) and with the raw
checks (mode 3), the Jacobian sweep's contraction phase from the solver's HIP events: without the correction's walk
it is k_contract_q + k_rhs_dot + k_jac_finish (plus, in mode 3, the two backward-error walks).

    python tools/jacobian_time.py [--nfreq 2048] [--reps 12] [--out FILE.json]
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
        raise SystemExit("jacobian_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    p = bench.build_problem(a.ny, dev, max_batch=a.nfreq)
    th0 = p.parameters.copy()
    freqs = np.linspace(40.0, 600.0, a.nfreq)
    ref = p.solveForward(freqs, th0)
    theta = th0 * (1 + np.array([0.1, 0.1, 0.2, 0.1, 0.1]))
    loss_fn = p.getLossFunction(freqs, ref, "MSE_LOG_AFC")
    jac_fn = p.getFRJacobianFunction()
    f_dev = p._freqs(freqs)

    def loss_step():
        x = torch.tensor(theta, requires_grad=True)
        loss_fn(x).backward()
        torch.cuda.synchronize()

    def jac_step():
        fr, J = jac_fn(f_dev, theta)
        torch.cuda.synchronize()
        return fr, J

    for _ in range(2):                       # every shape of the timed window warmed up
        loss_step()
        jac_step()
    tl, tj = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        loss_step()
        t1 = time.perf_counter()
        jac_step()
        t2 = time.perf_counter()
        tl.append(t1 - t0)
        tj.append(t2 - t1)
    eng = p.engine()
    out = {"ny": a.ny, "dof": int(p.mat_size), "nfreq": a.nfreq, "lanes": eng.n_lanes, "max_batch": eng.max_batch,
           "check_mode": eng.check_mode, "reps": a.reps,
           "loss_step_ms": {"median": 1e3 * float(np.median(tl)), "min": 1e3 * min(tl), "max": 1e3 * max(tl)},
           "jacobian_ms": {"median": 1e3 * float(np.median(tj)), "min": 1e3 * min(tj), "max": 1e3 * max(tj)},
           "ratio_median": float(np.median(tj) / np.median(tl))}
    # the phases of the two sweeps in the default mode, then the Jacobian sweep without the correction's walk
    mode0 = eng.check_mode
    eng.set_timing(True)
    try:
        loss_step()
        out["loss_phases_ms"] = [float(v) for v in eng.last_timings()]
        jac_step()
        out["jacobian_phases_ms"] = [float(v) for v in eng.last_timings()]
        for mode in (0, 3):
            eng.set_check(mode)
            jac_step()
            jac_step()
            out[f"jacobian_phases_ms_mode{mode}"] = [float(v) for v in eng.last_timings()]
    finally:
        eng.set_check(mode0)
        eng.set_timing(False)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
