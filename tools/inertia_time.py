"""Time of an inertia sweep (pfr_inertia_sweep) against the Jacobian sweep (pfr_jacobian_sweep) of the same build, in
one process, alternating (C3: ny = 25, 19,353 DOF, one lane, one chunk of 2,048 frequencies by default; check mode
11).  Each sample is a host clock around a call that ends in a device synchronise.  Then the two new kernels'
time from the solver's HIP events: the contraction phase of the inertia sweep minus that of the Jacobian sweep, in
the default mode and with the checks off (mode 0) -- where the Jacobian sweep's contraction phase is the yardstick
k_contract_q + k_rhs_dot + k_jac_finish (no walk contracts anything without the correction), measured in the same run.

    python tools/inertia_time.py [--nfreq 2048] [--reps 12] [--out FILE.json]
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
        raise SystemExit("inertia_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    p = bench.build_problem(a.ny, dev, max_batch=a.nfreq)
    theta = p.parameters * (1 + np.array([0.1, 0.1, 0.2, 0.1, 0.1]))
    freqs = np.linspace(40.0, 600.0, a.nfreq)
    f_dev = p._freqs(freqs)
    eng = p.engine(a.nfreq)
    eng.set_coefficients(p._coeffs_jacobian(None)(theta)[0])
    fr, flags, berr, jc = eng.outputs(a.nfreq, jc=True)
    jm = torch.empty((a.nfreq, 4), dtype=torch.complex128, device=dev)

    def jac_step():
        eng.jacobian_sweep(f_dev, jc, fr=fr, flags=flags, berr=berr)
        torch.cuda.synchronize()

    def inertia_step(with_jc=True):
        eng.inertia_sweep(f_dev, jm, jc=jc if with_jc else None, fr=fr, flags=flags, berr=berr)
        torch.cuda.synchronize()

    for _ in range(2):                       # every shape of the timed window warmed up
        jac_step()
        inertia_step()
    jac_step()
    jc_ref, fr_ref = jc.clone(), fr.clone()
    inertia_step()
    same = bool(torch.equal(jc, jc_ref) and torch.equal(fr, fr_ref))
    tj, ti = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        jac_step()
        t1 = time.perf_counter()
        inertia_step()
        t2 = time.perf_counter()
        tj.append(t1 - t0)
        ti.append(t2 - t1)
    listed, padded = eng.solver.mass_list()
    out = {"ny": a.ny, "dof": int(p.mat_size), "nfreq": a.nfreq, "lanes": eng.n_lanes, "max_batch": eng.max_batch,
           "check_mode": eng.check_mode, "reps": a.reps, "n_stiff": eng.n_stiff, "nnz": int(eng.keep.size),
           "mass_entries_listed": listed, "mass_list_padded": padded, "jc_and_fr_bitwise_jacobian_sweep": same,
           "jacobian_ms": {"median": 1e3 * float(np.median(tj)), "min": 1e3 * min(tj), "max": 1e3 * max(tj)},
           "inertia_ms": {"median": 1e3 * float(np.median(ti)), "min": 1e3 * min(ti), "max": 1e3 * max(ti)},
           "ratio_median": float(np.median(ti) / np.median(tj))}
    # the contraction phase (HIP events around phase_finish) of both sweeps: their difference is k_contract_mass +
    # k_inertia_finish; in mode 0 the Jacobian sweep's is k_contract_q + k_rhs_dot + k_jac_finish, the yardstick
    mode0 = eng.check_mode
    eng.set_timing(True)
    try:
        for mode in (mode0, 0):
            eng.set_check(mode)
            pj, pi = [], []
            for _ in range(max(3, a.reps // 2)):
                jac_step()
                pj.append(eng.last_timings()[4])
                inertia_step()
                pi.append(eng.last_timings()[4])
            out[f"mode{mode}"] = {"jacobian_contraction_phase_ms": float(np.median(pj)),
                                  "inertia_contraction_phase_ms": float(np.median(pi)),
                                  "new_kernel_pair_ms": float(np.median(pi) - np.median(pj))}
        inertia_step(with_jc=False)
        inertia_step(with_jc=False)
        out["mode0"]["inertia_without_jc_contraction_phase_ms"] = float(eng.last_timings()[4])
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
