"""Time of a field sweep against the forward sweep of the same build, in one process, alternating (C3: ny = 25,
19,353 DOF, one lane, one chunk of 2,048 frequencies by default; check mode 3):

  (a) pfr_sweep(PFR_LOSS_NONE)                      the yardstick
  (b) pfr_field_sweep over every row               n x 16 B read and written per frequency more than (a)
  (c) pfr_field_sweep over the V vertex rows of w

Each sample is a host clock around one C call that ends in a device synchronise, on buffers allocated before the
timed window.  Then, with the solver's HIP events on, the gather's own time (the field sweep's last phase,
pfr_last_timings) and from it the kernel's achieved bandwidth: 2 x nfreq x n_sel x 16 B plus the index list.

    python tools/field_time.py [--nfreq 2048] [--reps 9] [--out FILE.json]
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
from plate_inverse_problem_amd import _native  # noqa: E402


def stats(t):
    return {"median": 1e3 * float(np.median(t)), "min": 1e3 * min(t), "max": 1e3 * max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, default=25)
    ap.add_argument("--nfreq", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["PFR_LANES"] = "1"               # read when the engine is built: the whole sweep is one chunk
    if not torch.cuda.is_available():
        raise SystemExit("field_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    p = bench.build_problem(a.ny, dev, max_batch=a.nfreq)
    freqs = np.linspace(40.0, 600.0, a.nfreq)
    p.solveForward(freqs)                        # builds the engine and sets the coefficients
    eng = p.engine()
    sv = eng.solver
    assert eng.n_lanes == 1 and sv.max_batch >= a.nfreq
    mode = _native.PFR_CHECK_FORWARD | _native.PFR_CHECK_ADJOINT
    eng.set_check(mode)
    n, F = p.mat_size, a.nfreq
    w_rows = p.vertex_rows()[2]
    f_dev = p._freqs(freqs)
    fr = torch.empty(F, dtype=torch.float64, device=dev)
    flags = torch.zeros(F, dtype=torch.int32, device=dev)
    out_all = torch.empty((F, n), dtype=torch.complex128, device=dev)
    out_w = torch.empty((F, w_rows.size), dtype=torch.complex128, device=dev)

    def forward():
        sv.sweep(f_dev, _native.LOSS_NONE, fr=fr, flags=flags)
        torch.cuda.synchronize()

    def field_all():
        sv.field_sweep(f_dev, out_all, fr=fr, flags=flags)
        torch.cuda.synchronize()

    def field_w():
        sv.field_sweep(f_dev, out_w, rows=w_rows, fr=fr, flags=flags)
        torch.cuda.synchronize()

    steps = (("forward", forward), ("field_all", field_all), ("field_w", field_w))
    for _ in range(2):                           # every shape of the timed window warmed up
        for _, fn in steps:
            fn()
    t = {k: [] for k, _ in steps}
    for _ in range(a.reps):
        for k, fn in steps:
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = {"ny": a.ny, "dof": int(n), "vertex_rows": int(w_rows.size), "nfreq": F, "lanes": eng.n_lanes,
           "max_batch": sv.max_batch, "check_mode": mode, "reps": a.reps, "tile_rows": _native.field_tile_rows(),
           "forward_ms": stats(t["forward"]), "field_all_ms": stats(t["field_all"]), "field_w_ms": stats(t["field_w"]),
           "ratio_all": med["field_all"] / med["forward"], "ratio_w": med["field_w"] / med["forward"],
           "extra_all_ms": 1e3 * (med["field_all"] - med["forward"]),
           "bytes_all_per_freq": 32 * int(n), "factor_bytes_per_freq": int(sv.alg_bytes().sum())}
    # the phases from the solver's events: the field sweep's last phase is the gather alone
    eng.set_timing(True)
    try:
        forward()
        out["forward_phases_ms"] = [float(v) for v in eng.last_timings()]
        for key, fn, n_sel in (("all", field_all, n), ("w", field_w, int(w_rows.size))):
            g = []
            for _ in range(5):
                fn()
                g.append(float(eng.last_timings()[4]))
            out[f"field_{key}_phases_ms"] = [float(v) for v in eng.last_timings()]
            ms = float(np.median(g))
            out[f"gather_{key}_ms"] = {"median": ms, "min": min(g), "max": max(g)}
            out[f"gather_{key}_TBps"] = (2.0 * F * n_sel * 16 + 4 * n_sel) / (ms * 1e-3) / 1e12 if ms > 0 else None
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
