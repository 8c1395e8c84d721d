"""Time of a field-loss sweep against its parts, in one process, alternating (C3: ny = 25, 19,353 DOF, one lane, one
chunk of 2,048 frequencies by default; check mode 3):

  (a) pfr_field_sweep over every row                     the forward sweep and the gather
  (b) pfr_field_loss_sweep over the V vertex rows of w   FIELD_MSE
  (c) pfr_field_loss_sweep over every row                FIELD_MSE, and FIELD_MAC (four sums per tile, not one)
  (d) pfr_sweep, loss + gradient                         the paired reverse sweep the project's other losses run

From the code (c) is (a) without the gather, plus the three field-loss kernels, one unpaired adjoint solve over every
front, k_contract_eg, the adjoint check walk, k_rhs_dot and k_reduce.  Each sample is a host clock around one C call
that ends in a device synchronise, on buffers allocated before the timed window.  Then, with the solver's HIP events
on, the phases of each (pfr_last_timings: factor, forward, functional -- here k_zero on G and the three kernels --,
adjoint, finish), and the sum of the parts against the whole.

The three kernels' own times come from a profiler run of this script (a separate process, fewer repetitions):
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/field_loss_time.py --reps 2
    python tools/kernel_stats.py DIR/.../*_results.db --out STATS.csv
    python tools/field_loss_time.py --kernel-stats STATS.csv --merge FILE.json
which adds their average durations, the bytes each moves and the bandwidth to FILE.json.

    python tools/field_loss_time.py [--nfreq 2048] [--reps 9] [--out FILE.json]
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NSUM = {"FIELD_MSE": 1, "FIELD_RMSE": 2, "FIELD_MAC": 4}


def stats(t):
    return {"median": 1e3 * float(np.median(t)), "min": 1e3 * min(t), "max": 1e3 * max(t)}


def kernel_bytes(F, n_sel, nsum, tile_rows):
    """Bytes each of the three kernels reads and writes (complex 16 B, the partials 8 B; index lists left out)."""
    tiles = -(-n_sel // tile_rows)
    return {"k_field_terms": 48 * F * n_sel + 8 * tiles * nsum * F,       # ref and X in, G and the partials out
            "k_field_finish": 8 * tiles * nsum * F + 32 * F,              # the partials in, term and coefficients out
            "k_field_seed": 48 * F * n_sel + 24 * F}                      # X and G in, G out


def merge_kernel_stats(stats_csv, path):
    """Average durations of the k_field_* kernels from a kernel_stats.py CSV into the JSON at ``path``."""
    with open(path) as fh:
        out = json.loads(fh.read())
    F, n = out["nfreq"], out["dof"]
    with open(stats_csv, newline="") as fh:
        table = list(csv.DictReader(fh))
    want = ("Name", "Calls", "AverageNs", "MinNs", "MaxNs")       # tools/kernel_stats.py's columns, by name
    if not table or any(c not in table[0] for c in want):
        raise SystemExit(f"{stats_csv}: expected the columns {want} of tools/kernel_stats.py")
    kern = {}
    for r in table:
        if "k_field_" not in r["Name"]:
            continue
        kern[r["Name"].replace("pfr::", "")] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
                                                "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
    if not kern:
        raise SystemExit(f"{stats_csv}: no k_field_* kernel in it")
    out["kernels_note"] = ("averages over every launch of the profiled run: the all-rows and the vertex-row sweeps "
                           "together for k_field_seed and per loss id for the templates; min is the vertex-row "
                           "launch, max the all-rows one")
    by = kernel_bytes(F, n, 1, out["tile_rows"])
    by4 = kernel_bytes(F, n, 4, out["tile_rows"])
    out["kernel_bytes_all_rows"] = {"FIELD_MSE": by, "FIELD_MAC": by4}
    for short, k in kern.items():
        base = short.split("<")[0]
        b = (by4 if "<34>" in short else by).get(base)
        if b and k["max_us"] > 0:
            k["TBps_all_rows_at_max"] = b / (k["max_us"] * 1e-6) / 1e12
    out["kernels"] = kern
    with open(path, "w") as fh:
        fh.write(json.dumps(out) + "\n")
    print(json.dumps(out["kernels"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, default=25)
    ap.add_argument("--nfreq", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--merge", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return merge_kernel_stats(a.kernel_stats, a.merge)
    import torch

    import bench
    from plate_inverse_problem_amd import _native
    os.environ["PFR_LANES"] = "1"               # read when the engine is built: the whole sweep is one chunk
    if not torch.cuda.is_available():
        raise SystemExit("field_loss_time.py needs a GPU")
    dev = torch.device("cuda", 0)
    p = bench.build_problem(a.ny, dev, max_batch=a.nfreq)
    freqs = np.linspace(40.0, 600.0, a.nfreq)
    fr_ref = p.solveForward(freqs)               # builds the engine and sets the coefficients
    eng = p.engine()
    sv = eng.solver
    assert eng.n_lanes == 1 and sv.max_batch >= a.nfreq
    mode = _native.PFR_CHECK_FORWARD | _native.PFR_CHECK_ADJOINT
    eng.set_check(mode)
    n, F = p.mat_size, a.nfreq
    w_rows = p.vertex_rows()[2]
    f_dev = p._freqs(freqs)
    flags = torch.zeros(F, dtype=torch.int32, device=dev)
    fr = torch.empty(F, dtype=torch.float64, device=dev)
    out_all = torch.empty((F, n), dtype=torch.complex128, device=dev)
    sv.field_sweep(f_dev, out_all, flags=flags)
    torch.cuda.synchronize()
    # the data: the field itself with an amplitude and phase error per point (fixed seed)
    rng = np.random.default_rng(0)
    fac = torch.as_tensor((1 + 0.3 * rng.uniform(-1, 1, n)) * np.exp(1j * rng.uniform(-1, 1, n)), device=dev)
    ref_all = (out_all * fac).contiguous()
    ref_w = ref_all[:, torch.as_tensor(w_rows, device=dev)].contiguous()
    ref_fr = torch.view_as_real(torch.as_tensor((fr_ref * 1.01).astype(np.complex128), device=dev))
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    w = torch.zeros(eng.n_stiff, dtype=torch.complex128, device=dev)
    wr = torch.view_as_real(w)

    def field_all():
        sv.field_sweep(f_dev, out_all, flags=flags)
        torch.cuda.synchronize()

    def floss(ref, rows, lt):
        def run():
            sv.field_loss_sweep(f_dev, lt, ref, wr, rows=rows, scale=1.0 / F, loss=loss, flags=flags, fresh=True)
            torch.cuda.synchronize()
        return run

    def loss_sweep():
        sv.sweep(f_dev, _native.LOSS_MSE_LOG_AFC, ref=ref_fr, scale=1.0 / F, fr=fr, loss=loss, w=wr, flags=flags,
                 fresh=True)
        torch.cuda.synchronize()

    steps = (("field_all", field_all), ("floss_w", floss(ref_w, w_rows, _native.LOSS_FMSE)),
             ("floss_all", floss(ref_all, None, _native.LOSS_FMSE)),
             ("floss_all_mac", floss(ref_all, None, _native.LOSS_FMAC)), ("loss_sweep", loss_sweep))
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
           "n_stiff": eng.n_stiff}
    for k in t:
        out[k + "_ms"] = stats(t[k])
    out["ratio_floss_all_to_field_all"] = med["floss_all"] / med["field_all"]
    out["ratio_floss_all_to_loss_sweep"] = med["floss_all"] / med["loss_sweep"]
    out["ratio_floss_w_to_floss_all"] = med["floss_w"] / med["floss_all"]
    # the phases from the solver's events
    eng.set_timing(True)
    try:
        ph = {}
        for k, fn in steps:
            rows_ = []
            for _ in range(5):
                fn()
                rows_.append([float(v) for v in eng.last_timings()])
            ph[k] = [float(x) for x in np.median(np.array(rows_), axis=0)]
            out[k + "_phases_ms"] = ph[k]
    finally:
        eng.set_timing(False)
    # (c) against its parts measured in this run: (a)'s factorisation and forward phases, its own other phases
    a_fwd = ph["field_all"][0] + ph["field_all"][1]
    c = ph["floss_all"]
    out["floss_all_phase_sum_ms"] = float(sum(c))
    out["floss_all_parts_ms"] = {"factor_and_forward_of_a": a_fwd, "factor_and_forward_own": c[0] + c[1],
                                 "zero_and_three_kernels": c[2], "unpaired_adjoint": c[3],
                                 "contract_walk_rhs_dot_reduce": c[4], "gather_of_a": ph["field_all"][4]}
    out["floss_all_excess_over_parts_ms"] = float(sum(c)) - (a_fwd + c[2] + c[3] + c[4])
    out["host_minus_events_ms"] = {k: 1e3 * med[k] - float(sum(ph[k])) for k in ph}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
