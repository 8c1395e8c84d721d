"""GPU: pruning (include/pfr.h, pfr_set_prune; the engine's default, PFR_PRUNE=0 turns it off) against the full
plan, orthotropic ny = 6, 100 frequencies, one lane.

Exact by construction, whatever the schedules: the forward rows of unloaded trees are 0.0, the partials of the A
matrices are 0.0, the flags are equal, the adjoint's backward error (taken over the loaded rows) is not larger.

The numbers the sweeps return -- loss, the 18 partials, fr, Jacobian rows, the complex response, a population member
-- are bit-equal when the active view's schedule agrees with the full one, on the levels that hold loaded fronts, in
every column that is not a count (the forms, splits, wave counts, row blocks and LDS sizes: what orders the
arithmetic).  A view takes its launch decisions as the full plan takes them (plan.hpp, level_schedule), so they agree
for every chunk size; ``test_schedules_agree`` asserts that first, for the chunks used here (128 and 64).  Should
they ever not agree, each of on and off is held to the bounds tests/test_gpu_fullsize.py states against the oracle for
ny <= 6 -- fr and loss 5e-9, gradient 1e-7, backward error 1e-12.  The on-versus-off differences are reported either
way ($PFR_TEST_REPORT)."""
import gc
import os

import numpy as np
import pytest
import torch

from helpers import make_problem, oracle_for, report

pytestmark = pytest.mark.gpu

FR_RTOL, GRAD_RTOL, BERR_MAX = 5e-9, 1e-7, 1e-12      # tests/test_gpu_fullsize.py, ny <= 6
ADJ_SEED_BERR = 1e-8                                    # tests/test_gpu_debug_solution.py
FREQS = np.linspace(40.0, 600.0, 100)
COUNTS = {"factor": ("nf", "f0_small", "nasm", "nitems", "nblocks", "ntiles"), "pair": ("nf",),
          "chain": ("nf0", "nf1", "nmax", "nsum"), "solve_all": ("nf",), "solve_reach0": ("nf",), "solve_reach1": ("nf",)}


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _schedules_agree(on, off):
    """The active view's records against the full schedule's on the levels with loaded fronts, counts aside."""
    for name, skip in COUNTS.items():
        lv = on[name]["nmax" if name == "chain" else "nf"] > 0
        for col in on[name].dtype.names:
            if col not in skip and not np.array_equal(on[name][col][lv], off[name][col][lv]):
                return False
    return True


def _engine_run(prune, material="orthotropic", max_batch=None):
    """Everything the comparisons need from one engine, as host arrays."""
    from oracle.plate_oracle import loss_and_grad
    from plate_inverse_problem_amd import _native
    from plate_inverse_problem_amd.Problem import _coeffs18
    old = {k: os.environ.get(k) for k in ("PFR_PRUNE", "PFR_LANES")}
    os.environ["PFR_PRUNE"] = "1" if prune else "0"
    os.environ["PFR_LANES"] = "1"
    p = make_problem(material, ny=6, device="cuda:0", max_batch=max_batch)
    try:
        out = {}
        fr, berr, flags = p.solveForwardChecked(FREQS)
        out["fr"], out["berr_f"], out["flags_f"] = fr, berr, flags
        ref = fr * np.exp(0.1j) * 1.02
        theta = p.parameters * 1.04
        x = torch.tensor(theta, requires_grad=True)
        val = p.getLossFunction(FREQS, ref, "MSE_LOG_AFC")(x)
        val.backward()
        out["loss"], out["grad"] = val.item(), x.grad.numpy().copy()
        eng = p.engine()
        assert eng.n_lanes == 1
        sv = eng.solvers[0]
        out["berr"] = eng.last_berr.cpu().numpy().copy()
        out["flags"] = np.asarray(eng.last_flags).copy()
        out["mask"] = sv.active_fronts().astype(bool)
        out["sched_on"], out["sched_full"] = sv.schedule_active(), sv.schedule()
        out["fronts"], out["perm"] = eng.sym.export("FRONTS"), eng.sym.export("PERM")
        # the 18 partials of one sweep, and the last chunk's vectors (caller numbering)
        dev = eng.device
        eng.set_coefficients(_coeffs18(p._transform(), torch.as_tensor(theta)).detach().numpy())
        w = torch.zeros(eng.n_stiff, dtype=torch.complex128, device=dev)
        loss = torch.zeros(1, dtype=torch.float64, device=dev)
        eng.sweep(torch.as_tensor(FREQS, device=dev), _native.LOSS_MSE_LOG_AFC,
                  ref=torch.view_as_real(torch.as_tensor(ref.astype(np.complex128), device=dev)), scale=1.0, loss=loss,
                  w=torch.view_as_real(w))
        torch.cuda.synchronize()
        out["w18"] = eng.expand(w).cpu().numpy()
        assert eng.n_stiff == 12 or material != "orthotropic"
        q_last = (FREQS.size - 1) % eng.max_batch
        out["x_last"] = sv.debug_solution(0, q_last)
        out["mu_last"] = sv.debug_solution(1, q_last)
        _, J = p.solveForwardJacobian(FREQS, theta)
        out["jac"] = J
        out["H"] = p.solveForwardComplex(FREQS, theta, axis=(0.1, 0.2, 1.0))
        out["pop"] = p.solveForwardPopulation(FREQS, np.stack([p.parameters, theta]))[1]
        orc = oracle_for(p)
        out["fr_orc"] = orc.fr(FREQS, p.parameters)
        out["lg_orc"] = loss_and_grad(orc, FREQS, ref, "MSE_LOG_AFC", theta)
        return out
    finally:
        p._engine = None
        del p
        gc.collect()
        torch.cuda.empty_cache()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def pair():
    return _engine_run(True), _engine_run(False)


def _unloaded_rows(r):
    rows = []
    for t, (ns, f, row0, col0, *_r) in enumerate(r["fronts"]):
        if not r["mask"][t]:
            rows.extend(r["perm"][col0:col0 + ns].tolist())
    return np.asarray(rows, dtype=np.int64)


def test_schedules_agree(pair):
    on, off = pair
    assert _schedules_agree(on["sched_on"], off["sched_full"])
    assert on["sched_on"]["factor"]["nf"].sum() == on["mask"].sum() < off["sched_full"]["factor"]["nf"].sum()


def test_exact_by_construction(pair):
    on, off = pair
    assert 0 < on["mask"].sum() < on["mask"].size and off["mask"].all()
    rows = _unloaded_rows(on)
    assert rows.size > 0
    for r in (on, off):                       # the forward solution of the in-plane block is exactly zero
        assert np.all(r["x_last"].view(np.complex128)[rows] == 0.0)
        assert np.all(r["w18"][:6] == 0.0) and np.all(r["w18"][6:12] == 0.0)      # A (and the dropped B) partials
        assert np.any(r["w18"][12:] != 0.0)
    assert np.array_equal(on["flags_f"], off["flags_f"]) and np.array_equal(on["flags"], off["flags"])
    assert np.all(on["flags"] == 0)
    # the forward backward error is bit-equal; the adjoint's is taken over the loaded rows only: not larger
    assert np.array_equal(on["berr_f"], off["berr_f"]) and np.array_equal(on["berr"][:, 0], off["berr"][:, 0])
    assert np.all(on["berr"][:, 1] <= off["berr"][:, 1])
    report("prune_adjoint_berr", on=float(on["berr"][:, 1].max()), off=float(off["berr"][:, 1].max()))


def test_results_on_against_off(pair):
    on, off = pair
    keys = ("fr", "loss", "grad", "w18", "jac", "H", "pop")
    diffs = {k: _rel(on[k], off[k]) for k in keys}
    report("prune_on_vs_off", **diffs)
    if _schedules_agree(on["sched_on"], off["sched_full"]):
        for k in keys:
            assert np.array_equal(on[k], off[k]), (k, diffs[k])
        return
    for tag, r in (("on", on), ("off", off)):
        lo, go = r["lg_orc"]
        e = dict(fr=_rel(r["fr"] / r["fr_orc"], np.ones(FREQS.size)), loss=abs(r["loss"] - lo) / abs(lo),
                 grad=_rel(r["grad"], go), berr_f=float(np.max(r["berr_f"])), berr=float(np.max(r["berr"])))
        report("prune_" + tag + "_vs_oracle", **e)
        assert e["fr"] < FR_RTOL and e["loss"] < FR_RTOL and e["grad"] < GRAD_RTOL, (tag, e)
        assert e["berr_f"] <= BERR_MAX and e["berr"] <= BERR_MAX, (tag, e)
    # the sweeps the oracle has no twin for here: on against off within the sum of the two fr bounds
    for k in ("jac", "H", "pop"):
        assert diffs[k] < 2 * (GRAD_RTOL if k == "jac" else FR_RTOL), (k, diffs[k])


def _adjoint_bound(orc, sv, theta, freqs, q, lane):
    """tests/test_gpu_debug_solution.py's checks of the accessor's vectors for frequency q (chunk lane ``lane``)."""
    c = orc.coefficients(theta)
    aU, aV, aW = orc.averaging_vectors()
    ts2 = orc.acc_ts ** 2
    A = orc.matrix(freqs[q], c).tocsc()
    b = orc.rhs_vec * orc.rhs_scale(freqs[q], c)
    x, mu = sv.debug_solution(0, lane), sv.debug_solution(1, lane)
    r = b - A @ x
    den = abs(A) @ np.abs(x) + np.abs(b)
    assert np.max(np.abs(r)[den > 0] / den[den > 0]) < BERR_MAX, q
    U, V, W = aU @ x, aV @ x, aW @ x
    fr = np.sqrt(ts2 * abs(U) ** 2 + ts2 * abs(V) ** 2 + abs(W) ** 2)
    g = (ts2 * np.conj(U) * aU + ts2 * np.conj(V) * aV + np.conj(W) * aW) / fr
    ra = g - A.T @ mu
    dena = abs(A.T) @ np.abs(mu) + np.abs(g)
    assert np.max(np.abs(ra)[dena > 0] / dena[dena > 0]) < ADJ_SEED_BERR, q
    return mu


def test_no_stale_state_and_whole_adjoint(monkeypatch):
    """Two sweeps at different theta on one engine, then one sweep of 100 frequencies in two chunks of 64: after each
    the accessor's adjoint solves the whole system (the unloaded trees completed on demand, for that chunk)."""
    from plate_inverse_problem_amd import _native
    from plate_inverse_problem_amd.Problem import _coeffs18
    monkeypatch.setenv("PFR_LANES", "1")
    for max_batch in (None, 64):
        p = make_problem("orthotropic", ny=6, device="cuda:0", max_batch=max_batch)
        orc = oracle_for(p)
        ref = orc.fr(FREQS, p.parameters).astype(np.complex128)
        eng = p.engine(FREQS.size)
        sv = eng.solvers[0]
        dev = eng.device
        mus = []
        for scale in ((1.03, 0.97) if max_batch is None else (1.03,)):
            theta = p.parameters * scale
            eng.set_coefficients(_coeffs18(p._transform(), torch.as_tensor(theta)).detach().numpy())
            w = torch.zeros(eng.n_stiff, dtype=torch.complex128, device=dev)
            loss = torch.zeros(1, dtype=torch.float64, device=dev)
            eng.sweep(torch.as_tensor(FREQS, device=dev), _native.LOSS_MSE_LOG_AFC,
                      ref=torch.view_as_real(torch.as_tensor(ref, device=dev)), scale=1.0, loss=loss,
                      w=torch.view_as_real(w))
            torch.cuda.synchronize()
            assert 0 < sv.active_fronts().sum() < sv.active_fronts().size
            first = 0 if max_batch is None else 64          # the last chunk's first frequency
            for q in (first, first + 17, FREQS.size - 1):
                mus.append(_adjoint_bound(orc, sv, theta, FREQS, q, q - first))
        if max_batch is None:
            assert not np.array_equal(mus[0], mus[3])        # the second theta's vectors, not the first's
        p._engine = None
        del p, eng, sv
        gc.collect()
        torch.cuda.empty_cache()


def test_sol_on_and_off_bit_equal():
    on, off = _engine_run(True, "sol"), _engine_run(False, "sol")
    assert on["mask"].all() and off["mask"].all()
    for name in on["sched_on"]:
        assert np.array_equal(on["sched_on"][name], off["sched_full"][name]), name
    for k in ("fr", "loss", "grad", "w18", "jac", "H", "pop", "berr", "berr_f", "flags", "x_last", "mu_last"):
        assert np.array_equal(on[k], off[k]), k


def _deep_tree_run(monkeypatch, prune):
    """ny = 6 on the deep tree (leaf 10,000: 16 levels, the in-plane trees 13 deep): first the plate's own load, whose
    complement view has no front on levels 13-15, with the accessor's adjoint checked; then a load on an in-plane
    row, whose ACTIVE view has none there, with the loss sweep's outputs returned."""
    from plate_inverse_problem_amd import _native
    from plate_inverse_problem_amd.Problem import _coeffs18
    monkeypatch.setenv("PFR_LANES", "1")
    monkeypatch.setenv("PFR_LEAF_SIZE", "10000")
    monkeypatch.setenv("PFR_PRUNE", "1" if prune else "0")
    p = make_problem("orthotropic", ny=6, device="cuda:0")
    try:
        orc = oracle_for(p)
        theta = p.parameters * 1.03
        eng = p.engine(FREQS.size)
        sv, dev = eng.solvers[0], eng.device
        c = _coeffs18(p._transform(), torch.as_tensor(theta)).detach().numpy()
        fr_dev = torch.zeros(FREQS.size, dtype=torch.float64, device=dev)

        def sweep(ref):
            w = torch.zeros(eng.n_stiff, dtype=torch.complex128, device=dev)
            loss = torch.zeros(1, dtype=torch.float64, device=dev)
            flags = torch.zeros(FREQS.size, dtype=torch.int32, device=dev)
            eng.sweep(torch.as_tensor(FREQS, device=dev), _native.LOSS_MSE_LOG_AFC,
                      ref=torch.view_as_real(torch.as_tensor(ref.astype(np.complex128), device=dev)), scale=1.0,
                      fr=fr_dev, loss=loss, w=torch.view_as_real(w), flags=flags)
            torch.cuda.synchronize()
            return loss.item(), eng.expand(w).cpu().numpy(), fr_dev.cpu().numpy().copy(), int(flags.count_nonzero())

        eng.set_coefficients(c)
        out = {"plate": sweep(orc.fr(FREQS, p.parameters))}
        fronts, perm = eng.sym.export("FRONTS"), eng.sym.export("PERM")
        levels = fronts[:, 5]
        mask = sv.active_fronts().astype(bool)
        if prune:
            # the rest has no front on the top levels: the accessor's completion launches nothing there
            top = levels.max()
            assert mask[levels == top].all() and levels[~mask].max() < top and (~mask).any()
            for q in (0, 37, 99):
                _adjoint_bound(orc, sv, theta, FREQS, q, q)
        # a load on a pivot row of the deepest unloaded (in-plane) tree
        inpl = ~eng.sym.prune(FREQS.size, p.vec, eng._sup)[0].astype(bool)     # the plate's own unloaded fronts
        t = int(np.nonzero(inpl & (fronts[:, 4] >= 0))[0][0])
        rhs = np.zeros(p.mat_size)
        rhs[perm[fronts[t, 3]]] = 1.0
        eng.rhs = rhs
        eng._coef_key = None
        eng.set_coefficients(c)
        mask2 = sv.active_fronts().astype(bool)
        if prune:
            assert mask2[t] and not np.array_equal(mask2, mask)
            assert levels[mask2].max() < levels.max()           # the active view's top levels are empty
        else:
            assert mask2.all()
        first = sweep(np.ones(FREQS.size))
        out["inplane"] = sweep(first[2] * 1.02)
        return out
    finally:
        p._engine = None
        del p
        gc.collect()
        torch.cuda.empty_cache()


def test_views_with_empty_levels(monkeypatch):
    """A view may hold no front on a level (plan.hpp): the complement of the plate's load on the deep tree, and the
    active view of an in-plane load.  Every pass must launch nothing there; results stay the full plan's bits."""
    on, off = _deep_tree_run(monkeypatch, True), _deep_tree_run(monkeypatch, False)
    for case in ("plate", "inplane"):
        assert on[case][3] == 0 and off[case][3] == 0, case
        assert np.all(np.isfinite(on[case][2])) and np.all(on[case][2] > 0), case
        for i in range(3):
            assert np.array_equal(on[case][i], off[case][i]), (case, i)
