"""GPU: pruned sweeps (include/pfr.h, pfr_set_prune) on the synthetic forests of tests/synthetic.py -- the views
csrc/api.cpp make_view / upload_view build over the loaded trees and, for the accessor's adjoint, over the rest, at
every launch class (tests/test_synthetic_forest_cpu.py lists which view runs which).

a. Against the extended-precision reference of the whole block-diagonal operator (test_against_the_reference), at the
   bound of tests/test_gpu_synthetic.py, 10 x max(e_model, e_dense, 1e-14), from the model on the forest's own analysis
   at run time: fr at every frequency, the loss, every w_k, x and the adjoint of every lane of the last chunk.  The
   adjoint read through the accessor is the completed one (the rest's view factorised and solved on demand).  x on
   the unloaded components is exactly 0.0; every flag 0, every backward error <= BERR_MAX.
b. Pruning on against off, bit for bit (test_on_off, test_knob_on_off): the active schedule first (no column that is
   not a count may differ), then np.array_equal on the outputs of every sweep entry point.  No tolerance anywhere.
c. State sequences on one solver against fresh solvers put directly into the same state (test_state_*).

130 frequencies at max_batch 64 (two chunks and a 2-lane tail); on ETF0 (n = 560) every other one.

Measured on an MI355X, pruning on (raw = check mode FORWARD | ADJOINT, default = mode 11 where the accessor's vector is
mu = A^-T d fr / d x; the adjoint's backward error is taken over the loaded rows with pruning on):

  case         n      raw: x / lam / fr / loss / w                default: fr / loss / w / mu         adjoint berr on / off
  AC-load0     277    1.6e-16 8.5e-15 8.4e-15 9.3e-15 4.3e-14    5.3e-16 3.0e-15 3.6e-15 1.2e-15    1.9e-15 / 2.2e-15
  AC-load1     277    2.2e-16 2.0e-14 8.4e-16 9.7e-16 1.7e-15    3.5e-16 1.9e-15 1.9e-15 2.1e-16    2.2e-15 / 2.2e-15
  ETF0-load0   560    2.2e-16 2.0e-15 1.3e-15 4.2e-15 8.9e-15    5.0e-16 1.4e-15 2.4e-15 9.7e-17    2.9e-15 / 2.9e-15
  ETF0-load1   560    1.7e-16 4.2e-14 1.5e-15 9.7e-16 9.1e-15    3.4e-16 5.3e-16 4.3e-15 1.0e-16    1.2e-15 / 2.8e-15
  ETF0-load2   560    1.1e-16 6.1e-15 2.4e-15 1.4e-15 1.1e-14    5.1e-16 3.6e-15 5.2e-15 3.4e-16    6.6e-16 / 3.1e-15
  BFA4-load02  456    4.9e-16 3.7e-14 2.9e-15 1.7e-15 1.7e-14    2.3e-15 2.1e-15 1.8e-14 5.5e-16    1.5e-15 / 2.1e-15
  FA8-load0    288    2.6e-16 4.5e-14 3.0e-15 5.5e-15 3.0e-14    4.4e-16 1.7e-15 3.6e-15 3.5e-16    1.8e-15 / 1.8e-15
  FA8-load1    288    9.1e-16 5.1e-14 3.6e-15 2.3e-15 2.9e-14    5.6e-16 3.9e-15 4.5e-15 3.8e-16    1.0e-15 / 2.4e-15
  F0F0-load0   52     1.2e-16 2.1e-14 6.9e-15 1.3e-14 1.4e-13    1.3e-15 1.2e-15 1.2e-14 1.6e-16    8.6e-16 / 1.5e-15
  F0F0-load1   52     8.7e-17 1.3e-14 5.3e-15 7.2e-15 3.4e-14    6.2e-16 2.5e-15 9.9e-15 2.1e-16    3.7e-15 / 3.7e-15
  F0G-load0    48     8.4e-17 2.6e-14 6.1e-15 9.9e-15 3.7e-14    5.3e-16 3.0e-15 7.1e-15 2.3e-16    8.8e-16 / 1.0e-15
  F0G-load1    48     1.5e-16 1.3e-14 9.8e-15 9.7e-15 7.9e-14    2.8e-15 1.5e-15 8.1e-14 2.4e-16    6.6e-16 / 1.0e-15
  A4A4-load0   96     1.5e-16 2.2e-14 1.9e-15 3.6e-15 1.8e-14    4.5e-16 2.5e-15 2.1e-15 2.5e-16    8.0e-16 / 1.5e-15
  A8A8-load1   110    3.6e-16 1.8e-14 7.5e-15 2.6e-16 6.7e-14    1.3e-15 3.3e-15 1.4e-14 2.3e-16    1.1e-15 / 1.2e-15
  DA8T-load2   499    1.7e-16 3.3e-15 3.1e-15 4.5e-15 4.4e-15    5.0e-16 1.1e-15 2.7e-15 4.5e-16    1.3e-15 / 3.2e-15
  DA8T-load0   499    5.3e-16 1.6e-15 1.5e-15 3.6e-15 4.5e-15    3.7e-16 5.6e-15 3.3e-15 3.0e-16    2.5e-15 / 2.5e-15

The bounds are 1.0e-13 (the floor) for x and fr, 1.1e-13 .. 4.7e-13 for lam, 1.0e-13 .. 5.9e-13 for the loss and
1.0e-13 .. 8.9e-13 for w; the closest is w of F0F0-load0, 1.4e-13 against 1.6e-13 (as in tests/test_gpu_synthetic.py,
lam, the loss and w carry what fp64 loses in (log fr - log |ref|)^2).  Largest backward error 3.7e-15, no flag.  AC
loaded on C against the other references: Jacobian rows 3.1e-15, complex H / loss / w / rows 9.8e-16 / 2.9e-16 / 8.0e-16 /
3.1e-15, a population member's rows 5.2e-15 (bounds 1.0e-13); the accessor's second adjoint 6.0e-15.  Every on / off
comparison and every state sequence held bit for bit, the knob variants included.
"""
import numpy as np
import pytest
import torch

import synthetic as sy
import synthetic_jacobian as sj
import synthetic_population as sp
from helpers import report
from plate_inverse_problem_amd import _native
from test_gpu_synthetic import DEFAULT, DEV, KNOBS, LOSS_ID, RAW, _bounds, _t, check_sweep, make_solver, run_sweep
from test_gpu_synthetic_complex import _cbounds, check_complex, run_cjacobian, run_complex
from test_gpu_synthetic_hessian import run_hessian
from test_gpu_synthetic_jacobian import _jac_bounds, check_jacobian, run_jacobian

pytestmark = pytest.mark.gpu
REFINE, REFINE_ADJ = _native.PFR_CHECK_REFINE, _native.PFR_CHECK_REFINE_ADJ
AXIS = (0.1, 0.2, 1.0)
CASE_IDS = [sy.forest_id(f, l) for f, l in sy.FOREST_CASES]


def _freqs(forest):
    """The sweep of a forest: the 130 FREQS; on ETF0 every other one (65: one chunk and a 1-lane tail), as weak_freqs
    does for shape E -- its reference costs the host ~8 s per 130 frequencies."""
    return sy.FREQS[::2] if forest == "ETF0" else sy.FREQS


def _case(forest, load):
    pat, op = sy.case(forest, load=load)
    return pat, op, sy.symbolic(forest), _freqs(forest)


def _unloaded_rows(pat, load):
    return sy.component_rows(pat, [k for k in range(len(pat.parts)) if k not in load])


def _assert_pruned(sv, sym, pat, load):
    """The solver sweeps a real view: exactly the loaded components' fronts, and its schedule takes every decision as
    the full plan does (no column that is not a count differs on the view's levels)."""
    mask = sv.active_fronts().astype(bool)
    perm, fr = sym.export("PERM"), sym.export("FRONTS")
    rows_on = np.concatenate([perm[c0:c0 + ns] for (ns, f, r0, c0, *_r), m in zip(fr, mask) if m])
    assert 0 < mask.sum() < mask.size
    assert np.array_equal(np.sort(rows_on), np.sort(sy.component_rows(pat, load)))
    assert sy.schedule_disagreements(sv.schedule_active(), sv.schedule()) == []


# ----------------------------------------------------------------------------- a. against the reference
@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("forest,load", sy.FOREST_CASES, ids=CASE_IDS)
def test_against_the_reference(forest, load, mode):
    pat, op, sym, freqs = _case(forest, load)
    name = f"prune-{sy.forest_id(forest, load)}-mode{mode}"
    correct = bool(mode & _native.PFR_CHECK_CORRECT)
    bound = _bounds(op, sym, freqs, "MSE_LOG_AFC", **({"correct": True} if correct else {}))
    solver = make_solver(op, sym, prune=True)
    _assert_pruned(solver[0], sym, pat, load)
    out = run_sweep(op, sym, freqs, mode=mode, solver=solver)
    check_sweep(name, out, bound, mode=mode)
    off = _unloaded_rows(pat, load)
    assert off.size and np.all(out["x"][:, off] == 0.0)
    assert np.all(np.isfinite(out["adj"].view(np.float64))) and np.any(out["adj"][:, off] != 0.0)   # completed there
    if correct:
        # the vector is mu = A^-T d fr / d x at the GPU's own x, completed on the unloaded trees by the accessor:
        # against the refined dense solve of the whole system, at the unrefined model's and dense solve's error
        refc, lanes = out["refc"], out["last"]
        e_raw, _, e_dense = sy.mu_model_errors(op, sym, freqs, lanes)
        mu_bound = 10 * np.maximum(np.maximum(e_raw, e_dense), sy.FLOOR)
        err = []
        for i, q in enumerate(lanes):
            seed = sy.adjoint_seed(op, out["x"][i].astype(sy.CLD), sy.LD(1))
            mu_ref = sy.refined_solve(refc.mats[q], seed, refc.lus[q], trans=True)[0]
            err.append(sy.rel(out["adj"][i], mu_ref))
            assert np.any(mu_ref[off] != 0)
        print(name, "mu", " ".join(f"{e:.2e}/{b:.1e}" for e, b in zip(err, mu_bound)))
        report("synthetic::" + name + "-mu", mu=max(err), mu_bound=float(mu_bound.max()))
        assert np.all(np.array(err) <= mu_bound), (err, mu_bound)


# ----------------------------------------------------------------------------- b. on against off, bit for bit
def _eq(name, on, off, keys):
    for k in keys:
        a, b = on[k], off[k]
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (name, k)


def _all_entry_points(op, sym, freqs, prune, mode, base_ops=None):
    """Every operator-form sweep entry point once on one solver; the outputs on the host by entry point."""
    solver = make_solver(op, sym, prune=prune)
    sv = solver[0]
    out = {"mask": sv.active_fronts(), "sched_active": sv.schedule_active(), "sched": sv.schedule()}
    out["sweep"] = run_sweep(op, sym, freqs, mode=mode, solver=solver)
    out["fresh"] = run_sweep(op, sym, freqs, mode=mode, solver=solver, fresh=True, vectors=False,
                             prefill=(3.0, 2.0, 7, 5.0))
    out["complex"] = run_complex(op, sym, freqs, AXIS, mode=mode, solver=solver)
    out["jacobian"] = run_jacobian(op, sym, freqs, mode=mode, solver=solver)
    out["cjacobian"] = run_cjacobian(op, sym, freqs, AXIS, mode=mode, solver=solver)
    if base_ops is not None:
        base, ops = base_ops
        f, member, valid = sp.lanes(2, freqs[:64])                            # 2 members x 64 lanes
        for jac in (True, False):
            out["pop-jc" if jac else "pop"] = sp.run_population(base, ops, sym, f, member, max_batch=64, mode=mode,
                                                                make_solver=make_solver, t=_t, jac=jac, solver=solver)
        out["lanes"] = (f, member, valid)
    return out


def _compare_on_off(name, pat, op, sym, freqs, load, mode, base_ops=None):
    on = _all_entry_points(op, sym, freqs, True, mode, base_ops)
    off = _all_entry_points(op, sym, freqs, False, mode, base_ops)
    mask = on["mask"].astype(bool)
    assert 0 < mask.sum() < mask.size and off["mask"].all()
    assert sy.schedule_disagreements(on["sched_active"], off["sched"]) == []
    for name_t in on["sched"]:
        assert np.array_equal(on["sched"][name_t], off["sched"][name_t]), name_t      # the full plan is untouched
    _eq(name, on["sweep"], off["sweep"], ("fr", "loss", "w", "flags", "x"))
    assert np.array_equal(on["sweep"]["berr"][:, 0], off["sweep"]["berr"][:, 0])
    assert np.all(on["sweep"]["berr"][:, 1] <= off["sweep"]["berr"][:, 1])            # taken over the loaded rows
    rows_off = _unloaded_rows(pat, load)
    rows_on = sy.component_rows(pat, load)
    assert np.all(on["sweep"]["x"][:, rows_off] == 0.0)
    assert np.array_equal(on["sweep"]["adj"][:, rows_on], off["sweep"]["adj"][:, rows_on])
    _eq(name, on["fresh"], off["fresh"], ("fr", "loss", "w", "flags"))
    _eq(name, on["complex"], off["complex"], ("H", "loss", "w", "flags"))
    _eq(name, on["jacobian"], off["jacobian"], ("fr", "jc", "flags"))
    _eq(name, on["cjacobian"], off["cjacobian"], ("H", "jc", "flags"))
    if base_ops is not None:
        for k in ("pop-jc", "pop"):
            _eq(name, on[k], off[k], ("fr", "flags") + (("jc",) if k == "pop-jc" else ()))
    assert np.all(on["sweep"]["flags"] == 0) and np.any(on["sweep"]["w"] != 0)
    report("synthetic::" + name, adj_berr_on=float(on["sweep"]["berr"][:, 1].max()),
           adj_berr_off=float(off["sweep"]["berr"][:, 1].max()), fwd_berr=float(on["sweep"]["berr"][:, 0].max()))
    return on, off


@pytest.mark.parametrize("forest,load", sy.FOREST_CASES, ids=CASE_IDS)
def test_on_off(forest, load):
    """pfr_sweep, pfr_sweep_fresh, pfr_sweep_complex with a loss, the two Jacobian sweeps and pfr_population_sweep with
    and without rows, default mode: the same bits with pruning on and off."""
    pat, op, sym, freqs = _case(forest, load)
    _compare_on_off(f"prune-onoff-{sy.forest_id(forest, load)}", pat, op, sym, freqs, load, DEFAULT,
                    sp.members(forest, 2, load=load))


def test_on_off_raw_mode():
    pat, op, sym, freqs = _case("AC", (1,))
    _compare_on_off("prune-onoff-AC-load1-raw", pat, op, sym, freqs, (1,), RAW, sp.members("AC", 2, load=(1,)))


@pytest.mark.parametrize("forest,load,env", sy.FOREST_KNOBS, ids=[sy.knob_id(*c) for c in sy.FOREST_KNOBS])
def test_knob_on_off(forest, load, env, monkeypatch):
    """The knob variants of tests/test_gpu_synthetic.py::KNOBS on the forests that hold the matching shape."""
    assert env in [e for _, e in KNOBS]
    for k, v in env.items():
        monkeypatch.setenv(k, v)              # the launch knobs are read in pfr_solver_create
    pat, op, sym, freqs = _case(forest, load)
    _compare_on_off("prune-onoff-" + sy.knob_id(forest, load, env), pat, op, sym, freqs, load, DEFAULT)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_other_sweeps_against_their_references(mode):
    """AC loaded on C, pruning on: the Jacobian, complex and population sweeps against the references and bounds of
    tests/synthetic_jacobian.py, synthetic_complex.py and synthetic_population.py."""
    load = (1,)
    pat, op, sym, freqs = _case("AC", load)
    correct = bool(mode & _native.PFR_CHECK_CORRECT)
    solver = make_solver(op, sym, prune=True)
    _assert_pruned(solver[0], sym, pat, load)
    check_jacobian(f"prune-AC-load1-mode{mode}", run_jacobian(op, sym, freqs, mode=mode, solver=solver),
                   _jac_bounds(op, sym, freqs, correct=correct))
    cb = _cbounds(op, sym, freqs, AXIS, correct=correct)
    for lt in ("MSE_LOG_COMPLEX", "CCOTANGENT"):
        check_complex(f"prune-AC-load1-mode{mode}-{lt}", run_complex(op, sym, freqs, AXIS, mode=mode, loss_type=lt,
                                                                      solver=solver), cb[lt], lt)
    check_complex(f"prune-AC-load1-mode{mode}-rows", run_cjacobian(op, sym, freqs, AXIS, mode=mode, solver=solver),
                  cb["CCOTANGENT"], None)
    base, ops = sp.members("AC", 2, load=load)
    f, member, valid = sp.lanes(2, freqs)
    pop = sp.run_population(base, ops, sym, f, member, max_batch=64, mode=mode, make_solver=make_solver, t=_t,
                            solver=solver)
    assert np.all(pop["flags"] == 0)
    for p, m in list(enumerate(ops))[1:]:                    # member 1, as tests/test_gpu_synthetic_population.py
        sel = np.repeat(member == p, 64) & valid
        refc = sy.reference(m, freqs)
        b, em, ed = _jac_bounds(m, sym, freqs, correct=correct)
        err = {"jc": sj.row_errors(pop["jc"][:-1][sel], sj.jacobian_reference(refc)),
               "fr": float(np.max(np.abs(pop["fr"][:-1][sel].astype(sy.LD) / refc.fr - 1)))}
        report(f"synthetic_population::prune-AC-load1-mode{mode}-member{p}", **err)
        assert np.all(np.isfinite(pop["berr"][sel])) and pop["berr"][sel].max() <= sy.BERR_MAX
        for k, v in err.items():
            assert v <= b[k], (p, k, v, b[k])


# ----------------------------------------------------------------------------- c. state sequences on one solver
def _same(a, b, keys=("fr", "loss", "w", "flags", "berr", "x", "adj")):
    for k in keys:
        if k in a or k in b:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def _with_load(op, pat, load):
    """The operator ``op`` with the right-hand side of the case loaded on ``load`` (same matrices: make_operator draws
    the values before the load)."""
    import dataclasses
    other = sy.case("AC", load=load)[1]
    assert np.array_equal(other.K, op.K) and np.array_equal(other.M, op.M)
    return dataclasses.replace(op, rhs=other.rhs, _cache={})


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_state_load_moves_between_trees(mode):
    """set_rhs moves the load A -> C (another mask) -> both (nothing pruned) -> A on ONE solver; each sweep equals a
    fresh solver's loaded that way from the start."""
    pat, op, sym, freqs = _case("AC", (0,))
    solver = make_solver(op, sym, prune=True)
    sv = solver[0]
    masks = []
    for load in ((0,), (1,), (0, 1), (0,)):
        opl = _with_load(op, pat, load)
        sv.set_rhs(opl.rhs, opl.beta, opl.mass_sum)
        masks.append(sv.active_fronts().astype(bool))
        got = run_sweep(opl, sym, freqs, mode=mode, solver=solver)
        want = run_sweep(opl, sym, freqs, mode=mode, solver=make_solver(opl, sym, prune=True))
        _same(got, want)
        if len(load) == 1:
            assert np.all(got["x"][:, _unloaded_rows(pat, load)] == 0.0)
            assert sy.schedule_disagreements(sv.schedule_active(), sv.schedule()) == []
    assert not np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0] ^ masks[1], np.ones_like(masks[0]))
    assert masks[2].all() and np.array_equal(masks[3], masks[0])


@pytest.mark.parametrize("refine", [REFINE, REFINE_ADJ], ids=["refine", "refine_adj"])
def test_state_refinement_mode_between(refine):
    """Mode 11 (pruned), then the refinement mode (the full plan), then mode 11: the first and third equal, the second
    equal to a never-pruned solver's, and x on the unloaded rows exactly 0.0 again after the third."""
    load = (1,)
    pat, op, sym, freqs = _case("AC", load)
    solver = make_solver(op, sym, prune=True)
    kw = dict(refine_tol=0.0) if refine == REFINE_ADJ else {}
    first = run_sweep(op, sym, freqs, mode=DEFAULT, solver=solver)
    second = run_sweep(op, sym, freqs, mode=DEFAULT | refine, solver=solver, **kw)
    third = run_sweep(op, sym, freqs, mode=DEFAULT, solver=solver)
    _same(first, third)
    off = run_sweep(op, sym, freqs, mode=DEFAULT | refine, solver=make_solver(op, sym, prune=False), **kw)
    _same(second, off)
    assert np.all(third["x"][:, _unloaded_rows(pat, load)] == 0.0)
    assert np.all(first["flags"] == 0) and np.all(second["flags"] == 0)


def test_state_hessian_sweep_between():
    load = (1,)
    pat, op, sym, freqs = _case("AC", load)
    dcoef = sy.direction(2, op.n_stiff)
    solver = make_solver(op, sym, prune=True)
    first = run_sweep(op, sym, freqs, mode=DEFAULT, solver=solver)
    hs = run_hessian(op, sym, freqs, dcoef, mode=DEFAULT, solver=solver)
    third = run_sweep(op, sym, freqs, mode=DEFAULT, solver=solver)
    _same(first, third)
    assert np.all(third["x"][:, _unloaded_rows(pat, load)] == 0.0)
    _same(hs, run_hessian(op, sym, freqs, dcoef, mode=DEFAULT, solver=make_solver(op, sym, prune=False)),
          ("loss", "w", "h", "flags"))
    assert np.any(hs["h"] != 0)


def test_state_accessor_between_sweeps():
    """Sweep, accessor's adjoint, a sweep with other coefficients, the accessor's adjoint again: the second adjoint is
    the second sweep's (within the reference bound, and not the first); both sweeps equal fresh solvers'."""
    load = (1,)
    pat, op, sym, freqs = _case("AC", load)
    _, (op2,) = sp.members("AC", 1, load=load)              # other coefficients, exact K and beta
    solver = make_solver(op, sym, prune=True)
    sv, K = solver
    first = run_sweep(op, sym, freqs, mode=RAW, solver=solver)
    sv.combine(op2.coef, torch.view_as_real(K))            # K is the solver's operator buffer
    sv.set_rhs(op2.rhs, op2.beta, op2.mass_sum)
    second = run_sweep(op2, sym, freqs, mode=RAW, solver=solver)
    _same(first, run_sweep(op, sym, freqs, mode=RAW, solver=make_solver(op, sym, prune=True)))
    _same(second, run_sweep(op2, sym, freqs, mode=RAW, solver=make_solver(op2, sym, prune=True)))
    assert not np.array_equal(first["adj"], second["adj"])
    bound = _bounds(op2, sym, freqs, "MSE_LOG_AFC")
    err = sy.errors(second["refc"], "MSE_LOG_AFC", second["last"], lam=second["adj"], scale=second["scale"])
    report("synthetic::prune-accessor-second-adjoint", lam=err["lam"], lam_bound=bound["lam"])
    assert err["lam"] <= bound["lam"], (err, bound["lam"])
    assert np.any(second["adj"][:, _unloaded_rows(pat, load)] != 0)


def test_state_functional_changed_after_the_view_exists():
    import dataclasses
    load = (1,)
    pat, op, sym, freqs = _case("AC", load)
    comps = pat.components()
    sup = np.sort(np.concatenate([comps[0][2][[1, 4, 9]], comps[1][2][[3, 30, 77]], comps[1][0][1][:1]])).astype(np.int32)
    a3 = np.random.default_rng(11).standard_normal((3, sup.size))
    op2 = dataclasses.replace(op, sup=sup, a3=a3, _cache={})
    solver = make_solver(op, sym, prune=True)
    sv = solver[0]
    run_sweep(op, sym, freqs, mode=DEFAULT, solver=solver)
    sv.set_functional(op2.sup, op2.a3, op2.ts)
    got = run_sweep(op2, sym, freqs, mode=DEFAULT, solver=solver)
    _same(got, run_sweep(op2, sym, freqs, mode=DEFAULT, solver=make_solver(op2, sym, prune=True)))
    off = run_sweep(op2, sym, freqs, mode=DEFAULT, solver=make_solver(op2, sym, prune=False))
    _same(got, off, ("fr", "loss", "w", "flags", "x"))
    check_sweep("prune-AC-load1-other-support", got, _bounds(op2, sym, freqs, "MSE_LOG_AFC", correct=True), mode=DEFAULT)


def test_state_prune_before_rhs_and_off_again():
    """set_prune(True) before any set_rhs; set_prune(False) after pruned sweeps."""
    load = (1,)
    pat, op, sym, freqs = _case("AC", load)
    sv = _native.Solver(sym, 0, 64)
    sv.set_prune(True)
    assert sv.active_fronts().all()                                           # nothing to prune by yet
    sv.set_stiffness(_t(op.S.T), op.e)
    K = torch.empty(op.pat.nnz, dtype=torch.complex128, device=DEV)
    sv.combine(op.coef, torch.view_as_real(K))
    sv.set_operator(torch.view_as_real(K), _t(op.M))
    sv.set_functional(op.sup, op.a3, op.ts)
    sv.set_rhs(op.rhs, op.beta, op.mass_sum)
    _assert_pruned(sv, sym, pat, load)
    on = run_sweep(op, sym, freqs, mode=DEFAULT, solver=(sv, K))
    _same(on, run_sweep(op, sym, freqs, mode=DEFAULT, solver=make_solver(op, sym, prune=True)))
    sv.set_prune(False)
    assert sv.active_fronts().all()
    never = run_sweep(op, sym, freqs, mode=DEFAULT, solver=make_solver(op, sym))
    _same(run_sweep(op, sym, freqs, mode=DEFAULT, solver=(sv, K)), never)
    _same(on, never, ("fr", "loss", "w", "flags", "x"))


def test_state_graph_replay_past_the_accessor(monkeypatch):
    """PFR_GRAPH=1: the same pruned sweep four times (direct, captured, replayed, replayed), the accessor's completed
    adjoint read between the third and fourth: all four equal the PFR_GRAPH=0 result, three served by the graph."""
    load = (1,)
    pat, op, sym, freqs = _case("AC", load)
    direct = run_sweep(op, sym, freqs, mode=DEFAULT, solver=make_solver(op, sym, prune=True))
    monkeypatch.setenv("PFR_GRAPH", "1")
    with torch.cuda.stream(torch.cuda.Stream(DEV)):          # the default stream cannot be captured
        solver = make_solver(op, sym, prune=True)
        sv = solver[0]
        nf = len(freqs)
        berr = torch.full((nf, 2), float("nan"), dtype=torch.float64, device=DEV)
        sv.set_check(DEFAULT, sy.BERR_MAX, berr)
        ft, rt = _t(freqs), torch.view_as_real(_t(direct["refc"].ref))
        fr = torch.zeros(nf, dtype=torch.float64, device=DEV)
        loss = torch.zeros(1, dtype=torch.float64, device=DEV)
        w = torch.zeros(op.n_stiff, dtype=torch.complex128, device=DEV)
        flags = torch.zeros(nf, dtype=torch.int32, device=DEV)
        q0 = (nf - 1) // 64 * 64
        for call in range(4):
            loss.zero_()
            w.zero_()
            flags.zero_()
            sv.sweep(ft, LOSS_ID["MSE_LOG_AFC"], ref=rt, scale=direct["scale"], fr=fr, loss=loss,
                     w=torch.view_as_real(w), flags=flags)
            torch.cuda.synchronize()
            got = dict(fr=fr.cpu().numpy(), loss=float(loss.cpu()[0]), w=w.cpu().numpy(), berr=berr.cpu().numpy(),
                       flags=flags.cpu().numpy())
            _same(got, direct, ("fr", "loss", "w", "berr", "flags"))
            if call >= 2:
                mu = np.array([sv.debug_solution(1, q - q0) for q in direct["last"]])
                assert np.array_equal(mu, direct["adj"])
                x = np.array([sv.debug_solution(0, q - q0) for q in direct["last"]])
                assert np.array_equal(x, direct["x"])
        assert sv.graph_launches() == 3                       # tests/test_gpu_graph.py: the first call runs directly
