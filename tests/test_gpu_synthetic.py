"""GPU: the factorisation and solve kernels on synthetic fronts at every dispatch boundary of the launchers
(tests/synthetic.py; tests/test_synthetic_cpu.py proves which branch each shape reaches and lists the test ids).

Every quantity (fr at every frequency, the loss, every partial w_k, the solution vectors x and lam of the last
chunk's lanes, x of every batch item in general mode) is compared with the extended-precision-refined dense
reference; no frequency, partial or batch item is left out.  The bound of each comparison is

    10 x max(e_model, e_dense, 1e-14)

with e_model / e_dense the errors, against the same reference, of the fp64 multifrontal model (tests/mf_model.py)
and of the unrefined fp64 dense solve for the same shape and quantity, maximised over the first, middle and last
frequency; it is computed here from the model at run time, never from the GPU's output.  The kernels perform the
model's operations in another order (fused multiply-adds, 16 x 16 blocked updates, split update parts: sums of at
most 320 terms); a wrong index or a lost update shows as 1e-3 or more on these systems (cond <= 1e4, asserted by
the generator).  Besides: every flag 0, every componentwise backward error <= BERR_MAX = 1e-12.

Measured (default knobs, raw solves = check mode FORWARD | ADJOINT, 130 frequencies, MSE_LOG_AFC; lam, the loss and
w carry what fp64 loses in (log fr - log |ref|)^2 with |ref| = 1.02 fr, ~5e-14):

  shape        e_model: x / lam / fr / loss / w                 GPU: x / lam / fr / loss / w
  A   n=97     1.6e-16 4.8e-14 4.4e-16 1.7e-14 3.0e-14          1.9e-16 6.1e-15 5.4e-15 1.4e-14 4.9e-14
  A4  n=48     1.9e-16 2.2e-13 4.2e-15 1.5e-13 1.1e-13          1.6e-16 8.8e-14 8.1e-15 6.0e-14 3.5e-14
  A8  n=55     1.5e-16 6.0e-14 1.0e-15 1.1e-13 8.4e-14          1.8e-16 3.8e-14 9.9e-15 1.8e-14 1.1e-13
  B   n=175    2.9e-16 9.1e-14 1.9e-15 6.1e-14 6.3e-14          2.0e-16 4.3e-14 3.6e-15 4.0e-15 2.3e-14
  C   n=180    1.9e-16 4.7e-14 3.8e-16 2.9e-14 3.5e-14          1.6e-16 3.9e-14 8.5e-15 6.6e-15 1.1e-13
  D   n=238    3.4e-16 8.3e-15 9.4e-16 3.4e-15 8.6e-15          2.7e-16 9.2e-14 8.3e-15 3.9e-15 3.8e-14
  E   n=328    2.5e-16 6.3e-13 1.3e-14 3.3e-13 1.6e-12          1.6e-16 1.8e-13 9.4e-14 9.6e-14 1.1e-13
  F   n=233    3.6e-16 2.8e-13 4.6e-15 2.4e-13 8.4e-14          4.3e-16 1.7e-13 1.6e-14 6.2e-14 2.9e-14
  F0  n=26     2.3e-16 2.9e-14 4.5e-16 3.9e-14 3.0e-14          2.0e-16 5.8e-15 1.0e-14 2.1e-14 6.1e-14
  T   n=206    1.7e-16 4.6e-14 3.1e-16 3.0e-14 1.6e-14          1.2e-16 4.7e-14 2.3e-15 1.4e-15 1.4e-14
  general mode x, e_model (A / C / E / T): 2.8e-16 / 6.4e-16 / 9.3e-16 / 2.9e-16
  general mode x, GPU (worst of the four forms, A and A^T): 1.9e-14 / 3.4e-15 / 2.9e-15 / 3.3e-15

Over all 128 cases on an MI355X: largest error / bound 0.72 (fr of shape E, 9.4e-14 against 1.3e-13: fr falls to
8.5e-7 of a peak of 0.22 inside the sweep), largest backward error 4.0e-15, no flag; in the default mode (functional
correction on) fr is within 4.3e-15, the loss within 8.5e-15 and w within 3.2e-14 on every shape.

If fr of shape E ever misses its bound: e_model is sampled at three frequencies while the GPU's error is the maximum
over 130, and fr's relative error is largest where fr is smallest (452 Hz).  Measure e_model and e_dense at that
frequency first (synthetic.model_errors on that frequency list) before suspecting a kernel; a wrong kernel misses by
orders of magnitude, not by a factor.
"""
import numpy as np
import pytest
import torch

import synthetic as sy
from helpers import report
from plate_inverse_problem_amd import _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
RAW = _native.PFR_CHECK_FORWARD | _native.PFR_CHECK_ADJOINT                 # fr, x, lam are the raw solves
DEFAULT = RAW | _native.PFR_CHECK_CORRECT                                   # the engine's default mode (11)

_BOUNDS = {}


def _bounds(op, sym, freqs, loss_type, **model_kw):
    """10 x max(e_model, e_dense, 1e-14) per quantity; ``model_kw``: symmetric / refine / correct / scale_corr of
    synthetic.model_errors (the model that matches the sweep's check mode and analysis)."""
    key = (id(op), id(sym), np.asarray(freqs).tobytes(), loss_type, tuple(sorted(model_kw.items())))
    if key not in _BOUNDS:
        _BOUNDS[key] = sy.bounds(*sy.model_errors(op, sym, freqs, loss_type, **model_kw))
    return _BOUNDS[key]


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


LOSS_ID = dict(_native.LOSS_IDS, NONE=_native.LOSS_NONE, COTANGENT=_native.LOSS_COTANGENT)


def make_solver(op, sym, max_batch=64, prune=None):
    """A solver with the operator-form state of ``op`` set, as Problem._Engine sets it.  Returns (solver, K).
    ``prune``: pfr_set_prune with that value (None: never called, the C ABI's default -- off)."""
    sv = _native.Solver(sym, 0, max_batch)
    sv.set_stiffness(_t(op.S.T), op.e)                                        # (nnz, n_stiff)
    K = torch.empty(op.pat.nnz, dtype=torch.complex128, device=DEV)
    sv.combine(op.coef, torch.view_as_real(K))
    sv.set_operator(torch.view_as_real(K), _t(op.M))
    sv.set_rhs(op.rhs, op.beta, op.mass_sum)
    sv.set_functional(op.sup, op.a3, op.ts)
    if prune is not None:
        sv.set_prune(prune)
    return sv, K


def sweep_ref(refc, loss_type):
    """The ``ref`` argument of a sweep: the reference response, or d L / d fr (real part) for PFR_LOSS_COTANGENT."""
    return None if loss_type == "NONE" else refc.cot + 0j if loss_type == "COTANGENT" else refc.ref


def run_sweep(op, sym, freqs, *, max_batch=64, mode=RAW, loss_type="MSE_LOG_AFC", vectors=True, solver=None,
              prefill=None, fresh=False, calls=1, refine_tol=None, vector_lanes=None):
    """One loss sweep through the C ABI, as Problem._Engine drives it.  Returns the device's results on the host.
    ``solver``: (solver, K) of make_solver to sweep on again; ``prefill`` = (loss, w, flag, berr): the outputs'
    initial values (default 0, 0, 0, NaN); ``fresh``: pfr_sweep_fresh; ``calls``: that many sweeps into the same
    outputs; ``vector_lanes``: the lanes of the last chunk whose vectors are read back (default: all)."""
    refc = sy.reference(op, freqs)
    nf, n = len(freqs), op.pat.n
    sv, K = solver or make_solver(op, sym, max_batch)
    p_loss, p_w, p_flag, p_berr = prefill or (0.0, 0.0, 0, float("nan"))
    berr = torch.full((nf, 2), p_berr, dtype=torch.float64, device=DEV)
    sv.set_check(mode, sy.BERR_MAX, berr)
    if refine_tol is not None:
        sv.set_refine_tol(refine_tol)
    fr = torch.zeros(nf, dtype=torch.float64, device=DEV)
    loss = torch.full((1,), p_loss, dtype=torch.float64, device=DEV)
    w = torch.full((op.n_stiff,), p_w, dtype=torch.complex128, device=DEV)
    flags = torch.full((nf,), p_flag, dtype=torch.int32, device=DEV)
    scale = 1.0 / nf
    ref = sweep_ref(refc, loss_type)
    ft = _t(freqs)
    rt = None if ref is None else torch.view_as_real(_t(ref))
    for _ in range(calls):
        sv.sweep(ft, LOSS_ID[loss_type], ref=rt, scale=scale, fr=fr, loss=loss, w=torch.view_as_real(w), flags=flags,
                 fresh=fresh)
    torch.cuda.synchronize()
    out = dict(fr=fr.cpu().numpy(), loss=float(loss.cpu()[0]), w=w.cpu().numpy(), berr=berr.cpu().numpy(),
               flags=flags.cpu().numpy(), K=K.cpu().numpy(), scale=scale, refc=refc, solver=(sv, K))
    if vectors:
        q0 = (nf - 1) // sv.max_batch * sv.max_batch                          # the last chunk's lanes
        out["last"] = np.arange(q0, nf) if vector_lanes is None else q0 + np.asarray(vector_lanes)
        out["x"] = np.array([sv.debug_solution(0, q - q0) for q in out["last"]])
        out["adj"] = np.array([sv.debug_solution(1, q - q0) for q in out["last"]])
    return out


def check_sweep(name, out, bound, loss_type="MSE_LOG_AFC", mode=RAW, fr_sel=None, clean=True, only=None):
    """Every comparison of one sweep against the reference; the measured errors go to $PFR_TEST_REPORT.
    ``loss_type`` "NONE": fr and x only (no adjoint unless the mode has PFR_CHECK_CORRECT); ``clean`` = False: the
    caller asserts the flags and backward errors itself (the weak-pivot cases, where they must be set); ``only``: the
    quantities asserted (default: all; the others are still measured and reported)."""
    refc = out["refc"]
    op = refc.op
    every = np.arange(refc.freqs.size)
    reverse = loss_type != "NONE"
    lt = loss_type if reverse else "MSE_LOG_AFC"
    assert np.array_equal(out["K"], op.K)                                     # pfr_combine: exact by construction
    err = sy.errors(refc, lt, every, terms=[out["loss"]], w=out["w"], scale=out["scale"]) if reverse else {}
    sel = every if fr_sel is None else fr_sel
    err["fr"] = sy.errors(refc, lt, sel, fr=out["fr"][sel])["fr"]
    if "x" in out:
        # under PFR_CHECK_CORRECT the vector is mu, the adjoint of fr
        lam = out["adj"] if reverse and not mode & _native.PFR_CHECK_CORRECT else None
        err.update(sy.errors(refc, lt, out["last"], x=out["x"], lam=lam, scale=out["scale"]))
    be = out["berr"] if reverse or mode & _native.PFR_CHECK_CORRECT else out["berr"][:, :1]   # no adjoint solve
    print(name, " ".join(f"{k}={v:.2e}/{bound[k]:.1e}" for k, v in sorted(err.items())),
          f"berr={np.nanmax(be):.1e}")
    report("synthetic::" + name, berr=float(np.nanmax(be)), **err)
    if clean:
        assert np.all(out["flags"] == 0), out["flags"]
        assert np.all(np.isfinite(be)) and be.max() <= sy.BERR_MAX, be.max()
    for k, v in err.items():
        assert v <= bound[k] or (only is not None and k not in only), (name, k, v, bound[k])
    return err


def _sweep_case(name, shape, monkeypatch, env=None, mode=RAW, freqs=sy.FREQS, loss_type="MSE_LOG_AFC", max_batch=64,
                last=True, fr_sel=None, vectors=True, symmetric=True, model_kw=None, **case_kw):
    """``symmetric`` = False: a general analysis of the same pattern (the unsymmetric kernels on operator data);
    ``model_kw``: the model the bounds come from (synthetic.model_errors: refine / correct / scale_corr)."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)              # the launch knobs are read in pfr_solver_create
    _, op = sy.case(shape, **case_kw)
    sym = sy.symbolic(shape, symmetric=symmetric, last=last)
    kw = dict(model_kw or {}, **({} if symmetric else {"symmetric": False}))
    bound = _bounds(op, sym, freqs, loss_type, **kw)
    out = run_sweep(op, sym, freqs, max_batch=max_batch, mode=mode, loss_type=loss_type, vectors=vectors)
    check_sweep(name, out, bound, loss_type, mode, fr_sel)
    return out, bound


# ----------------------------------------------------------------------------- every shape, raw and default mode
@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("shape", sorted(sy.SHAPES))
def test_shape(shape, mode, monkeypatch):
    _sweep_case(f"{shape}-mode{mode}", shape, monkeypatch, mode=mode)


# ----------------------------------------------------------------------------- launch knobs on the shapes that reach them
_RL = [{"PFR_US2_RL": "0"}, {"PFR_LS_RL": "0"}, {"PFR_US2_RL": "0", "PFR_LS_RL": "0"}, {"PFR_US2_NAR": "0"},
       {"PFR_US2_NAR": "1000000000"}]
_WIDE = {"PFR_US2_NAR": "0", "PFR_SOLVE_SPLIT": "0"}     # wide, unsplit launches: where the tiny forms are chosen
KNOBS = (
    [(s, e) for s in ("C", "B", "F") for e in _RL]
    + [(s, {"PFR_FAC_LDS": v}) for s in ("A", "B") for v in ("0", "1")]
    + [(s, {"PFR_SCHUR_BLK_MIN": v}) for s in ("A", "E") for v in ("0", "4")]
    # the fused bottom level exists on F0 only; on A and T (the issue's cases) the knob changes nothing
    + [(s, {"PFR_FRONT0": "0"}) for s in ("A", "T", "F0")]
    + [("A", {"PFR_US2_TINY": v}) for v in ("0", "4")]
    + [(s, {"PFR_SOLVE_SPLIT": v}) for s in ("C", "D") for v in ("0", "1000000")]
    + [(s, dict(_WIDE, **e)) for s in ("A4", "A8") for e in ({}, {"PFR_US2_TINY": "0"}, {"PFR_US2_TINY": "4"})]
)


@pytest.mark.parametrize("shape,env", KNOBS, ids=[s + "-" + ",".join(f"{k[4:]}={v}" for k, v in e.items())
                                                  for s, e in KNOBS])
def test_knob(shape, env, monkeypatch):
    """Each variant against the reference (not against another variant: the operation order differs)."""
    _sweep_case(shape + "-" + ",".join(f"{k[4:]}={v}" for k, v in env.items()), shape, monkeypatch, env=env)


# the size-based wave counts: under the default PFR_SOLVE_WMAX = 8 every solve launch of these shapes is raised to 8
# waves (csrc/plan.hpp solve_waves; fewer than 4,096 workgroups); with 1 the level kernels run at waves_for(maxf):
# F0 1, A 3 / 2, T 4 / 3, B 5 / 3, C 8 / 6, D 8 / 7 (tests/test_synthetic_cpu.py::test_solve_launch_waves)
_W1 = [{}, {"PFR_US2_RL": "0", "PFR_LS_RL": "0"}, {"PFR_US2_NAR": "0"}, {"PFR_FAC_WMAX": "1"}]
WAVES = [(s, dict({"PFR_SOLVE_WMAX": "1"}, **e)) for s in ("F0", "A", "T", "B", "C", "D") for e in _W1]


@pytest.mark.parametrize("shape,env", WAVES, ids=[s + "-" + ",".join(f"{k[4:]}={v}" for k, v in e.items())
                                                  for s, e in WAVES])
def test_solve_waves(shape, env, monkeypatch):
    _sweep_case(shape + "-" + ",".join(f"{k[4:]}={v}" for k, v in env.items()), shape, monkeypatch, env=env)


@pytest.mark.parametrize("shape", ["A", "C", "F", "T", "F0"])
def test_solver_schedule(shape):
    """The live schedule of a solver with its right-hand side and functional set (nothing is launched) against the
    analysis' schedule with every front reached: the reach-independent passes equal, the reach-dependent records
    over at most the level's fronts and never empty at the root; on T the right-hand side (two leaf cliques and one
    Dirichlet node) reaches only part of the bottom of its 5-level tree."""
    _, op = sy.case(shape)
    sym = sy.symbolic(shape)
    sv, _ = make_solver(op, sym)
    live, full = sv.schedule(), sym.schedule(64)
    for name in ("factor", "pair", "solve_all"):
        assert np.array_equal(live[name], full[name]), name
    nf = full["solve_all"]["nf"]
    assert nf.size == sym.stats()["n_levels"] and np.all(nf > 0)
    for counts in (live["chain"]["nf0"], live["chain"]["nf1"], live["solve_reach0"]["nf"], live["solve_reach1"]["nf"]):
        assert np.all(counts >= 0) and np.all(counts <= nf) and counts[-1] > 0
    chain = live["chain"]
    assert np.array_equal(chain["nf0"], live["solve_reach0"]["nf"])
    assert np.array_equal(chain["nf1"], live["solve_reach1"]["nf"])
    assert np.array_equal(chain["nmax"], np.maximum(chain["nf0"], chain["nf1"]))
    if shape == "T":
        assert nf.size == 5 and np.any(chain["nf0"] < nf)


# ----------------------------------------------------------------------------- once, not per shape
@pytest.mark.parametrize("nfreq", [1, 63, 64, 65])
def test_batch_edges(nfreq, monkeypatch):
    _sweep_case(f"B-nfreq{nfreq}", "B", monkeypatch, freqs=sy.FREQS[:nfreq])


@pytest.mark.parametrize("ls_rl", ["1", "0"])
def test_chunk_of_2048_lanes(ls_rl, monkeypatch):
    """One 2,048-lane chunk (32 frequency groups per front: the wide launches); fr at 64 evenly spaced frequencies,
    the loss and w of the whole sweep."""
    freqs = np.linspace(40.0, 600.0, 2048)
    _sweep_case(f"A-2048-LS_RL={ls_rl}", "A", monkeypatch, env={"PFR_LS_RL": ls_rl}, freqs=freqs, max_batch=2048,
                fr_sel=np.arange(0, 2048, 32), vectors=False)


@pytest.mark.parametrize("loss_type", ["MSE", "RMSE", "MSE_AFC"])
def test_losses(loss_type, monkeypatch):
    _sweep_case(f"A-{loss_type}", "A", monkeypatch, loss_type=loss_type)
    _sweep_case(f"A-{loss_type}-default", "A", monkeypatch, loss_type=loss_type, mode=DEFAULT)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_18_stiffness_matrices(mode, monkeypatch):
    _sweep_case(f"T-n_stiff18-mode{mode}", "T", monkeypatch, mode=mode, n_stiff=18)


@pytest.mark.parametrize("fn_dot", ["1", "0"])
def test_support_outside_the_root(fn_dot, monkeypatch):
    """Analysis without `last`, the functional's support spread over two leaf cliques and the border."""
    _sweep_case(f"T-spread-FN_DOT={fn_dot}", "T", monkeypatch, env={"PFR_FN_DOT": fn_dot}, last=False, spread=True)


def test_dense_rhs(monkeypatch):
    _sweep_case("B-dense-rhs", "B", monkeypatch, dense_rhs=True)


# ----------------------------------------------------------------------------- general mode: pfr_solve, pfr_solve_multi
def _general(shape):
    gc = sy.general_case(shape)
    sv = _native.Solver(gc.sym, 0, 64)
    return gc, sv, gc.pat.n, gc.pat.nnz, gc.data.shape[0]


def _check_general(name, gc, x, pairs, trans, berr, flags, bound):
    """x[i] against the refined dense solve of A_q (A_q^T) x = b for pairs[i] = (q, b)."""
    err = max(sy.rel(x[i], gc.solve(q, b, trans)[0]) for i, (q, b) in enumerate(pairs))
    be = berr[:, int(trans)]
    print(name, f"x={err:.2e}/{bound[0]:.1e} (e_model {bound[1]:.1e}, e_dense {bound[2]:.1e}) berr={be.max():.1e}")
    report("synthetic::" + name, x=err, berr=float(be.max()))
    assert np.all(flags == 0) and np.all(np.isfinite(be)) and be.max() <= sy.BERR_MAX
    assert err <= bound[0], (name, err, bound)


@pytest.mark.parametrize("form", ["batch", "data_stride0", "b_stride0"])
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("shape", sorted(sy.GENERAL_SHAPES))
def test_general_solve(shape, transpose, form):
    """Batch 65 at max_batch 64 (one chunk and a 1-lane tail), unsymmetric values, A and A^T; one matrix for 65
    right-hand sides; one right-hand side for 65 matrices."""
    gc, sv, n, nnz, B = _general(shape)
    data, b = gc.data, gc.b
    if form == "data_stride0":
        dt, ds, bt, bs = _t(data[0]), 0, _t(b), n
        pairs = [(0, b[q]) for q in range(B)]
        items = ((0, 0), (0, B // 2), (0, B - 1))
    elif form == "b_stride0":
        dt, ds, bt, bs = _t(data), nnz, _t(b[0]), 0
        pairs = [(q, b[0]) for q in range(B)]
        items = ((0, 0), (B // 2, 0), (B - 1, 0))
    else:
        dt, ds, bt, bs = _t(data), nnz, _t(b), n
        pairs = [(q, b[q]) for q in range(B)]
        items = ((0, 0), (B // 2, B // 2), (B - 1, B - 1))
    berr = torch.full((B, 2), float("nan"), dtype=torch.float64, device=DEV)
    sv.set_check(RAW, sy.BERR_MAX, berr)
    x = torch.zeros((B, n), dtype=torch.complex128, device=DEV)
    flags = torch.zeros(B, dtype=torch.int32, device=DEV)
    sv.solve(torch.view_as_real(dt), ds, torch.view_as_real(bt), bs, torch.view_as_real(x), transpose, B, flags)
    torch.cuda.synchronize()
    _check_general(f"general-{shape}-{form}-t{transpose}", gc, x.cpu().numpy(), pairs, transpose,
                   berr.cpu().numpy(), flags.cpu().numpy(), gc.bound(transpose, items))


@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("shape", sorted(sy.GENERAL_SHAPES))
def test_general_solve_multi(shape, transpose):
    """Three right-hand sides per matrix on one factorisation."""
    gc, sv, n, nnz, B = _general(shape)
    berr = torch.full((B, 2), float("nan"), dtype=torch.float64, device=DEV)
    sv.set_check(RAW, sy.BERR_MAX, berr)     # backward errors of the first right-hand side, flags of all three
    x = torch.zeros((3, B, n), dtype=torch.complex128, device=DEV)
    flags = torch.zeros(B, dtype=torch.int32, device=DEV)
    sv.solve_multi(torch.view_as_real(_t(gc.data)), nnz, torch.view_as_real(_t(gc.b3)), n, B * n,
                   torch.view_as_real(x), B * n, transpose, B, 3, flags)
    torch.cuda.synchronize()
    xs = x.cpu().numpy()
    bound = gc.bound(transpose, ((0, 0), (B // 2, B // 2), (B - 1, B - 1)))
    err = max(sy.rel(xs[r, q], gc.solve(q, gc.b3[r, q], transpose)[0]) for r in range(3) for q in range(B))
    be = berr.cpu().numpy()[:, int(transpose)]
    print(f"general-{shape}-multi-t{transpose} x={err:.2e}/{bound[0]:.1e} berr={be.max():.1e}")
    report(f"synthetic::general-{shape}-multi-t{transpose}", x=err, berr=float(be.max()))
    assert np.all(flags.cpu().numpy() == 0)
    assert np.all(np.isfinite(be)) and be.max() <= sy.BERR_MAX
    assert err <= bound[0], (err, bound)
