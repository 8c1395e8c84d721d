"""GPU: pfr_hessian_sweep on the synthetic fronts of tests/synthetic.py, against the extended-precision dense
reference (synthetic.hessian_reference, itself checked against finite differences of the reference gradient by
tests/test_synthetic_cpu.py::test_hessian_reference_matches_finite_differences).

The Hessian sweep runs code no loss sweep of tests/test_gpu_synthetic.py reaches: k_tangent_spmv in row and column
form, k_functional_tangent with its four l'' branches, forward_solve with a vector right-hand side (and its
Dirichlet move, launch_dirichlet_rhs(2, ...)), the unpaired adjoint_solve over every front, the two contract_rows +
launch_reduce accumulations into h and the Kdir regrowth.  tests/test_gpu_hessian.py sees it through central
differences of the GPU's own gradient at 2e-5; here every h_ik is compared at

    10 x max(e_model, e_dense, 1e-14)

with e_model / e_dense the errors of the same sequence run in fp64 through the multifrontal model and the unrefined
dense LU (synthetic.hessian_model_errors, first, middle and last frequency), computed at run time and never from
the GPU's output; the loss and w at the loss sweep's bounds.  Besides: the assembled Re(h dcoef^T) is symmetric to
1e-12 of its maximum and within sum_k |d_jk| times the bound of h of the reference's; every flag is 0.

66 frequencies at max_batch 64 (one full chunk and a 2-lane tail), two complex directions, scale 1 / 66.

The unpaired passes' launches (synthetic.unpaired_classes; tests/test_synthetic_cpu.py::
test_unpaired_dispatch_classes) select on the split of the update parts and the wave count only: test_unpaired_knobs.

Measured on an MI355X (h: max_ik |h_ik - ref_ik| / max_ik |ref_ik|; raw mode, MSE_LOG_AFC):

  case             h: e_model / e_dense / GPU        GPU: loss / w
  A   n=97         2.1e-15 / 1.5e-15 / 1.3e-14       2.7e-14 / 9.2e-14
  A4  n=48         2.2e-15 / 1.0e-15 / 6.5e-15       6.3e-14 / 6.8e-14
  A8  n=55         6.8e-15 / 1.1e-15 / 3.5e-15       6.7e-15 / 2.6e-14
  B   n=175        4.9e-15 / 3.0e-15 / 3.4e-15       2.6e-15 / 5.7e-14
  C   n=180        1.2e-15 / 2.3e-15 / 5.4e-15       1.3e-14 / 5.1e-14
  D   n=238        7.5e-16 / 5.8e-16 / 3.0e-15       6.2e-15 / 3.9e-14
  E   n=328        7.4e-15 / 4.8e-15 / 1.5e-14       1.6e-13 / 1.8e-13
  F   n=233        3.9e-15 / 2.2e-15 / 3.9e-15       8.8e-15 / 5.4e-14
  F0  n=26         4.0e-16 / 1.5e-15 / 2.3e-15       6.6e-15 / 4.5e-14
  T   n=206        5.8e-16 / 7.6e-16 / 3.3e-15       4.2e-15 / 5.4e-14
  default mode     A 1.4e-14, E 1.5e-14, T 3.4e-15 (the bounds of the raw mode)
  A   MSE          1.8e-15 / 7.9e-16 / 3.0e-15       1.3e-15 / 2.8e-14
  A   RMSE         1.2e-15 / 5.3e-16 / 1.0e-14       7.9e-16 / 1.2e-13
  A   MSE_AFC      1.3e-15 / 7.9e-16 / 3.0e-15       4.0e-14 / 2.2e-14
  T, n_stiff 18    1.3e-13 / 1.1e-13 / 9.1e-14       T, support outside the root   1.1e-15 / 1.6e-16 / 2.0e-15
  general analysis (A / C / E / T), GPU h            1.2e-14 / 2.8e-15 / 2.3e-14 / 1.5e-15

Over the 42 cases: every bound of h is the floor's 1e-13 except T with 18 matrices (1.3e-12); largest error / bound
0.77 (w of the general analysis of T, 7.7e-14 against 1e-13; for h 0.23, E general), largest asymmetry of
Re(h dcoef^T) 6.4e-15 of its maximum, no flag.  The launch knobs change nothing measurable (A: 1.3e-14 under each).
"""
import numpy as np
import pytest
import torch

import synthetic as sy
from helpers import report
from test_gpu_synthetic import DEFAULT, DEV, LOSS_ID, RAW, _bounds, _t, make_solver, run_sweep

pytestmark = pytest.mark.gpu
FREQS = np.linspace(40.0, 600.0, 66)
_HB = {}


def _h_bound(op, sym, freqs, loss_type, dcoef, symmetric):
    key = (id(op), id(sym), np.asarray(freqs).tobytes(), loss_type, dcoef.tobytes(), symmetric)
    if key not in _HB:
        em, ed = sy.hessian_model_errors(op, sym, freqs, loss_type, dcoef, symmetric=symmetric)
        _HB[key] = (10 * max(em["h"], ed["h"], sy.FLOOR), em["h"], ed["h"])
    return _HB[key]


def run_hessian(op, sym, freqs, dcoef, *, max_batch=64, mode=RAW, loss_type="MSE_LOG_AFC", solver=None, prefill=None):
    """As run_sweep, then pfr_hessian_sweep.  ``prefill`` = (loss, w, h): the outputs' initial values (default 0)."""
    refc = sy.reference(op, freqs)
    nf = len(freqs)
    sv, K = solver or make_solver(op, sym, max_batch)
    sv.set_check(mode, sy.BERR_MAX, None)
    p_loss, p_w, p_h = prefill or (0.0, 0.0, 0.0)
    loss = torch.full((1,), p_loss, dtype=torch.float64, device=DEV)
    w = torch.full((op.n_stiff,), p_w, dtype=torch.complex128, device=DEV)
    h = torch.full((dcoef.shape[0], op.n_stiff), p_h, dtype=torch.complex128, device=DEV)
    flags = torch.zeros(nf, dtype=torch.int32, device=DEV)
    scale = 1.0 / nf
    sv.hessian_sweep(_t(freqs), LOSS_ID[loss_type], torch.view_as_real(_t(refc.ref)), scale, dcoef, loss=loss,
                     w=torch.view_as_real(w), h=torch.view_as_real(h), flags=flags)
    torch.cuda.synchronize()
    return dict(loss=float(loss.cpu()[0]), w=w.cpu().numpy(), h=h.cpu().numpy(), flags=flags.cpu().numpy(),
                K=K.cpu().numpy(), scale=scale, refc=refc, solver=(sv, K))


def check_hessian(name, out, bound, hb, dcoef, loss_type="MSE_LOG_AFC", minus=None):
    """The loss, w, every h_ik and the assembled Re(h dcoef^T) against the reference.  ``minus`` = (loss, w, h): a
    prefill taken off first (in extended precision)."""
    refc = out["refc"]
    every = np.arange(refc.freqs.size)
    loss, w, h = np.longdouble(out["loss"]), out["w"].astype(sy.CLD), out["h"].astype(sy.CLD)
    if minus is not None:
        loss, w, h = loss - np.longdouble(minus[0]), w - sy.CLD(minus[1]), h - sy.CLD(minus[2])
    assert np.array_equal(out["K"], refc.op.K)
    err = sy.errors(refc, loss_type, every, terms=[loss], w=w, scale=out["scale"])
    href = sy.hessian_reference(refc, loss_type, dcoef, out["scale"])
    err["h"] = sy.hessian_error(h, href)
    d = dcoef.astype(sy.CLD)
    H, Href = (h @ d.T).real, (href @ d.T).real
    top = float(np.abs(Href).max())
    asym = float(np.abs(H - H.T).max()) / top
    errH = float(np.abs(H - Href).max())
    boundH = hb[0] * float(np.abs(href).max()) * float(np.abs(dcoef).sum(axis=1).max())
    print(name, f"h={err['h']:.2e}/{hb[0]:.1e} (e_model {hb[1]:.1e}, e_dense {hb[2]:.1e})",
          " ".join(f"{k}={err[k]:.2e}/{bound[k]:.1e}" for k in ("loss", "w")),
          f"H={errH / top:.2e} (bound {boundH / top:.1e}) asym={asym:.1e}")
    report("synthetic_hessian::" + name, h=err["h"], h_bound=hb[0], e_model=hb[1], e_dense=hb[2], loss=err["loss"],
           w=err["w"], ratio=max(err["h"] / hb[0], err["loss"] / bound["loss"], err["w"] / bound["w"]), asym=asym)
    assert np.all(out["flags"] == 0), out["flags"]
    assert err["h"] <= hb[0], (name, "h", err["h"], hb)
    for k in ("loss", "w"):
        assert err[k] <= bound[k], (name, k, err[k], bound[k])
    assert asym <= 1e-12, (name, "asymmetry", asym)
    assert errH <= boundH, (name, "H", errH, boundH)
    return err


def _hessian_case(name, shape, monkeypatch, env=None, mode=RAW, freqs=FREQS, loss_type="MSE_LOG_AFC", n_dir=2,
                  last=True, symmetric=True, **case_kw):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)              # the launch knobs are read in pfr_solver_create
    _, op = sy.case(shape, **case_kw)
    sym = sy.symbolic(shape, symmetric=symmetric, last=last)
    dcoef = sy.direction(n_dir, op.n_stiff)
    bound = _bounds(op, sym, freqs, loss_type, **({} if symmetric else {"symmetric": False}))
    hb = _h_bound(op, sym, freqs, loss_type, dcoef, symmetric)
    out = run_hessian(op, sym, freqs, dcoef, mode=mode, loss_type=loss_type)
    check_hessian(name, out, bound, hb, dcoef, loss_type)


@pytest.mark.parametrize("shape", sorted(sy.SHAPES))
def test_shape(shape, monkeypatch):
    _hessian_case(f"{shape}-raw", shape, monkeypatch)


@pytest.mark.parametrize("shape", ["A", "E", "T"])
def test_default_mode(shape, monkeypatch):
    """Check mode 11: the loss and w are the corrected sweep's, h the uncorrected functional's (include/pfr.h); on
    these systems (cond <= 1e4) the two agree to rounding, so the same reference and bounds hold."""
    _hessian_case(f"{shape}-default", shape, monkeypatch, mode=DEFAULT)


@pytest.mark.parametrize("loss_type", ["MSE", "RMSE", "MSE_AFC"])
def test_losses(loss_type, monkeypatch):
    """Each loss has its own l'' branch in k_functional_tangent."""
    _hessian_case(f"A-{loss_type}", "A", monkeypatch, loss_type=loss_type)


def test_18_stiffness_matrices(monkeypatch):
    _hessian_case("T-n_stiff18", "T", monkeypatch, n_stiff=18)


def test_support_outside_the_root(monkeypatch):
    _hessian_case("T-spread", "T", monkeypatch, last=False, spread=True)


@pytest.mark.parametrize("shape", sorted(sy.GENERAL_SHAPES))
def test_general_analysis(shape, monkeypatch):
    """symmetric = 0 on the patterns WITH Dirichlet nodes: operator-form factorisation by the unsymmetric kernels,
    the U^T / L^T passes on vector right-hand sides."""
    _hessian_case(f"{shape}-general", shape, monkeypatch, symmetric=False)


@pytest.mark.parametrize("nfreq", [1, 63, 64, 65])
def test_batch_edges(nfreq, monkeypatch):
    _hessian_case(f"B-nfreq{nfreq}", "B", monkeypatch, freqs=FREQS[:nfreq])


def test_direction_count_regrowth():
    """n_dir 1, then 5 on one solver: the Kdir block is allocated again, larger (the first stays owned)."""
    _, op = sy.case("A")
    sym = sy.symbolic("A")
    bound = _bounds(op, sym, FREQS, "MSE_LOG_AFC")
    solver = None
    for n_dir in (1, 5):
        dcoef = sy.direction(n_dir, op.n_stiff, seed=n_dir)
        out = run_hessian(op, sym, FREQS, dcoef, solver=solver)
        solver = out["solver"]
        check_hessian(f"A-ndir{n_dir}", out, bound, _h_bound(op, sym, FREQS, "MSE_LOG_AFC", dcoef, True), dcoef)


def test_outputs_are_accumulated_into():
    """loss, w and h prefilled with values of the results' size come back as prefill + result."""
    _, op = sy.case("A")
    sym = sy.symbolic("A")
    dcoef = sy.direction(2, op.n_stiff)
    refc = sy.reference(op, FREQS)
    L = refc.loss("MSE_LOG_AFC")
    href = sy.hessian_reference(refc, "MSE_LOG_AFC", dcoef, 1.0 / FREQS.size)
    pre = (float(0.5 * L["terms"].sum()),           # the loss output is the plain sum of the terms; w and h carry scale
           complex(float(np.abs(L["w"].sum(axis=0)).max()) / FREQS.size * (0.5 - 0.25j)),
           complex(float(np.abs(href).max()) * (0.5 + 0.125j)))
    out = run_hessian(op, sym, FREQS, dcoef, prefill=pre)
    assert abs(out["loss"]) > abs(pre[0]) and np.all(np.abs(out["h"] - pre[2]) > 0)
    check_hessian("A-prefilled", out, _bounds(op, sym, FREQS, "MSE_LOG_AFC"),
                  _h_bound(op, sym, FREQS, "MSE_LOG_AFC", dcoef, True), dcoef, minus=pre)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_loss_sweep_is_unchanged_by_a_hessian_sweep_between(mode):
    """A loss sweep, a Hessian sweep, the same loss sweep again on one solver: the Hessian sweep overwrites G, XA, Y,
    tq, partial and loss_terms, and the second loss sweep's fr, loss and w are bit-identical to the first's."""
    _, op = sy.case("T")
    sym = sy.symbolic("T")
    first = run_sweep(op, sym, FREQS, mode=mode, vectors=False)
    run_hessian(op, sym, FREQS, sy.direction(2, op.n_stiff), mode=mode, solver=first["solver"])
    second = run_sweep(op, sym, FREQS, mode=mode, vectors=False, solver=first["solver"])
    for k in ("fr", "w", "berr", "flags"):
        assert np.array_equal(first[k], second[k]), k
    assert first["loss"] == second["loss"]


# what launch_solve selects on when forward_solve / adjoint_solve call it (synthetic.unpaired_classes): the split
# (target 0: none; 64: 8 / 10 on the bottom levels of A / B, 16 above; 1000000 and the default: 16) and the waves
KNOBS = ([(s, {"PFR_SOLVE_SPLIT": v}, True) for s in ("A", "C") for v in ("0", "1000000")]
         + [(s, {"PFR_SOLVE_SPLIT": "64"}, True) for s in ("A", "B")]
         + [(s, {"PFR_SOLVE_WMAX": "1"}, True) for s in ("A", "B", "C", "T")]
         + [("A", {"PFR_SOLVE_SPLIT": "0"}, False), ("C", {"PFR_SOLVE_WMAX": "1"}, False)])


@pytest.mark.parametrize("shape,env,symmetric", KNOBS,
                         ids=[s + ("" if m else "-general") + "-" + ",".join(f"{k[4:]}={v}" for k, v in e.items())
                              for s, e, m in KNOBS])
def test_unpaired_knobs(shape, env, symmetric, monkeypatch):
    _hessian_case(shape + ("" if symmetric else "-general") + "-" + ",".join(f"{k[4:]}={v}" for k, v in env.items()),
                  shape, monkeypatch, env=env, symmetric=symmetric)
