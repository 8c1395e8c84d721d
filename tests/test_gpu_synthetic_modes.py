"""GPU: the sweep paths tests/test_gpu_synthetic.py does not reach, on the same synthetic fronts and against the same
extended-precision dense reference (tests/synthetic.py), each bound 10 x max(e_model, e_dense, 1e-14) computed at
run time from the fp64 multifrontal model and the unrefined dense solve, never from the GPU's output.

Paths (csrc/api.cpp sweep_launches; `paired = sym && adj && !refine`):
  PFR_LOSS_NONE, raw mode        the unpaired forward_solve with a full top-down pass (x, fr)
  PFR_LOSS_NONE, default mode    the fr adjoint and the functional correction without a loss
  PFR_LOSS_COTANGENT             what Problem's autograd backward calls: d L / d fr supplied, the loss untouched
  check modes 7 and 15           PFR_CHECK_REFINE: unpaired, and both refinement solves run
  a general analysis             symmetric = 0 on operator data: factor_all mode 0 with the unsymmetric kernels, the
                                 U^T / L^T passes (shapes A, C, E, T with their Dirichlet nodes)
  PFR_CONTRACT_WALK / PFR_SCALE_CORR = 0   k_contract_eg with and without the cotangent scales, k_correct_finish
                                 with a real m_q
  pfr_sweep twice / pfr_sweep_fresh        accumulated into, and initialised by the sweep

66 frequencies at max_batch 64 (one full chunk and a 2-lane tail) unless stated.

Weak pivots (synthetic.make_operator(weak_bits = WEAK_BITS[shape], 24 or 28): one diagonal entry per leaf clique times
2^-24 / 2^-28; cond <= 1e4 kept, the static-order elimination grows by about that factor.  On the well-conditioned
unit-growth systems above the unrefined solves already sit at 2e-16, so a refinement step or a functional correction
that adds the wrong thing cannot be seen; here the unrefined model is >= 10 x (measured >= 26 x) above the refined
bounds and above BERR_MAX
(tests/test_synthetic_cpu.py::test_weak_variant_conditions asserts it), so:
  mode 3     x, lam, fr at the UNREFINED model's bounds; each frequency's flag bits set exactly when its backward error
             is above the tolerance; the device's backward errors within a factor 2 of the host's for the returned
             vectors; the model's sampled frequencies flagged.  Finite, merely inaccurate solves -- no fault.
  mode 7     everything at the REFINED model's bounds, every backward error <= BERR_MAX, no flag
  mode 11    fr (every frequency), the loss and w at the bounds of the model that corrects as the kernels do
             (synthetic.model_errors(correct=True): fr + Re(mu^T r), the cotangent m_q = dl fr / (mu^T b - mu^T r) of
             k_correct_finish's solve-error scale mirrored), x still at the unrefined level
  mode 15    refinement and correction together, at that model's bounds
  mode 27    the selective adjoint refinement (k_select_groups: the largest indicators above the tolerance, at most
             REFINE_CAP = 4 groups -- the code does what its comment says): 512 frequencies in one chunk of 8 groups

Measured on an MI355X:

  Weak cases (x of the last chunk's lanes, fr over every frequency, the largest backward error of the sweep):
                    mode 3: x / fr / berr            mode 7: x / fr / berr             mode 11: fr / bound  mode 15: fr
  A   symmetric     1.2e-11 2.8e-09 5.5e-09          9.1e-17 3.5e-15 9.9e-16           2.3e-15 / 1.1e-13      2.8e-15
  A   general       2.1e-11 4.9e-09 9.4e-09          9.1e-17 3.5e-15 9.9e-16           2.5e-15 / 1.1e-13      2.8e-15
  C   symmetric     2.0e-10 1.1e-07 3.1e-08          1.1e-16 2.6e-15 1.3e-15           7.4e-15 / 1.5e-13      3.7e-16
  C   general       4.9e-10 8.3e-08 4.8e-08          1.1e-16 2.9e-15 1.6e-15           1.3e-14 / 1.4e-13      3.7e-16
  E   symmetric     3.3e-11 2.9e-10 8.2e-10          3.0e-16 2.0e-15 2.0e-15           1.9e-15 / 1.1e-13      2.2e-15
  E   general       4.2e-11 6.1e-10 1.4e-09          3.0e-16 2.0e-15 2.0e-15           2.4e-15 / 1.1e-13      2.2e-15
  T   symmetric     5.4e-10 9.3e-08 4.8e-08          1.1e-16 2.1e-15 6.8e-15           1.0e-14 / 1.0e-13      7.4e-16
  T   general       6.5e-10 5.2e-08 1.1e-07          1.1e-16 4.2e-15 5.3e-15           4.2e-15 / 1.4e-13      7.4e-16
  F0  symmetric     8.0e-11 3.5e-08 1.0e-08          1.7e-16 1.7e-15 3.5e-16           7.9e-16 / 1.0e-13      1.3e-15
  F0  general       8.9e-11 4.6e-08 7.8e-09          1.7e-16 1.5e-15 3.5e-16           1.1e-15 / 1.0e-13      1.3e-15
  Mode 3 flags every frequency of every weak sweep (smallest backward error 4.8e-12, shape E).  Mode 27, tolerance
  0: the mu of groups 1-4 at 1.1e-16 ... 2.8e-16 (bound 1e-13), of groups 0, 5, 6, 7 at 3.0e-11 ... 7.4e-11;
  tolerance 1: all eight at 3.0e-11 ... 4.3e-09; fr within 3.2e-15 either way.

Over the 97 cases: largest error / bound 0.77 (w of the general analysis of T in raw mode, 7.7e-14 against 1e-13);
among the weak cases 0.59 (the loss in mode 3, shape C); largest backward error of the cases that must be clean
6.8e-15.

History of the weak variant: with 2^-30 on every shape the gaps are >= 345 x, but what one refinement step leaves is
second order in the unrefined error and no longer below the floor -- shape F0 then has a refined backward error of
9.6e-13, and at 2^-28 its refined w is at 1.07 x the bound on the general analysis.  Hence the smallest exponent per
shape at which the gaps hold (synthetic.WEAK_BITS).  With three sampled frequencies for the model, fr over 130
frequencies misses the unrefined bound on every shape by 3 ... 100 x (the weak pivots' growth peaks at frequencies
of their own); the model over every frequency is what the device's maximum over every frequency compares with.
"""
import numpy as np
import pytest

import synthetic as sy
from helpers import report
from plate_inverse_problem_amd import _native
from test_gpu_synthetic import DEFAULT, RAW, _bounds, _sweep_case, check_sweep, run_sweep

pytestmark = pytest.mark.gpu
FREQS = np.linspace(40.0, 600.0, 66)
REFINE = _native.PFR_CHECK_REFINE
FWD_BIT, ADJ_BIT = _native.PFR_FLAG_BACKWARD_ERROR, _native.PFR_FLAG_BACKWARD_ERROR_ADJ
MODES = {"raw": RAW, "default": DEFAULT}


# ----------------------------------------------------------------------------- sweep paths not yet reached
@pytest.mark.parametrize("shape", sorted(sy.SHAPES))
def test_loss_none_raw(shape, monkeypatch):
    out, _ = _sweep_case(f"{shape}-none-raw", shape, monkeypatch, freqs=FREQS, loss_type="NONE")
    assert out["loss"] == 0.0 and not out["w"].any()         # no reverse pass: nothing accumulated


@pytest.mark.parametrize("shape", ["A", "E", "T"])
def test_loss_none_default(shape, monkeypatch):
    _sweep_case(f"{shape}-none-default", shape, monkeypatch, freqs=FREQS, loss_type="NONE", mode=DEFAULT)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", ["A", "T"])
def test_loss_cotangent(shape, mode):
    """ref.re = d L / d fr (a fixed seed, both signs): w = scale sum_q partials(lam_q, x_q) with A^T lam_q =
    ref_q d fr / d x; the loss output keeps its value."""
    _, op = sy.case(shape)
    sym = sy.symbolic(shape)
    out = run_sweep(op, sym, FREQS, mode=MODES[mode], loss_type="COTANGENT", prefill=(0.375, 0.0, 0, float("nan")))
    assert out["loss"] == 0.375
    out["loss"] = 0.0
    check_sweep(f"{shape}-cotangent-{mode}", out, _bounds(op, sym, FREQS, "COTANGENT"), "COTANGENT", MODES[mode])


@pytest.mark.parametrize("mode", [RAW | REFINE, DEFAULT | REFINE], ids=["mode7", "mode15"])
@pytest.mark.parametrize("shape", sorted(sy.SHAPES))
def test_refined_modes(shape, mode, monkeypatch):
    _sweep_case(f"{shape}-mode{mode}", shape, monkeypatch, freqs=FREQS, mode=mode)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", sorted(sy.GENERAL_SHAPES))
def test_general_analysis(shape, mode, monkeypatch):
    _sweep_case(f"{shape}-general-{mode}", shape, monkeypatch, freqs=FREQS, mode=MODES[mode], symmetric=False)


_CW = [{"PFR_CONTRACT_WALK": "0"}, {"PFR_SCALE_CORR": "0"}, {"PFR_CONTRACT_WALK": "0", "PFR_SCALE_CORR": "0"}]


@pytest.mark.parametrize("env", _CW, ids=[",".join(f"{k[4:]}={v}" for k, v in e.items()) for e in _CW])
@pytest.mark.parametrize("shape,n_stiff", [("A", 12), ("T", 18)])
def test_contraction_forms(shape, n_stiff, env, monkeypatch):
    _sweep_case(f"{shape}-n_stiff{n_stiff}-" + ",".join(f"{k[4:]}={v}" for k, v in env.items()), shape, monkeypatch,
                env=env, freqs=FREQS, mode=DEFAULT, n_stiff=n_stiff)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_sweep_accumulates_and_fresh_initialises(mode):
    """pfr_sweep twice into the same loss / w / flags: twice one call's (halved exactly, then against the reference).
    pfr_sweep_fresh onto prefilled outputs: the prefill is gone, the flags cleared and the backward errors written."""
    _, op = sy.case("B")
    sym = sy.symbolic("B")
    bound = _bounds(op, sym, FREQS, "MSE_LOG_AFC")
    out = run_sweep(op, sym, FREQS, mode=MODES[mode], calls=2)
    out["loss"], out["w"] = out["loss"] / 2, out["w"] / 2
    check_sweep(f"B-twice-{mode}", out, bound, mode=MODES[mode])
    out = run_sweep(op, sym, FREQS, mode=MODES[mode], fresh=True, prefill=(3.0, 2.0 - 1.0j, 8, 7.0))
    check_sweep(f"B-fresh-{mode}", out, bound, mode=MODES[mode])


# ----------------------------------------------------------------------------- weak pivots
WEAK = tuple(sy.WEAK_BITS)                   # tests/test_synthetic_cpu.py WEAK_SHAPES
ANALYSES = {"symmetric": True, "general": False}


def _weak(shape, symmetric):
    """(operator, analysis, frequencies, model options) of a weak case.  The bounds take the model over EVERY
    frequency of the sweep (synthetic.model_errors(every=True)): the weak systems' errors peak at frequencies of
    their own (synthetic.weak_freqs: the 130 FREQS, every other one on shape E)."""
    _, op = sy.case(shape, weak_bits=sy.WEAK_BITS[shape])
    kw = dict(every=True, **({} if symmetric else {"symmetric": False}))
    return op, sy.symbolic(shape, symmetric=symmetric), sy.weak_freqs(shape), kw


def _flags_follow_berr(out):
    """Each frequency's flag bit set exactly when its backward error is above the tolerance or not finite."""
    be, fl = out["berr"], out["flags"]
    for col, bit in ((0, FWD_BIT), (1, ADJ_BIT)):
        want = ~(be[:, col] <= sy.BERR_MAX)
        assert np.array_equal((fl & bit) != 0, want), (col, np.nonzero(((fl & bit) != 0) != want)[0])
    assert not np.any(fl & _native.PFR_FLAG_BAD_PIVOT) and not np.any(fl & ~(1 | FWD_BIT | ADJ_BIT))


def _device_berr_matches_host(out, loss_type="MSE_LOG_AFC"):
    """tests/test_gpu_check.py's criterion on the last chunk's lanes: the device's backward errors within a factor 2
    of the host's, computed from the returned vectors (the adjoint's seed from the returned x)."""
    refc = out["refc"]
    op = refc.op
    for i, q in enumerate(out["last"]):
        x, lam = out["x"][i], out["adj"][i]
        host = sy.berr_of(refc.mats[q], x, op.b_ld(refc.freqs[q]))
        assert out["berr"][q, 0] == pytest.approx(host, rel=0.5, abs=1e-15), (q, out["berr"][q, 0], host)
        g = sy.adjoint_seed(op, x, out["scale"] * sy.loss64(sy.fr_of(op, x)[0], refc.ref[q], loss_type)[1])
        host = sy.berr_of(refc.mats[q], lam, g, tr=True)
        assert out["berr"][q, 1] == pytest.approx(host, rel=0.5, abs=1e-15), (q, out["berr"][q, 1], host)


@pytest.mark.parametrize("analysis", sorted(ANALYSES))
@pytest.mark.parametrize("shape", WEAK)
def test_weak_raw(shape, analysis):
    op, sym, freqs, kw = _weak(shape, ANALYSES[analysis])
    out = run_sweep(op, sym, freqs, mode=RAW)
    err = check_sweep(f"weak-{shape}-{analysis}-mode3", out, _bounds(op, sym, freqs, "MSE_LOG_AFC", **kw), clean=False)
    assert np.all(np.isfinite(out["berr"])) and np.all(np.isfinite(out["fr"]))
    _flags_follow_berr(out)
    _device_berr_matches_host(out)
    sampled = sy.three(freqs)
    assert np.all(out["flags"][sampled] & FWD_BIT) and np.all(out["flags"][sampled] & ADJ_BIT), out["flags"][sampled]
    report(f"synthetic::weak-{shape}-{analysis}-mode3-flags", flagged=int(np.count_nonzero(out["flags"])),
           berr_min=float(out["berr"].min()), berr_max=float(out["berr"].max()), x=err["x"])


@pytest.mark.parametrize("analysis", sorted(ANALYSES))
@pytest.mark.parametrize("shape", WEAK)
def test_weak_refined(shape, analysis):
    """Mode 7: the test with teeth for the refinement kernels (k_residual<..., CMP> into G / Y2, the vector
    right-hand-side solves, k_axpy_vec)."""
    op, sym, freqs, kw = _weak(shape, ANALYSES[analysis])
    out = run_sweep(op, sym, freqs, mode=RAW | REFINE)
    check_sweep(f"weak-{shape}-{analysis}-mode7", out, _bounds(op, sym, freqs, "MSE_LOG_AFC", refine=True, **kw),
                mode=RAW | REFINE)


@pytest.mark.parametrize("analysis", sorted(ANALYSES))
@pytest.mark.parametrize("shape", WEAK)
def test_weak_corrected(shape, analysis):
    """Mode 11: fr + Re(mu^T r) at every frequency, the loss and w at the correcting model's bounds (the cotangent
    scale of k_correct_finish mirrored by the model); x stays unrefined, so its checks flag it.  Then mode 15."""
    op, sym, freqs, kw = _weak(shape, ANALYSES[analysis])
    out = run_sweep(op, sym, freqs, mode=DEFAULT)
    bound = _bounds(op, sym, freqs, "MSE_LOG_AFC", correct=True, **kw)
    raw = _bounds(op, sym, freqs, "MSE_LOG_AFC", **kw)
    assert bound["x"] == raw["x"] and raw["fr"] >= 10 * bound["fr"]       # the model's x is the unrefined one
    check_sweep(f"weak-{shape}-{analysis}-mode11", out, bound, mode=DEFAULT, clean=False)
    _flags_follow_berr(out)
    out = run_sweep(op, sym, freqs, mode=DEFAULT | REFINE)
    check_sweep(f"weak-{shape}-{analysis}-mode15", out,
                _bounds(op, sym, freqs, "MSE_LOG_AFC", refine=True, correct=True, **kw), mode=DEFAULT | REFINE)


@pytest.mark.parametrize("tol,n_refined", [(0.0, 4), (1.0, 0)], ids=["tol0", "tol1"])
def test_weak_selective_adjoint_refinement(tol, n_refined):
    """Mode 27 (PFR_CHECK_REFINE_ADJ) on shape A, 512 frequencies in one chunk of 8 groups.  For lanes 0 and 63 of
    every group mu_ref = refined A^-T d fr / d x at the GPU's own x against the GPU's mu: with tolerance 0 exactly
    REFINE_CAP = 4 groups are at the refined bound and the others at least 10 x above it, both lanes of a group
    agreeing; with tolerance 1 none is refined.  fr at all 512 frequencies within the corrected bound either way."""
    mode = DEFAULT | _native.PFR_CHECK_REFINE_ADJ
    freqs = np.linspace(40.0, 600.0, 512)
    op, sym, _, kw = _weak("A", True)
    lanes = np.array([64 * g + l for g in range(8) for l in (0, 63)])
    out = run_sweep(op, sym, freqs, max_batch=512, mode=mode, refine_tol=tol, vector_lanes=lanes)
    refc = out["refc"]
    # per sampled frequency: the model's unrefined and once-refined mu and the dense solve, against the refined one
    e_raw, e_ref, e_dense = sy.mu_model_errors(op, sym, freqs, lanes)
    bound = 10 * np.maximum(np.maximum(e_ref, e_dense), sy.FLOOR)
    assert np.all(e_raw >= 10 * bound), (e_raw, bound)        # the model's gap: an unrefined mu is told apart
    err = []
    for i, q in enumerate(lanes):
        x = out["x"][i].astype(sy.CLD)
        mu_ref = sy.refined_solve(refc.mats[q], sy.adjoint_seed(op, x, sy.LD(1)), refc.lus[q], trans=True)[0]
        err.append(sy.rel(out["adj"][i], mu_ref))
    err, bound = np.array(err).reshape(8, 2), bound.reshape(8, 2)
    print(f"weak-A-mode27-tol{tol:g} mu error / bound per group (lanes 0, 63):",
          " ".join(f"{a:.1e}/{c:.0e},{b:.1e}/{d:.0e}" for (a, b), (c, d) in zip(err, bound)))
    refined = err <= bound
    report(f"synthetic::weak-A-mode27-tol{tol:g}", mu_refined=float(err[refined].max()) if refined.any() else 0.0,
           mu_unrefined=float(err[~refined].min()) if (~refined).any() else 0.0, bound=float(bound.max()))
    assert np.array_equal(refined[:, 0], refined[:, 1]) and refined[:, 0].sum() == n_refined, (err, bound)
    assert np.all(err[~refined] >= 10 * bound[~refined]), (err, bound)
    check_sweep(f"weak-A-mode27-tol{tol:g}", {k: v for k, v in out.items() if k not in ("x", "adj", "last")},
                _bounds(op, sym, freqs, "MSE_LOG_AFC", correct=True, **kw), mode=mode, clean=False, only=("fr",))
