"""GPU: pfr_jacobian_sweep on the synthetic fronts (tests/synthetic.py, tests/synthetic_jacobian.py).

Every row of jc and every fr is compared with the extended-precision reference at

    10 x max(e_model, e_dense, 1e-14)

with e_model / e_dense the row (fr) errors of the same sequence in fp64 through the multifrontal model and through the
unrefined dense LU, maximised over every sixth frequency of the sweep (22 of 130); computed here at run time, never
from the GPU's output.  The measure of a row is max_k |row_k - ref_k| / max_k |ref_k|.  Besides: every flag 0, every
backward error <= BERR_MAX, and jc is allocated with one row more than the sweep has, all NaN before the sweep -- the
rows of the sweep come back without a NaN and the last row untouched.
"""
import numpy as np
import pytest
import torch

import synthetic as sy
import synthetic_jacobian as sj
from helpers import report
from plate_inverse_problem_amd import _native
from test_gpu_synthetic import DEFAULT, RAW, _bounds, _t, make_solver, run_sweep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REFINE = RAW | _native.PFR_CHECK_REFINE                                       # mode 7 (15 with the correction)
MODEL_EVERY = 6                                                               # the model's sample of the sweep

_JB = {}


def _jac_bounds(op, sym, freqs, symmetric=True, correct=False, scale_corr=True, refine=False):
    sub = np.asarray(freqs)[::MODEL_EVERY]
    key = (id(op), id(sym), sub.tobytes(), symmetric, correct, scale_corr, refine)
    if key not in _JB:
        em, ed = sj.jacobian_model_errors(op, sym, sub, symmetric=symmetric, correct=correct, scale_corr=scale_corr,
                                          refine=refine)
        _JB[key] = (sj.bounds(em, ed), em, ed)
    return _JB[key]


def run_jacobian(op, sym, freqs, *, max_batch=64, mode=RAW, solver=None):
    """One Jacobian sweep through the C ABI.  jc has nfreq + 1 rows, prefilled with NaN."""
    nf = len(freqs)
    sv, K = solver or make_solver(op, sym, max_batch)
    berr = torch.full((nf, 2), float("nan"), dtype=torch.float64, device=DEV)
    sv.set_check(mode, sy.BERR_MAX, berr)
    fr = torch.zeros(nf, dtype=torch.float64, device=DEV)
    jc = torch.full((nf + 1, op.n_stiff), complex(float("nan"), float("nan")), dtype=torch.complex128, device=DEV)
    flags = torch.zeros(nf, dtype=torch.int32, device=DEV)
    sv.jacobian_sweep(_t(freqs), torch.view_as_real(jc), fr=fr, flags=flags)
    torch.cuda.synchronize()
    return dict(fr=fr.cpu().numpy(), jc=jc.cpu().numpy(), berr=berr.cpu().numpy(), flags=flags.cpu().numpy(),
                solver=(sv, K), refc=sy.reference(op, freqs))


def check_jacobian(name, out, bound):
    refc = out["refc"]
    nf = refc.freqs.size
    jc = out["jc"]
    assert not np.isnan(jc[:nf].view(np.float64)).any(), "a row of the sweep was skipped"
    assert np.isnan(jc[nf].view(np.float64)).all(), "a padded lane stored its row"
    b, em, ed = bound
    err = {"jc": sj.row_errors(jc[:nf], sj.jacobian_reference(refc)),
           "fr": float(np.max(np.abs(out["fr"].astype(sy.LD) / refc.fr - 1)))}
    be = out["berr"]
    print(name, " ".join(f"{k}={v:.2e}/{b[k]:.1e} (e_model {em[k]:.1e}, e_dense {ed[k]:.1e})" for k, v in err.items()),
          f"berr={np.nanmax(be):.1e}")
    report("synthetic_jacobian::" + name, berr=float(np.nanmax(be)), jc_bound=b["jc"], fr_bound=b["fr"], **err)
    assert np.all(out["flags"] == 0), out["flags"]
    assert np.all(np.isfinite(be)) and be.max() <= sy.BERR_MAX, be.max()
    for k, v in err.items():
        assert v <= b[k], (name, k, v, b[k])
    return err


def _model_kw(mode, env):
    return dict(correct=bool(mode & _native.PFR_CHECK_CORRECT), scale_corr=(env or {}).get("PFR_SCALE_CORR", "1") != "0")


def _jac_case(name, shape, monkeypatch, env=None, mode=RAW, freqs=sy.FREQS, last=True, symmetric=True, **case_kw):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)              # the knobs are read in pfr_solver_create
    _, op = sy.case(shape, **case_kw)
    sym = sy.symbolic(shape, symmetric=symmetric, last=last)
    bound = _jac_bounds(op, sym, freqs, symmetric=symmetric, **_model_kw(mode, env))
    out = run_jacobian(op, sym, freqs, mode=mode)
    check_jacobian(name, out, bound)
    return out


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("shape", sorted(sy.SHAPES))
def test_shape(shape, mode, monkeypatch):
    """130 frequencies at max_batch 64: two chunks and a 2-lane tail (the global row offset q0)."""
    _jac_case(f"{shape}-mode{mode}", shape, monkeypatch, mode=mode)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_18_stiffness_matrices(mode, monkeypatch):
    _jac_case(f"T-n_stiff18-mode{mode}", "T", monkeypatch, mode=mode, n_stiff=18)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_support_outside_the_root(mode, monkeypatch):
    _jac_case(f"T-spread-mode{mode}", "T", monkeypatch, mode=mode, last=False, spread=True)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("shape", sorted(sy.GENERAL_SHAPES))
def test_general_analysis(shape, mode, monkeypatch):
    _jac_case(f"{shape}-general-mode{mode}", shape, monkeypatch, mode=mode, symmetric=False)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("nfreq", [1, 63, 64, 65])
def test_batch_edges(nfreq, mode, monkeypatch):
    _jac_case(f"B-nfreq{nfreq}-mode{mode}", "B", monkeypatch, mode=mode, freqs=sy.FREQS[:nfreq])


ROUTES = [({"PFR_CONTRACT_WALK": "0"}, DEFAULT), ({"PFR_SCALE_CORR": "0"}, DEFAULT),
          ({"PFR_CONTRACT_WALK": "0", "PFR_SCALE_CORR": "0"}, DEFAULT)]


@pytest.mark.parametrize("env,mode", ROUTES, ids=[",".join(f"{k[4:]}={v}" for k, v in e.items()) for e, _ in ROUTES])
@pytest.mark.parametrize("shape", ["A", "T"])
def test_contraction_routes(shape, env, mode, monkeypatch):
    """k_contract_q under the correction (its rows scaled by m_q in k_jac_finish) and the unscaled finish (m_q = 1,
    t_q scaled by k_rhs_dot); RAW, the third route into k_contract_q, is test_shape's raw half."""
    _jac_case(f"{shape}-" + ",".join(f"{k[4:]}={v}" for k, v in env.items()), shape, monkeypatch, env=env, mode=mode)


@pytest.mark.parametrize("correct", [0, _native.PFR_CHECK_CORRECT], ids=["mode7", "mode15"])
def test_refined_sweep(correct, monkeypatch):
    """PFR_CHECK_REFINE on A: the unpaired forward / adjoint solves with one refinement step each (the model too)."""
    _, op = sy.case("A")
    sym = sy.symbolic("A")
    bound = _jac_bounds(op, sym, sy.FREQS, correct=bool(correct), refine=True)
    check_jacobian(f"A-mode{REFINE | correct}", run_jacobian(op, sym, sy.FREQS, mode=REFINE | correct), bound)


# ----------------------------------------------------------------------------- consistency with the loss sweep
@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("shape", ["A", "T"])
def test_rows_contract_to_the_cotangent_sweep(shape, mode):
    """cot @ jc against w of a PFR_LOSS_COTANGENT sweep (scale 1 / nfreq) on the same solver: both are within the w
    bound of the same reference, so they differ by at most twice it.  Then three one-hot cotangents (first, 64th and
    last frequency): that sweep's w against the row, at twice the row bound."""
    _, op = sy.case(shape)
    sym = sy.symbolic(shape)
    correct = bool(mode & _native.PFR_CHECK_CORRECT)
    out = run_jacobian(op, sym, sy.FREQS, mode=mode)
    refc, nf = out["refc"], sy.FREQS.size
    jc = out["jc"][:nf].astype(sy.CLD)
    wb = _bounds(op, sym, sy.FREQS, "COTANGENT", **({"correct": True} if correct else {}))["w"]
    sw = run_sweep(op, sym, sy.FREQS, mode=mode, loss_type="COTANGENT", vectors=False, solver=out["solver"])
    mine = (refc.cot.astype(sy.LD) @ jc) * sy.LD(sw["scale"])
    wref = sw["scale"] * refc.loss("COTANGENT")["w"].sum(axis=0)
    d_all = float(np.max(np.abs(mine - sw["w"].astype(sy.CLD))) / np.max(np.abs(wref)))
    jb = _jac_bounds(op, sym, sy.FREQS, correct=correct)[0]["jc"]
    sv, _ = out["solver"]
    sv.set_check(mode, sy.BERR_MAX, None)                    # run_sweep's backward-error buffer is gone
    ft = _t(sy.FREQS)
    d_one = []
    for q in (0, 63, nf - 1):
        hot = np.zeros(nf, dtype=np.complex128)
        hot[q] = 1.0
        w = torch.zeros(op.n_stiff, dtype=torch.complex128, device=DEV)
        sv.sweep(ft, _native.LOSS_COTANGENT, ref=torch.view_as_real(_t(hot)), scale=1.0, w=torch.view_as_real(w))
        torch.cuda.synchronize()
        d_one.append(sj.row_errors(w.cpu().numpy()[None, :], jc[q][None, :]))
    print(f"{shape}-mode{mode}: |cot @ jc - w| / max|w| = {d_all:.2e} (2 x {wb:.1e}); one-hot rows "
          + " ".join(f"{d:.2e}" for d in d_one) + f" (2 x {jb:.1e})")
    report(f"synthetic_jacobian::{shape}-mode{mode}-vs-cotangent", sum=d_all, sum_bound=2 * wb, rows=max(d_one),
           rows_bound=2 * jb)
    assert d_all <= 2 * wb, (d_all, wb)
    assert max(d_one) <= 2 * jb, (d_one, jb)


def _same(first, second):
    for k in ("fr", "w", "berr", "flags"):
        assert np.array_equal(first[k], second[k], equal_nan=True), k
    assert first["loss"] == second["loss"]


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_loss_sweep_is_unchanged_by_a_jacobian_sweep_between(mode):
    """A loss sweep, a Jacobian sweep, the same loss sweep again on one solver: bit-identical fr, w, berr, flags and
    loss (the Jacobian sweep overwrites kpart, tq, mscale, loss_terms, G, XA, ...)."""
    _, op = sy.case("T")
    sym = sy.symbolic("T")
    first = run_sweep(op, sym, sy.FREQS, mode=mode, vectors=False)
    run_jacobian(op, sym, sy.FREQS, mode=mode, solver=first["solver"])
    second = run_sweep(op, sym, sy.FREQS, mode=mode, vectors=False, solver=first["solver"])
    _same(first, second)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_loss_sweep_graph_is_not_replayed_past_a_jacobian_sweep(mode, monkeypatch):
    """PFR_GRAPH=1: three loss sweeps with the same arguments (the third is replayed from the graph), the Jacobian
    sweep, then the same loss sweep: bit-identical to a sweep into fresh outputs before it, and run directly.  On a
    stream of its own, as the engine's lanes run: the default stream cannot be captured."""
    monkeypatch.setenv("PFR_GRAPH", "1")
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        _graph_case(mode)


def _graph_case(mode):
    _, op = sy.case("T")
    sym = sy.symbolic("T")
    first = run_sweep(op, sym, sy.FREQS, mode=mode, vectors=False)
    sv, _ = first["solver"]
    refc = first["refc"]
    berr = torch.full((sy.FREQS.size, 2), float("nan"), dtype=torch.float64, device=DEV)
    sv.set_check(mode, sy.BERR_MAX, berr)
    ft, rt = _t(sy.FREQS), torch.view_as_real(_t(refc.ref))
    fr = torch.zeros(sy.FREQS.size, dtype=torch.float64, device=DEV)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    w = torch.zeros(op.n_stiff, dtype=torch.complex128, device=DEV)
    flags = torch.zeros(sy.FREQS.size, dtype=torch.int32, device=DEV)

    def sweep():
        loss.zero_()
        w.zero_()
        flags.zero_()
        sv.sweep(ft, _native.LOSS_MSE_LOG_AFC, ref=rt, scale=first["scale"], fr=fr, loss=loss, w=torch.view_as_real(w),
                 flags=flags)
        torch.cuda.synchronize()
        return dict(fr=fr.cpu().numpy(), loss=float(loss.cpu()[0]), w=w.cpu().numpy(), berr=berr.cpu().numpy(),
                    flags=flags.cpu().numpy())

    for _ in range(3):
        before = sweep()
    replayed = sv.graph_launches()
    assert replayed >= 1                                     # a graph exists
    _same(first, before)
    jc = torch.empty((sy.FREQS.size, op.n_stiff), dtype=torch.complex128, device=DEV)
    sv.jacobian_sweep(ft, torch.view_as_real(jc))
    after = sweep()
    assert sv.graph_launches() == replayed                   # not replayed: the graph was dropped
    _same(before, after)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_two_jacobian_sweeps_give_identical_bits(mode):
    _, op = sy.case("T")
    sym = sy.symbolic("T")
    a = run_jacobian(op, sym, sy.FREQS, mode=mode)
    b = run_jacobian(op, sym, sy.FREQS, mode=mode, solver=a["solver"])
    for k in ("fr", "jc", "berr", "flags"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
