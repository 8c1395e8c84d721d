"""GPU: pfr_sweep_complex and pfr_jacobian_sweep_complex on the synthetic fronts (tests/synthetic.py,
tests/synthetic_complex.py).

H at every frequency, the loss sum, every partial w_k and every Jacobian row are compared with the extended-precision
reference at

    10 x max(e_model, e_dense, 1e-14)

with e_model / e_dense the errors of the sweep's own sequence in fp64 through the multifrontal model and through the
unrefined dense LU, maximised over every sixth frequency of the sweep; computed here at run time, never from the GPU's
output.  Measures: H max_q |H_q - Href_q| / |Href_q|; the loss sum relative; w max_k |w_k - ref_k| / max_k |ref_k|; a
row max_k |row_k - ref_k| / max_k |ref_k|.  Besides: every flag 0, every backward error <= BERR_MAX, and h_dev / jc_dev
are allocated one entry / row longer, all NaN before the sweep -- the sweep's part comes back finite and the extra
entry untouched.
"""
import numpy as np
import pytest
import torch

import synthetic as sy
import synthetic_complex as sc
import synthetic_jacobian as sj
from helpers import report
from plate_inverse_problem_amd import _native
from test_gpu_synthetic import DEFAULT, RAW, _bounds, _t, check_sweep, make_solver, run_sweep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REFINE = RAW | _native.PFR_CHECK_REFINE                                       # mode 7 (15 with the correction)
Z, TILT = sc.AXES
ALL = sc.LOSSES + ("CCOTANGENT",)
LOSS_ID = dict(_native.COMPLEX_LOSS_IDS, NONE=_native.LOSS_NONE, CCOTANGENT=_native.LOSS_CCOTANGENT)
NAN = complex(float("nan"), float("nan"))

_CB = {}


def _cbounds(op, sym, freqs, axis, symmetric=True, correct=False, scale_corr=True, refine=False):
    """{loss_type: (bounds, e_model, e_dense)} from the model over every sixth frequency."""
    sub = np.asarray(freqs)[::sc.MODEL_EVERY]
    key = (id(op), id(sym), sub.tobytes(), tuple(axis), symmetric, correct, scale_corr, refine)
    if key not in _CB:
        me = sc.model_errors(op, sym, sub, axis, ALL, symmetric=symmetric, correct=correct, scale_corr=scale_corr,
                             refine=refine)
        _CB[key] = {lt: (sc.bounds(em, ed), em, ed) for lt, (em, ed) in me.items()}
    return _CB[key]


def run_complex(op, sym, freqs, axis, *, max_batch=64, mode=RAW, loss_type="MSE_LOG_COMPLEX", solver=None, fresh=False,
                scale=None):
    """One complex sweep through the C ABI.  h has nfreq + 1 entries, prefilled with NaN."""
    cref = sc.reference(op, freqs, axis)
    nf = len(freqs)
    sv, K = solver or make_solver(op, sym, max_batch)
    berr = torch.full((nf, 2), float("nan"), dtype=torch.float64, device=DEV)
    sv.set_check(mode, sy.BERR_MAX, berr)
    h = torch.full((nf + 1,), NAN, dtype=torch.complex128, device=DEV)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    w = torch.zeros(op.n_stiff, dtype=torch.complex128, device=DEV)
    flags = torch.zeros(nf, dtype=torch.int32, device=DEV)
    scale = 1.0 / nf if scale is None else scale
    ref = cref.sweep_ref(loss_type)
    sv.sweep_complex(_t(freqs), axis, LOSS_ID[loss_type], ref=None if ref is None else torch.view_as_real(_t(ref)),
                     scale=scale, h=torch.view_as_real(h), loss=loss, w=torch.view_as_real(w), flags=flags, fresh=fresh)
    torch.cuda.synchronize()
    return dict(H=h.cpu().numpy(), loss=float(loss.cpu()[0]), w=w.cpu().numpy(), berr=berr.cpu().numpy(),
                flags=flags.cpu().numpy(), scale=scale, cref=cref, solver=(sv, K))


def run_cjacobian(op, sym, freqs, axis, *, max_batch=64, mode=RAW, solver=None):
    """One complex Jacobian sweep.  h has nfreq + 1 entries and jc nfreq + 1 rows, prefilled with NaN."""
    nf = len(freqs)
    sv, K = solver or make_solver(op, sym, max_batch)
    berr = torch.full((nf, 2), float("nan"), dtype=torch.float64, device=DEV)
    sv.set_check(mode, sy.BERR_MAX, berr)
    h = torch.full((nf + 1,), NAN, dtype=torch.complex128, device=DEV)
    jc = torch.full((nf + 1, op.n_stiff), NAN, dtype=torch.complex128, device=DEV)
    flags = torch.zeros(nf, dtype=torch.int32, device=DEV)
    sv.jacobian_sweep_complex(_t(freqs), axis, torch.view_as_real(jc), h=torch.view_as_real(h), flags=flags)
    torch.cuda.synchronize()
    return dict(H=h.cpu().numpy(), jc=jc.cpu().numpy(), berr=berr.cpu().numpy(), flags=flags.cpu().numpy(),
                cref=sc.reference(op, freqs, axis), solver=(sv, K))


def check_complex(name, out, bound, loss_type):
    """Every comparison of one sweep (a loss sweep, or with "jc" in ``out`` a Jacobian sweep) with the reference."""
    cref = out["cref"]
    nf = cref.H.size
    every = np.arange(nf)
    b, em, ed = bound
    H = out["H"]
    assert np.isfinite(H[:nf].view(np.float64)).all(), "an entry of h was skipped"
    assert np.isnan(H[nf:].view(np.float64)).all(), "a padded lane stored its H"
    if "jc" in out:
        jc = out["jc"]
        assert np.isfinite(jc[:nf].view(np.float64)).all(), "a row of the sweep was skipped"
        assert np.isnan(jc[nf].view(np.float64)).all(), "a padded lane stored its row"
        err = sc.errors(cref, None, every, H=H[:nf], rows=jc[:nf])
    else:
        err = sc.errors(cref, loss_type, every, H=H[:nf], terms=[out["loss"]], w=out["w"], scale=out["scale"])
    be = out["berr"]
    print(name, " ".join(f"{k}={v:.2e}/{b[k]:.1e} (e_model {em[k]:.1e}, e_dense {ed[k]:.1e})" for k, v in err.items()),
          f"berr={np.nanmax(be):.1e}")
    report("synthetic_complex::" + name, berr=float(np.nanmax(be)), **err,
           **{k + "_ratio": v / b[k] for k, v in err.items()})
    assert np.all(out["flags"] == 0), out["flags"]
    assert np.all(np.isfinite(be)) and be.max() <= sy.BERR_MAX, be.max()
    for k, v in err.items():
        assert v <= b[k], (name, k, v, b[k])
    return err


def _model_kw(mode, env):
    return dict(correct=bool(mode & _native.PFR_CHECK_CORRECT), refine=bool(mode & _native.PFR_CHECK_REFINE),
                scale_corr=(env or {}).get("PFR_SCALE_CORR", "1") != "0")


def _complex_case(name, shape, monkeypatch, axis, env=None, mode=RAW, freqs=sy.FREQS, last=True, symmetric=True,
                  **case_kw):
    """The three losses, the caller's cotangent and the Jacobian rows on one solver, each against its bounds."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)              # the knobs are read in pfr_solver_create
    _, op = sy.case(shape, **case_kw)
    sym = sy.symbolic(shape, symmetric=symmetric, last=last)
    bound = _cbounds(op, sym, freqs, axis, symmetric=symmetric, **_model_kw(mode, env))
    solver = make_solver(op, sym, 64)
    for lt in ALL:
        check_complex(f"{name}-{lt}", run_complex(op, sym, freqs, axis, mode=mode, loss_type=lt, solver=solver),
                      bound[lt], lt)
    check_complex(f"{name}-rows", run_cjacobian(op, sym, freqs, axis, mode=mode, solver=solver), bound["CCOTANGENT"],
                  None)
    return solver


def _axid(a):
    return "z" if a == Z else "tilted"


# ----------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("axis", sc.AXES, ids=_axid)
@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("shape", ["F0", "A", "T"])
def test_shape(shape, mode, axis, monkeypatch):
    """130 frequencies at max_batch 64: two chunks and a 2-lane tail (h, ref and jc read at a global offset)."""
    _complex_case(f"{shape}-mode{mode}-{_axid(axis)}", shape, monkeypatch, axis, mode=mode)


# ----------------------------------------------------------------------------- routes
@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_18_stiffness_matrices(mode, monkeypatch):
    _complex_case(f"T-n_stiff18-mode{mode}", "T", monkeypatch, TILT, mode=mode, n_stiff=18)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_support_outside_the_root(mode, monkeypatch):
    _complex_case(f"T-spread-mode{mode}", "T", monkeypatch, TILT, mode=mode, last=False, spread=True)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_general_analysis(mode, monkeypatch):
    _complex_case(f"T-general-mode{mode}", "T", monkeypatch, TILT, mode=mode, symmetric=False)


@pytest.mark.parametrize("correct", [0, _native.PFR_CHECK_CORRECT], ids=["mode7", "mode15"])
def test_refined_sweep(correct, monkeypatch):
    """PFR_CHECK_REFINE on A: the unpaired forward / adjoint solves with one refinement step each (the model too)."""
    _complex_case(f"A-mode{REFINE | correct}", "A", monkeypatch, TILT, mode=REFINE | correct)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("shape", ["A", "T"])
def test_functional_from_the_top_down_solution(shape, mode, monkeypatch):
    """PFR_FN_DOT=0: the only way into k_functional<CPX> with G on the paired path."""
    _complex_case(f"{shape}-FN_DOT=0-mode{mode}", shape, monkeypatch, TILT, env={"PFR_FN_DOT": "0"}, mode=mode)


ROUTES = [{"PFR_SCALE_CORR": "0"}, {"PFR_CONTRACT_WALK": "0"}, {"PFR_SCALE_CORR": "0", "PFR_CONTRACT_WALK": "0"}]


@pytest.mark.parametrize("env", ROUTES, ids=[",".join(f"{k[4:]}={v}" for k, v in e.items()) for e in ROUTES])
@pytest.mark.parametrize("shape", ["A", "T"])
def test_contraction_routes(shape, env, monkeypatch):
    """The unscaled finish (m_q = scale g, t_q scaled by k_rhs_dot) and k_contract_eg / k_contract_q under the
    correction, with the complex m_q."""
    _complex_case(f"{shape}-" + ",".join(f"{k[4:]}={v}" for k, v in env.items()), shape, monkeypatch, TILT, env=env,
                  mode=DEFAULT)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("nfreq", [1, 63, 64, 65])
def test_batch_edges(nfreq, mode, monkeypatch):
    _complex_case(f"A4-nfreq{nfreq}-mode{mode}", "A4", monkeypatch, TILT, mode=mode, freqs=sy.FREQS[:nfreq])


# ----------------------------------------------------------------------------- tie to the verified magnitude path
def test_three_axes_give_the_magnitude():
    """RAW mode, forward only: sqrt(|H_e1|^2 + |H_e2|^2 + |H_e3|^2) on the solver of a magnitude sweep equals that
    sweep's fr to 1e-14 relative -- both are formed from the same U, V, W (k_functional on the same x) and differ by a
    handful of roundings."""
    _, op = sy.case("T")
    sym = sy.symbolic("T")
    mag = run_sweep(op, sym, sy.FREQS, mode=RAW, loss_type="NONE", vectors=False)
    nf = sy.FREQS.size
    s2 = 0
    for axis in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)):
        out = run_complex(op, sym, sy.FREQS, axis, mode=RAW, loss_type="NONE", solver=mag["solver"])
        assert np.all(out["flags"] == 0)
        s2 = s2 + np.abs(out["H"][:nf].astype(sy.CLD)) ** 2
    d = float(np.max(np.abs(np.sqrt(s2) / mag["fr"].astype(sy.LD) - 1)))
    print(f"T: |sqrt(sum |H_e|^2) / fr - 1| = {d:.2e}")
    report("synthetic_complex::T-three-axes", fr=d)
    assert d <= 1e-14


# ----------------------------------------------------------------------------- rows against the cotangent sweep
@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("shape", ["A", "T"])
def test_rows_contract_to_the_cotangent_sweep(shape, mode):
    """g @ jc against w of a PFR_LOSS_CCOTANGENT sweep (ref = g, scale 1) on the same solver: both are within the w
    bound of the same reference, so they differ by at most twice it.  Then three one-hot cotangents g = i (first, 64th
    and last frequency): that sweep's w against i x the row, at twice the row bound -- an imaginary g catches a dropped
    imaginary part."""
    _, op = sy.case(shape)
    sym = sy.symbolic(shape)
    bound = _cbounds(op, sym, sy.FREQS, TILT, correct=bool(mode & _native.PFR_CHECK_CORRECT))["CCOTANGENT"][0]
    out = run_cjacobian(op, sym, sy.FREQS, TILT, mode=mode)
    cref, nf = out["cref"], sy.FREQS.size
    jc = out["jc"][:nf].astype(sy.CLD)
    sw = run_complex(op, sym, sy.FREQS, TILT, mode=mode, loss_type="CCOTANGENT", solver=out["solver"], scale=1.0)
    mine = cref.cot.astype(sy.CLD) @ jc
    wref = cref.loss("CCOTANGENT")["w"].sum(axis=0)
    d_all = float(np.max(np.abs(mine - sw["w"].astype(sy.CLD))) / np.max(np.abs(wref)))
    sv, _ = out["solver"]
    sv.set_check(mode, sy.BERR_MAX, None)                    # run_complex's backward-error buffer is gone
    ft = _t(sy.FREQS)
    d_one = []
    for q in (0, 63, nf - 1):
        hot = np.zeros(nf, dtype=np.complex128)
        hot[q] = 1j
        w = torch.zeros(op.n_stiff, dtype=torch.complex128, device=DEV)
        sv.sweep_complex(ft, TILT, _native.LOSS_CCOTANGENT, ref=torch.view_as_real(_t(hot)), scale=1.0,
                         w=torch.view_as_real(w))
        torch.cuda.synchronize()
        d_one.append(sj.row_errors(w.cpu().numpy()[None, :], (sy.CLD(1j) * jc[q])[None, :]))
    print(f"{shape}-mode{mode}: |g @ jc - w| / max|w| = {d_all:.2e} (2 x {bound['w']:.1e}); one-hot rows "
          + " ".join(f"{d:.2e}" for d in d_one) + f" (2 x {bound['jc']:.1e})")
    report(f"synthetic_complex::{shape}-mode{mode}-vs-cotangent", sum=d_all, sum_bound=2 * bound["w"],
           rows=max(d_one), rows_bound=2 * bound["jc"])
    assert d_all <= 2 * bound["w"], (d_all, bound["w"])
    assert max(d_one) <= 2 * bound["jc"], (d_one, bound["jc"])


# ----------------------------------------------------------------------------- unchanged neighbours
def _same(first, second, keys=("fr", "w", "berr", "flags")):
    for k in keys:
        assert np.array_equal(first[k], second[k], equal_nan=True), k
    assert first["loss"] == second["loss"]


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_magnitude_sweep_is_unchanged_by_a_complex_sweep_between(mode):
    """A magnitude loss sweep, a complex loss sweep and a complex Jacobian sweep, the same magnitude sweep again on one
    solver: bit-identical fr, w, berr, flags and loss."""
    _, op = sy.case("T")
    sym = sy.symbolic("T")
    first = run_sweep(op, sym, sy.FREQS, mode=mode, vectors=False)
    run_complex(op, sym, sy.FREQS, TILT, mode=mode, solver=first["solver"])
    run_cjacobian(op, sym, sy.FREQS, TILT, mode=mode, solver=first["solver"])
    second = run_sweep(op, sym, sy.FREQS, mode=mode, vectors=False, solver=first["solver"])
    _same(first, second)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_magnitude_sweep_graph_is_not_replayed_past_a_complex_sweep(mode, monkeypatch):
    """PFR_GRAPH=1: three magnitude sweeps with the same arguments (the third is replayed from the graph), a complex
    sweep -- which does not advance graph_launches() --, then the same magnitude sweep: bit-identical and run directly.
    On a stream of its own: the default stream cannot be captured."""
    monkeypatch.setenv("PFR_GRAPH", "1")
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        _graph_case(mode)


def _graph_case(mode):
    _, op = sy.case("T")
    sym = sy.symbolic("T")
    first = run_sweep(op, sym, sy.FREQS, mode=mode, vectors=False)
    sv, _ = first["solver"]
    refc = first["refc"]
    nf = sy.FREQS.size
    berr = torch.full((nf, 2), float("nan"), dtype=torch.float64, device=DEV)
    sv.set_check(mode, sy.BERR_MAX, berr)
    ft, rt = _t(sy.FREQS), torch.view_as_real(_t(refc.ref))
    fr = torch.zeros(nf, dtype=torch.float64, device=DEV)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    w = torch.zeros(op.n_stiff, dtype=torch.complex128, device=DEV)
    flags = torch.zeros(nf, dtype=torch.int32, device=DEV)

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
    cref = sc.reference(op, sy.FREQS, TILT)
    wc = torch.zeros(op.n_stiff, dtype=torch.complex128, device=DEV)
    for _ in range(3):                                       # the same complex sweep again and again: never captured
        sv.sweep_complex(ft, TILT, _native.LOSS_CLOG, ref=torch.view_as_real(_t(cref.ref)), scale=first["scale"],
                         w=torch.view_as_real(wc))
    torch.cuda.synchronize()
    assert sv.graph_launches() == replayed
    after = sweep()
    assert sv.graph_launches() == replayed                   # not replayed: the graph was dropped
    _same(before, after)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_two_complex_sweeps_give_identical_bits(mode):
    _, op = sy.case("T")
    sym = sy.symbolic("T")
    a = run_complex(op, sym, sy.FREQS, TILT, mode=mode)
    b = run_complex(op, sym, sy.FREQS, TILT, mode=mode, solver=a["solver"])
    _same(a, b, keys=("H", "w", "berr", "flags"))
    ja = run_cjacobian(op, sym, sy.FREQS, TILT, mode=mode, solver=a["solver"])
    jb = run_cjacobian(op, sym, sy.FREQS, TILT, mode=mode, solver=a["solver"])
    for k in ("H", "jc", "berr", "flags"):
        assert np.array_equal(ja[k], jb[k], equal_nan=True), k


# ----------------------------------------------------------------------------- refusals
def test_refusals():
    """Every refused call returns PFR_ERR_ARG before anything is launched (the outputs stay as they were), and a
    valid sweep after them still passes its bounds."""
    _, op = sy.case("A")
    sym = sy.symbolic("A")
    sv, K = solver = make_solver(op, sym, 64)
    nf = sy.FREQS.size
    cref = sc.reference(op, sy.FREQS, TILT)
    sv.set_check(DEFAULT, sy.BERR_MAX, None)
    ft, rt = _t(sy.FREQS), torch.view_as_real(_t(cref.ref))
    h = torch.full((nf,), NAN, dtype=torch.complex128, device=DEV)
    w = torch.full((op.n_stiff,), NAN, dtype=torch.complex128, device=DEV)
    jc = torch.full((nf, op.n_stiff), NAN, dtype=torch.complex128, device=DEV)
    hv, wv, jv = torch.view_as_real(h), torch.view_as_real(w), torch.view_as_real(jc)

    def refused(call):
        with pytest.raises(_native.NativeError, match=r"\(status 1\)"):
            call()

    for bad in (0, 1, 2, 3, 4, 5, 15, 20, -2):                                # real ids, LOSS_UNIT, out of range
        refused(lambda: sv.sweep_complex(ft, TILT, bad, ref=rt, h=hv, w=wv))
    for axis in ((0.0, 0.0, 0.0), (float("nan"), 0.0, 1.0), (0.0, float("inf"), 1.0)):
        refused(lambda: sv.sweep_complex(ft, axis, _native.LOSS_NONE, h=hv))
        refused(lambda: sv.sweep_complex(ft, axis, _native.LOSS_CMSE, ref=rt, h=hv, w=wv))
        refused(lambda: sv.jacobian_sweep_complex(ft, axis, jv, h=hv))
    refused(lambda: sv.sweep_complex(ft, TILT, _native.LOSS_CMSE, ref=None, h=hv, w=wv))
    sv.set_check(DEFAULT | _native.PFR_CHECK_REFINE_ADJ, sy.BERR_MAX, None)
    refused(lambda: sv.sweep_complex(ft, TILT, _native.LOSS_CMSE, ref=rt, h=hv, w=wv))
    refused(lambda: sv.jacobian_sweep_complex(ft, TILT, jv, h=hv))
    sv.set_check(DEFAULT, sy.BERR_MAX, None)
    for cid in sorted(LOSS_ID[k] for k in ALL):                               # the magnitude's calls keep refusing them
        refused(lambda: sv.sweep(ft, cid, ref=rt, w=wv))
        refused(lambda: sv.hessian_sweep(ft, cid, rt, 1.0, sy.direction(1, op.n_stiff), w=wv, h=wv))
    torch.cuda.synchronize()
    for t in (h, w, jc):
        assert torch.isnan(torch.view_as_real(t)).all(), "a refused call wrote"
    bound = _cbounds(op, sym, sy.FREQS, TILT, correct=True)
    check_complex("A-after-refusals", run_complex(op, sym, sy.FREQS, TILT, mode=DEFAULT, solver=solver),
                  bound["MSE_LOG_COMPLEX"], "MSE_LOG_COMPLEX")
    mag = run_sweep(op, sym, sy.FREQS, mode=DEFAULT, vectors=False, solver=solver)
    check_sweep("A-after-complex-refusals", mag, _bounds(op, sym, sy.FREQS, "MSE_LOG_AFC", correct=True), mode=DEFAULT)
