"""GPU: pfr_inertia_sweep on the synthetic fronts (tests/synthetic.py, tests/synthetic_inertia.py).

Every row of jm and jc and every response is compared with the extended-precision reference at

    10 x max(e_model, e_dense, 1e-14)

with e_model / e_dense the errors of the same sequence in fp64 through the multifrontal model and through the unrefined
dense LU, maximised over every sixth frequency of the sweep; computed here at run time, never from the GPU's output.
The measure of a row is max_j |row_j - ref_j| / max_j |ref_j|.  Besides: every flag 0, every backward error <=
BERR_MAX, and jm / jc are allocated with one row more than the sweep has, all NaN before the sweep -- the rows of the
sweep come back without a NaN and the last row untouched.  130 frequencies at max_batch 64 unless said: two chunks and
a 2-lane tail.
"""
import numpy as np
import pytest
import torch

import synthetic as sy
import synthetic_inertia as si
import synthetic_jacobian as sj
from helpers import report
from plate_inverse_problem_amd import _native
from test_gpu_synthetic import DEFAULT, RAW, _t, make_solver, run_sweep
from test_gpu_synthetic_complex import run_cjacobian
from test_gpu_synthetic_jacobian import run_jacobian

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REFINE = RAW | _native.PFR_CHECK_REFINE                                       # mode 7 (15 with the correction)
MODEL_EVERY = 6                                                               # the model's sample of the sweep
AXES = ((0.0, 0.0, 1.0), (0.6, 0.8, 1.0))
NAN = complex(float("nan"), float("nan"))

_IB = {}


def _bounds(ins, sym, freqs, symmetric=True, correct=False, scale_corr=True, refine=False, axis=None):
    sub = np.asarray(freqs)[::MODEL_EVERY]
    key = (id(ins), id(sym), sub.tobytes(), symmetric, correct, scale_corr, refine, axis)
    if key not in _IB:
        em, ed = si.model_errors(ins, sym, sub, symmetric=symmetric, correct=correct, scale_corr=scale_corr,
                                 refine=refine, axis=axis)
        _IB[key] = (si.bounds(em, ed), em, ed)
    return _IB[key]


def inertia_solver(ins, sym, max_batch=64, prune=None, register=True):
    sv, K = make_solver(ins.op, sym, max_batch, prune=prune)
    if register:
        sv.set_inertia(_t(ins.G.T), ins.d)                                    # (nnz, n_mass)
    return sv, K


def run_inertia(ins, sym, freqs, *, max_batch=64, mode=RAW, axis=None, with_jc=True, solver=None):
    """One inertia sweep through the C ABI.  jm and jc have nfreq + 1 rows, prefilled with NaN."""
    op, nf = ins.op, len(freqs)
    sv, K = solver or inertia_solver(ins, sym, max_batch)
    berr = torch.full((nf, 2), float("nan"), dtype=torch.float64, device=DEV)
    sv.set_check(mode, sy.BERR_MAX, berr)
    resp = torch.zeros(nf, dtype=torch.float64 if axis is None else torch.complex128, device=DEV)
    jm = torch.full((nf + 1, ins.n_mass), NAN, dtype=torch.complex128, device=DEV)
    jc = torch.full((nf + 1, op.n_stiff), NAN, dtype=torch.complex128, device=DEV) if with_jc else None
    flags = torch.zeros(nf, dtype=torch.int32, device=DEV)
    sv.inertia_sweep(_t(freqs), torch.view_as_real(jm), axis=axis,
                     resp=resp if axis is None else torch.view_as_real(resp),
                     jc=None if jc is None else torch.view_as_real(jc), flags=flags)
    torch.cuda.synchronize()
    return dict(resp=resp.cpu().numpy(), jm=jm.cpu().numpy(), jc=None if jc is None else jc.cpu().numpy(),
                berr=berr.cpu().numpy(), flags=flags.cpu().numpy(), solver=(sv, K), axis=axis)


def check_inertia(name, ins, freqs, out, bound):
    nf = len(freqs)
    b, em, ed = bound
    resp, jc, jm = si.reference(ins, freqs, out["axis"])
    assert not np.isnan(out["jm"][:nf].view(np.float64)).any(), "a row of the sweep was skipped"
    assert np.isnan(out["jm"][nf].view(np.float64)).all(), "a padded lane stored its row"
    err = {"jm": sj.row_errors(out["jm"][:nf], jm), "resp": si.resp_error(out["resp"], resp)}
    if out["jc"] is not None:
        assert not np.isnan(out["jc"][:nf].view(np.float64)).any() and np.isnan(out["jc"][nf].view(np.float64)).all()
        err["jc"] = sj.row_errors(out["jc"][:nf], jc)
        err["hom"] = float(si.homogeneity(ins, out["jc"][:nf], out["jm"][:nf]).max())
    be = out["berr"]
    print(name, " ".join(f"{k}={v:.2e}/{b[k]:.1e} (e_model {em[k]:.1e}, e_dense {ed[k]:.1e})" for k, v in err.items()),
          f"berr={np.nanmax(be):.1e}")
    report("synthetic_inertia::" + name, berr=float(np.nanmax(be)), **err, **{k + "_bound": b[k] for k in err})
    assert np.all(out["flags"] == 0), out["flags"]
    assert np.all(np.isfinite(be)) and be.max() <= sy.BERR_MAX, be.max()
    for k, v in err.items():
        assert v <= b[k], (name, k, v, b[k])
    return err


def _model_kw(mode, env):
    return dict(correct=bool(mode & _native.PFR_CHECK_CORRECT), scale_corr=(env or {}).get("PFR_SCALE_CORR", "1") != "0")


def _case(name, shape, monkeypatch, env=None, mode=RAW, freqs=sy.FREQS, symmetric=True, general=False, axis=None,
          with_jc=True, split_kw=None, **case_kw):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)              # the knobs are read in pfr_solver_create
    _, op = sy.case(shape, general=general, **case_kw)
    ins = si.split(op, **(split_kw or {}))
    sym = sy.symbolic(shape, symmetric=symmetric, general=general)
    bound = _bounds(ins, sym, freqs, symmetric=symmetric, axis=axis, **_model_kw(mode, env))
    out = run_inertia(ins, sym, freqs, mode=mode, axis=axis, with_jc=with_jc)
    check_inertia(name, ins, freqs, out, bound)
    return ins, out


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("shape", sorted(sy.SHAPES))
def test_shape(shape, mode, monkeypatch):
    """n_mass = 4; the homogeneity of the GPU's own jc and jm at every frequency rides along (check_inertia: "hom",
    against 10 x the same residual of the fp64 model's rows)."""
    _case(f"{shape}-mode{mode}", shape, monkeypatch, mode=mode)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("n_mass", [1, 3])
def test_fewer_components(n_mass, mode, monkeypatch):
    """n_mass 1 and 3 on T (4 is test_shape's): the zero columns of the entry-ordered copy, rows of n_mass entries."""
    ins, out = _case(f"T-n_mass{n_mass}-mode{mode}", "T", monkeypatch, mode=mode, split_kw={"n_mass": n_mass})
    assert out["jm"].shape[1] == n_mass


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_18_stiffness_matrices(mode, monkeypatch):
    _case(f"T-n_stiff18-mode{mode}", "T", monkeypatch, mode=mode, n_stiff=18)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_without_stiffness_rows(mode, monkeypatch):
    """jc_dev = NULL: the same jm, resp, flags and backward errors, bit for bit, as with the rows."""
    ins, out = _case(f"T-nojc-mode{mode}", "T", monkeypatch, mode=mode, with_jc=False)
    both = run_inertia(ins, sy.symbolic("T"), sy.FREQS, mode=mode, solver=out["solver"])
    for k in ("resp", "jm", "berr", "flags"):
        assert np.array_equal(out[k], both[k], equal_nan=True), k


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_zero_component(mode, monkeypatch):
    """Component 1 zero everywhere: its rows are -om2 d_1 t_q, from the load term alone."""
    ins, out = _case(f"T-zero1-mode{mode}", "T", monkeypatch, mode=mode, split_kw={"zero": (1,)})
    assert not ins.G[1].any() and np.all(out["jm"][:-1, 1] != 0)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("entries", [1, 5])
def test_masked_components(entries, mode, monkeypatch):
    """Components masked to exactly 1 and 5 non-zero entries: the list's tail, and waves with no entry at all."""
    ins, out = _case(f"T-entries{entries}-mode{mode}", "T", monkeypatch, mode=mode,
                     split_kw={"n_mass": 1, "entries": entries})
    assert out["solver"][0].mass_list()[0] == entries


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("nfreq", [1, 63, 64, 65])
def test_batch_edges(nfreq, mode, monkeypatch):
    _case(f"B-nfreq{nfreq}-mode{mode}", "B", monkeypatch, mode=mode, freqs=sy.FREQS[:nfreq])


ROUTES = [{"PFR_CONTRACT_WALK": "0"}, {"PFR_SCALE_CORR": "0"}, {"PFR_CONTRACT_WALK": "0", "PFR_SCALE_CORR": "0"}]


@pytest.mark.parametrize("env", ROUTES, ids=[",".join(f"{k[4:]}={v}" for k, v in e.items()) for e in ROUTES])
@pytest.mark.parametrize("shape", ["A", "T"])
def test_contraction_routes(shape, env, monkeypatch):
    """The default mode without the walk's contraction (k_contract_q's partials in kpart before the mass partials
    take their place) and without the solve-error scale (m_q = 1, t_q scaled by k_rhs_dot)."""
    _case(f"{shape}-" + ",".join(f"{k[4:]}={v}" for k, v in env.items()), shape, monkeypatch, env=env, mode=DEFAULT)


@pytest.mark.parametrize("correct", [0, _native.PFR_CHECK_CORRECT], ids=["mode7", "mode15"])
def test_refined_sweep(correct):
    _, op = sy.case("A")
    ins = si.split(op)
    sym = sy.symbolic("A")
    bound = _bounds(ins, sym, sy.FREQS, correct=bool(correct), refine=True)
    check_inertia(f"A-mode{REFINE | correct}", ins, sy.FREQS, run_inertia(ins, sym, sy.FREQS, mode=REFINE | correct), bound)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("shape", sorted(sy.GENERAL_SHAPES))
def test_general_analysis(shape, mode, monkeypatch):
    _case(f"{shape}-general-mode{mode}", shape, monkeypatch, mode=mode, symmetric=False)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("axis", AXES, ids=["w", "tilted"])
def test_complex_response(axis, mode, monkeypatch):
    """The complex response H along two axes: dH / dI_j = jm[q][j], against the complex reference rows."""
    _case(f"T-axis{axis}-mode{mode}", "T", monkeypatch, mode=mode, axis=axis)


# ----------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("axis", [None, AXES[1]], ids=["fr", "H"])
@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_jacobian_outputs_are_those_of_the_jacobian_sweep(mode, axis):
    """resp, jc, flags and backward errors: bitwise pfr_jacobian_sweep's (_complex's) on the same solver state."""
    _, op = sy.case("T")
    ins = si.split(op)
    sym = sy.symbolic("T")
    out = run_inertia(ins, sym, sy.FREQS, mode=mode, axis=axis)
    if axis is None:
        jac = run_jacobian(ins.op, sym, sy.FREQS, mode=mode, solver=out["solver"])
        resp = jac["fr"]
    else:
        jac = run_cjacobian(ins.op, sym, sy.FREQS, axis, mode=mode, solver=out["solver"])
        resp = jac["H"][:-1]
    assert np.array_equal(out["resp"], resp)
    for k in ("jc", "berr", "flags"):
        assert np.array_equal(out[k], jac[k], equal_nan=True), k


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_loss_sweep_is_unchanged_by_an_inertia_sweep_between(mode):
    _, op = sy.case("T")
    ins = si.split(op)
    sym = sy.symbolic("T")
    solver = inertia_solver(ins, sym)
    first = run_sweep(ins.op, sym, sy.FREQS, mode=mode, vectors=False, solver=solver)
    run_inertia(ins, sym, sy.FREQS, mode=mode, solver=solver)
    second = run_sweep(ins.op, sym, sy.FREQS, mode=mode, vectors=False, solver=solver)
    for k in ("fr", "w", "berr", "flags"):
        assert np.array_equal(first[k], second[k], equal_nan=True), k
    assert first["loss"] == second["loss"]


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_two_inertia_sweeps_give_identical_bits(mode):
    _, op = sy.case("T")
    ins = si.split(op)
    sym = sy.symbolic("T")
    a = run_inertia(ins, sym, sy.FREQS, mode=mode)
    b = run_inertia(ins, sym, sy.FREQS, mode=mode, solver=a["solver"])
    for k in ("resp", "jc", "jm", "berr", "flags"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ----------------------------------------------------------------------------- pruning
def _forest_freqs(forest):
    return sy.FREQS[::2] if forest == "ETF0" else sy.FREQS     # as tests/test_gpu_synthetic_prune.py


@pytest.mark.parametrize("forest,load", sy.FOREST_CASES, ids=[sy.forest_id(f, l) for f, l in sy.FOREST_CASES])
def test_pruned(forest, load):
    """Pruning on, default mode: against the reference of the whole block-diagonal operator, and bit for bit against
    pruning off (the list of the view keeps every entry on the wave that owns it in the full list; what it drops
    adds exact zeros there)."""
    _, op = sy.case(forest, load=load)
    ins = si.split(op)
    sym = sy.symbolic(forest)
    freqs = _forest_freqs(forest)
    bound = _bounds(ins, sym, freqs, correct=True)
    on = run_inertia(ins, sym, freqs, mode=DEFAULT, solver=inertia_solver(ins, sym, prune=True))
    mask = on["solver"][0].active_fronts()
    assert 0 < mask.sum() < mask.size
    n_on = on["solver"][0].mass_list()[0]
    check_inertia(f"prune-{sy.forest_id(forest, load)}", ins, freqs, on, bound)
    off = run_inertia(ins, sym, freqs, mode=DEFAULT, solver=inertia_solver(ins, sym, prune=False))
    assert 0 < n_on < off["solver"][0].mass_list()[0]
    for k in ("resp", "jc", "jm", "flags"):
        assert np.array_equal(on[k], off[k], equal_nan=True), k


def test_pruned_list_follows_the_loaded_set():
    """One solver, pruning on: a sweep loaded on component 0 of AC, pfr_set_rhs moving the load to component 1, a
    sweep: each bitwise a fresh solver's put directly into that state."""
    sym = sy.symbolic("AC")
    ins = {load: si.split(sy.case("AC", load=load)[1]) for load in ((0,), (1,))}
    a, b = ins[(0,)], ins[(1,)]
    assert np.array_equal(a.G, b.G) and np.array_equal(a.op.M, b.op.M)        # the same operator, another load
    solver = inertia_solver(a, sym, prune=True)
    first = run_inertia(a, sym, sy.FREQS, mode=DEFAULT, solver=solver)
    n_first = solver[0].mass_list()[0]
    solver[0].set_rhs(b.op.rhs, b.op.beta, b.op.mass_sum)
    solver[0].set_functional(b.op.sup, b.op.a3, b.op.ts)                       # the cases draw their own weights
    second = run_inertia(b, sym, sy.FREQS, mode=DEFAULT, solver=solver)
    n_second = solver[0].mass_list()[0]
    assert n_first != n_second and n_first > 0 and n_second > 0
    for ins_k, got in ((a, first), (b, second)):
        fresh = run_inertia(ins_k, sym, sy.FREQS, mode=DEFAULT, solver=inertia_solver(ins_k, sym, prune=True))
        for k in ("resp", "jc", "jm", "berr", "flags"):
            assert np.array_equal(got[k], fresh[k], equal_nan=True), k
    check_inertia("prune-AC-moved-load", b, sy.FREQS, second, _bounds(b, sym, sy.FREQS, correct=True))


# ----------------------------------------------------------------------------- errors
def test_errors_launch_nothing():
    """A sweep before pfr_set_inertia: PFR_ERR_STATE; n_mass 0 and 5: PFR_ERR_ARG; jm untouched each time, and the
    next valid sweep is fine."""
    _, op = sy.case("A")
    ins = si.split(op)
    sym = sy.symbolic("A")
    sv, K = inertia_solver(ins, sym, register=False)
    L = _native.lib()
    ft = _t(sy.FREQS)
    jm = torch.full((sy.FREQS.size, 4), NAN, dtype=torch.complex128, device=DEV)
    args = (sv._h, ft.numel(), ft.data_ptr(), None, None, None, jm.data_ptr(), None, None)
    assert sv.mass_list() == (-1, 0)
    assert L.pfr_inertia_sweep(*args) == 5 and b"pfr_set_inertia" in L.pfr_last_error()      # PFR_ERR_STATE
    G = _t(np.ascontiguousarray(ins.G.T))
    w = (4 * _native.C.c_double)(*ins.d)
    for n_mass in (0, 5):
        assert L.pfr_set_inertia(sv._h, n_mass, G.data_ptr(), w) == 1                         # PFR_ERR_ARG
        assert L.pfr_inertia_sweep(*args) == 5
    assert L.pfr_inertia_sweep(sv._h, ft.numel(), ft.data_ptr(), None, None, None, None, None, None) == 1
    assert L.pfr_inertia_sweep(sv._h, 0, ft.data_ptr(), None, None, None, jm.data_ptr(), None, None) == 1
    torch.cuda.synchronize()
    assert torch.isnan(torch.view_as_real(jm)).all()
    sv.set_inertia(G, ins.d)
    bad_axis = (3 * _native.C.c_double)(0.0, 0.0, 0.0)
    assert L.pfr_inertia_sweep(sv._h, ft.numel(), ft.data_ptr(), bad_axis, None, None, jm.data_ptr(), None, None) == 1
    torch.cuda.synchronize()
    assert torch.isnan(torch.view_as_real(jm)).all()
    out = run_inertia(ins, sym, sy.FREQS, mode=RAW, solver=(sv, K))
    check_inertia("A-after-errors", ins, sy.FREQS, out, _bounds(ins, sym, sy.FREQS))
