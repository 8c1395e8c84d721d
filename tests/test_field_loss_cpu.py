"""No GPU: the host side of the field-loss sweep (include/pfr.h, pfr_field_loss_sweep) -- the reference the GPU tests
compare with (tests/synthetic_fieldloss.py) checked against finite differences in extended precision, the fp64 models'
errors the GPU bounds come from, the data's distance from MAC = 1, the Python layer's validation and refusals, and the
C ABI's declaration against the ctypes signature table."""
import os
import re

import numpy as np
import pytest

import synthetic as sy
import synthetic_fieldloss as sf
from helpers import make_problem
from plate_inverse_problem_amd import _native
from plate_inverse_problem_amd.Problem import field_reference, field_selection


# ----------------------------------------------------------------------------- the seeds
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("loss_type", sf.LOSSES)
def test_seed_matches_central_differences(loss_type, weighted):
    """d term = Re(sum_j g_j dx_j): each g against central differences of its term along five random complex
    directions dx, all in extended precision.  Step t = 1e-6: the truncation is O(t^2) = 1e-12 of the third
    derivative's scale, the rounding eps_ld / t = 1e-13; the bound 1e-9 is the one the other finite-difference checks
    of this suite use for the same construction."""
    rng = np.random.default_rng(8500)
    m = 9
    x = (rng.standard_normal(m) + 1j * rng.standard_normal(m)).astype(sy.CLD)
    r = (x * (1 + 0.3 * rng.uniform(-1, 1, m)) * np.exp(1j * rng.uniform(-1, 1, m))).astype(sy.CLD)
    v = sf.weights(m) if weighted else None
    term, g = sf.terms_g(x, r, v, loss_type)
    assert term.dtype == sy.LD and g.dtype == sy.CLD
    t = sy.LD(1e-6)
    worst = 0.0
    for _ in range(5):
        dx = (rng.standard_normal(m) + 1j * rng.standard_normal(m)).astype(sy.CLD)
        fd = (sf.terms_g(x + t * dx, r, v, loss_type)[0] - sf.terms_g(x - t * dx, r, v, loss_type)[0]) / (2 * t)
        an = np.sum(g * dx).real
        worst = max(worst, float(abs(an - fd) / np.sum(np.abs(g * dx))))
    print(f"{loss_type} weighted={weighted}: |Re(g.dx) - fd| / sum|g dx| = {worst:.1e}")
    assert worst <= 1e-9
    # the fp64 form agrees with the extended one to rounding
    t64, g64 = sf.terms_g(x.astype(np.complex128), r.astype(np.complex128), v, loss_type)
    assert g64.dtype == np.complex128
    assert abs(float(t64) - float(term)) <= 1e-14 * abs(float(term))
    assert np.max(np.abs(g64 - g.astype(np.complex128))) <= 1e-14 * np.max(np.abs(g64))
    if weighted:
        assert g[m // 3] == 0                                     # a zero weight: no seed on that row


def test_cotangent_seed_is_the_reference():
    r = np.array([1 + 2j, -3j], dtype=sy.CLD)
    term, g = sf.terms_g(np.zeros(2, dtype=sy.CLD), r, None, "FCOTANGENT")
    assert term == 0 and np.array_equal(g, r)


# ----------------------------------------------------------------------------- w of the reference
@pytest.mark.parametrize("some,weighted", [(False, False), (True, True)], ids=["all-unit", "some-weighted"])
def test_reference_gradient_matches_finite_differences(some, weighted):
    """Re sum_k w_qk d_k of each loss against central differences of the extended-precision terms along a fixed
    complex coefficient direction d, per frequency; step t = 1e-7, 4 frequencies and the bound 1e-9 of
    test_jacobian_cpu / test_complex_response_cpu for the same construction (synthetic_jacobian.fr_at's way of
    perturbing coef).  And FCOTANGENT with the seed of FIELD_MSE as its cotangent gives FIELD_MSE's w."""
    pat, op = sy.case("T", n_stiff=12)
    freqs = np.linspace(40.0, 600.0, 4)
    rows = sf.selection(pat.n, some)
    v = sf.weights(pat.n if rows is None else rows.size) if weighted else None
    fref = sf.reference(op, freqs, rows, v)
    d = sy.direction(1, 12)[0].astype(sy.CLD)
    t = sy.LD(1e-7)
    coef = op.coef.astype(sy.CLD)
    for lt in sf.LOSSES:
        L = fref.loss(lt)
        J = (L["w"] @ d).real
        Jfd = (sf.loss_at(op, freqs, coef + t * d, fref, lt) - sf.loss_at(op, freqs, coef - t * d, fref, lt)) / (2 * t)
        err = float(np.max(np.abs(J - Jfd)) / np.max(np.abs(J)))
        print(f"T some={some} weighted={weighted} {lt}: |J - J_fd| / max|J| = {err:.1e}")
        assert err <= 1e-9
    as_cot = sf.FieldReference(fref.refc, fref.rows, fref.v, fref.data, fref.loss("FIELD_MSE")["g"].astype(np.complex128))
    a, b = as_cot.loss("FCOTANGENT")["w"], fref.loss("FIELD_MSE")["w"]
    assert float(np.max(np.abs(a - b)) / np.max(np.abs(b))) <= 1e-15      # the seed rounded to fp64 on its way


# ----------------------------------------------------------------------------- the data
# (shape, load, the selections the GPU tests use on it: every row / synthetic_fieldloss.selection's partial one).  The
# forest is swept with every row only: a random partial selection of it lies mostly on the unloaded tree, where x = 0,
# and the two or three loaded rows left give a MAC next to 1 (measured here: 1 - MAC = 3e-3)
CASES = [("T", None, (False, True)), ("F0", None, (False, True)), ("A", None, (False, True)), ("AC", (0,), (False,))]


@pytest.mark.parametrize("shape,load,somes", CASES, ids=[c[0] for c in CASES])
def test_one_minus_mac_is_no_cancellation(shape, load, somes):
    """The GPU tests' data (true field x (1 + 0.3 xi) e^{i phi} per row) keeps 1 - MAC >= 1e-2 at every frequency of
    every selection they use: the FIELD_MAC term loses no more than two digits to the subtraction."""
    pat, op = sy.case(shape, **({} if load is None else {"load": load}))
    for some in somes:
        rows = sf.selection(pat.n, some)
        n_sel = pat.n if rows is None else rows.size
        for v in (None, sf.weights(n_sel)):
            fref = sf.reference(op, sy.FREQS, rows, v)
            m = fref.min_one_minus_mac()
            print(f"{shape} n_sel={n_sel} weighted={v is not None}: min (1 - MAC) = {m:.3f}")
            assert m >= 1e-2
            r2 = (np.abs(fref.data) ** 2 * (1.0 if v is None else v)).sum(axis=1)
            assert np.all(r2 > 0)


def test_edge_selections():
    """The tile-edge selections of the GPU tests on shape A: distinct, descending, holding the Dirichlet rows, and (but
    for the single row, where MAC = 1 identically and FIELD_MAC is not run) 1 - MAC >= 1e-2 over the 65 frequencies."""
    pat, op = sy.case("A")
    d = np.asarray(pat.dirichlet)
    assert d.size >= 2 and max(sf.EDGE_SIZES) < pat.n
    for k in sf.EDGE_SIZES + (pat.n,):
        rows = sf.edge_selection(pat, k)
        assert rows.size == k and np.all(np.diff(rows) < 0) and rows.dtype == np.int32
        assert np.all(np.isin(d, rows)) if k > 1 else (rows[0] == d[0] and op.rhs[d[0]] != 0)
        fref = sf.reference(op, sy.FREQS[:65], rows, None)
        assert np.all((np.abs(fref.data) ** 2).sum(axis=1) > 0)
        if k > 1:
            m = fref.min_one_minus_mac()
            print(f"A edge selection of {k}: min (1 - MAC) = {m:.3f}")
            assert m >= 1e-2


# ----------------------------------------------------------------------------- the models
@pytest.mark.parametrize("refine", [False, True], ids=["mode3", "mode7"])
def test_model_errors_sit_at_rounding_level(refine):
    """e_model and e_dense of shape A on a four-frequency sample, selection and weights on: recorded, and at the level
    cond x eps allows (cond_2 <= 1e4 by construction, eps 1.1e-16, a few hundred roundings: 1e-10 with two digits to
    spare); the GPU bounds are 10 x the larger of them."""
    pat, op = sy.case("A")
    sym = sy.symbolic("A")
    freqs = sy.FREQS[[0, 43, 86, 129]]
    rows = sf.selection(pat.n, True)
    got = sf.model_errors(op, sym, freqs, rows, sf.weights(rows.size), refine=refine)
    for lt, (em, ed) in got.items():
        print(f"A refine={refine} {lt}: e_model " + " ".join(f"{k}={x:.1e}" for k, x in sorted(em.items())) +
              " | e_dense " + " ".join(f"{k}={x:.1e}" for k, x in sorted(ed.items())))
        assert set(em) == set(ed) == ({"w", "lam"} if lt == "FCOTANGENT" else {"w", "lam", "loss"})
        assert max(em.values()) <= 1e-10 and max(ed.values()) <= 1e-10


# ----------------------------------------------------------------------------- the plate's CPU adjoint
@pytest.mark.parametrize("loss_type", sf.LOSSES)
def test_oracle_adjoint_matches_finite_differences(loss_type):
    """tests/field_loss_oracle.py -- the adjoint the GPU plate test compares with -- against 4th-order central
    differences of the oracle field loss, as tests/test_oracle.py checks the oracle's own adjoint: 1e-4 of the
    largest entry (the differences' truncation in the loss factor).  Vertex rows of w, non-uniform weights."""
    import field_loss_oracle as fo
    from helpers import oracle_for
    p = make_problem("orthotropic", ny=3)
    o = oracle_for(p)
    freqs = np.linspace(60.0, 560.0, 9)
    rows = p.vertex_rows()[2]
    v = sf.weights(rows.size)
    data = sf.make_data(o.solutions(freqs, p.parameters)[:, rows])
    th = p.parameters * np.array([1.1, 0.95, 1.2, 1.05, 1.3])
    L, g = fo.field_loss_and_grad(o, freqs, data, loss_type, th, rows, v)
    gfd = fo.fd_grad(o, freqs, data, loss_type, th, rows, v)
    err = float(np.max(np.abs(g - gfd)) / np.max(np.abs(gfd)))
    print(f"oracle {loss_type}: loss {L:.6e}, |g - g_fd| / max|g_fd| = {err:.1e}")
    assert abs(L - fo.field_loss(o, freqs, data, loss_type, th, rows, v)) <= 1e-12 * abs(L)
    assert err < 1e-4


# ----------------------------------------------------------------------------- the Python layer
def test_reference_validation():
    ref = np.ones((3, 4), dtype=np.complex128)
    out, v = field_reference(ref, 3, 4)
    assert out.dtype == np.complex128 and out.flags.c_contiguous and v is None
    assert field_reference(ref, 3, 4, [0, 1, 0, 2.5])[1].dtype == np.float64
    bad = [
        (np.ones((4, 3)), None, "shape"), (np.ones(12), None, "shape"),
        (np.where(np.arange(12).reshape(3, 4) == 5, np.nan, 1.0), None, "finite"),
        (np.where(np.arange(12).reshape(3, 4) == 0, np.inf, 1.0), None, "finite"),
        (np.where(np.arange(3)[:, None] == 1, 0.0, 1.0) * ref, None, "frequency 1"),
        (ref, [1, 1, 1], "weights"), (ref, [1, -1, 1, 1], "negative"), (ref, [1, np.nan, 1, 1], "finite"),
        (ref, [0, 0, 0, 0], "zero"),
        # a reference that lives only where the weights are zero
        (ref * np.array([1, 0, 0, 0]), [0, 1, 1, 1], "frequency 0"),
    ]
    for r, w, word in bad:
        with pytest.raises(ValueError, match=word):
            field_reference(r, 3, 4, w)


def test_selection_validation():
    assert field_selection(None, 10) is None
    rows = field_selection([9, 0, 4], 10)
    assert rows.dtype == np.int32 and rows.tolist() == [9, 0, 4]
    for bad, word in (([], "non-empty"), ([0.5], "integer"), ([10], "outside"), ([-1], "outside"), ([3, 4, 3], "twice")):
        with pytest.raises(ValueError, match=word):
            field_selection(bad, 10)


def test_field_loss_requests_are_checked_on_the_host():
    """Every refusal comes before a device is touched (this test has none)."""
    p = make_problem("orthotropic", ny=3)
    n = p.mat_size
    freqs = [100.0, 200.0]
    ref = np.ones((2, n), dtype=np.complex128)
    with pytest.raises(ValueError, match="not a field loss"):
        p.getFieldLossFunction(freqs, ref, "MSE")
    with pytest.raises(ValueError, match="shape"):
        p.getFieldLossFunction(freqs, ref[:, :5], "FIELD_MSE")
    with pytest.raises(ValueError, match="twice"):
        p.getFieldLossFunction(freqs, ref[:, :2], "FIELD_MAC", dofs=[1, 1])
    with pytest.raises(ValueError, match="zero"):
        p.getFieldLossFunction(freqs, ref * 0, "FIELD_RMSE")
    with pytest.raises(ValueError, match="no frequencies"):
        p.getFieldLossFunction([], ref[:0], "FIELD_MSE")
    with pytest.raises(ValueError, match="twice"):
        p.getFieldFunction(dofs=[0, 2, 0])
    x0 = np.asarray(p.parameters)
    with pytest.raises(ValueError, match="ref_field"):
        p.solveInverse(x0, "FIELD_MAC", "lbfgs", report=False, log=False)
    with pytest.raises(ValueError, match="FIELD_"):
        p.solveInverse(x0, "MSE", "lbfgs", ref_fr=(freqs, [1.0, 1.0]), ref_field=(freqs, ref), report=False, log=False)
    kw = dict(ref_field=(freqs, ref), report=False, log=False)
    for opt, extra, why in (("tr", {}, "Hessian"), ("lm", {}, "Jacobian"), ("de", {"vectorized": True}, "population"),
                            ("lbfgs", {"distributed": True}, "distributed"),
                            ("gd", {"compression": (True, 2)}, "compression")):
        with pytest.raises(NotImplementedError, match=why):
            p.solveInverse(x0, "FIELD_MSE", opt, **kw, **extra)


# ----------------------------------------------------------------------------- the C ABI's declaration
def _declared_arity(name):
    with open(_native.HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"PFR_API\s+[\w\s\*]+?\b" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m, name + " is not declared in include/pfr.h"
    return len(m.group(1).strip().split(","))


def test_header_and_signature_table_agree():
    assert "pfr_field_loss_sweep" in _native.header_symbols()
    assert _declared_arity("pfr_field_loss_sweep") == 15 == len(_native._PROTOS["pfr_field_loss_sweep"][1])
    with open(_native.HEADER_PATH) as f:
        txt = f.read()
    for name, val in (("FMSE", 32), ("FRMSE", 33), ("FMAC", 34), ("FCOTANGENT", 35)):
        assert re.search(rf"#define PFR_LOSS_{name} {val}\b", txt), name
        assert getattr(_native, "LOSS_" + name) == val == sf.LOSS_ID.get("FIELD_" + name[1:], sf.LOSS_ID["FCOTANGENT"])
    assert _native.FIELD_LOSS_IDS == {k: sf.LOSS_ID[k] for k in sf.LOSSES}
    # the sums per tile that size the partial buffer: the Python table against launch.hpp's field_nsum
    with open(os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc", "launch.hpp")) as f:
        nsum = dict(re.findall(r"loss == PFR_LOSS_(\w+) \? (\d)", f.read()))
    assert {"FIELD_" + k[1:]: int(v) for k, v in nsum.items()} == _native.FIELD_LOSS_SUMS
    assert not set(_native.FIELD_LOSS_IDS.values()) & (set(_native.LOSS_IDS.values()) |
                                                       set(_native.COMPLEX_LOSS_IDS.values()))
    from plate_inverse_problem_amd.Problem import _LANE_CALLS, _Engine
    assert _LANE_CALLS["field_loss", False] == ("field_loss_sweep", None)
    assert callable(_native.Solver.field_loss_sweep) and callable(_Engine.field_loss_step)
    flat = " ".join(txt.split()).replace(" * ", " ")
    for limit in ("the field Jacobian and covariance", "the Hessian", "population and distributed forms",
                  "a correction of the field loss", "magnitude-only field data"):
        assert limit in flat, limit


def test_symbol_resolves_when_the_library_loads():
    import ctypes
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libpfr.so is not built")
    # the one excuse for not loading is a machine without the HIP runtime, decided before the project's own library
    # is tried: an undefined symbol or a broken link of libpfr.so is an OSError too, and must fail
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in ("libamdhip64.so", os.path.join(rocm, "lib", "libamdhip64.so")):
        try:
            ctypes.CDLL(cand)
            break
        except OSError:
            continue
    else:
        pytest.skip("no HIP runtime (libamdhip64.so) on this machine")
    L = _native.lib()
    # refused before anything touches a device: a null solver
    assert L.pfr_field_loss_sweep(None, 1, None, 0, None, None, 32, None, 1.0, None, None, None, None, 0, None) == 1
