"""GPU: pfr_combine_batch and pfr_population_sweep on the synthetic fronts (tests/synthetic_population.py).

The main check is bitwise and has no tolerance: at the lanes of member p the population sweep gives the fr, the jc
rows, the flags and the backward errors of the existing pfr_jacobian_sweep run with theta_p set the ordinary way over
the same lanes on a solver of the same max_batch (same lane count, same chunking, same launch forms; the padded lanes
included).  One member is also compared with the extended-precision reference of its own operator, at the bound of
test_gpu_synthetic_jacobian.py, so the file is not only self-referential.

The forward sweep (jc NULL) is compared with its own twin, the single-theta forward pfr_sweep.  Its fr equals the jc
run's fr bitwise where both runs form fr the same way: under the functional correction (the default mode) and on a
general analysis; on a symmetric analysis in the raw mode a reverse sweep takes fr from the bottom-up dot products
and a forward sweep from the solution, in pfr_sweep as here, so that case is checked in the default mode.
"""
import numpy as np
import pytest
import torch

import synthetic as sy
import synthetic_jacobian as sj
import synthetic_population as sp
from plate_inverse_problem_amd import _native
from test_gpu_synthetic import DEFAULT, RAW, _t, make_solver, run_sweep
from test_gpu_synthetic_jacobian import _jac_bounds, _same

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KW = dict(make_solver=make_solver, t=_t)
# (members, frequencies per member, max_batch): 3 x 130 (Fpad 192) in chunks of 64 -- nine chunks, the member changes
# at chunk boundaries; 5 x 40 (Fpad 64) in chunks of 128 -- two members inside one chunk and a last chunk of one
# group below Fc, whose second group lies past the caller's table
LAYOUTS = {"3x130-b64": (3, sy.FREQS, 64), "5x40-b128": (5, sy.FREQS[:40], 128)}


def _slot(shape, layout, mode, symmetric=True, n_stiff=12, order=None, jac=True):
    P, freqs, mb = LAYOUTS[layout] if isinstance(layout, str) else layout
    base, ops = sp.members(shape, P, n_stiff)
    sym = sy.symbolic(shape, symmetric=symmetric)
    f, member, valid = sp.lanes(P, freqs, order)
    pop = sp.run_population(base, ops, sym, f, member, max_batch=mb, mode=mode, jac=jac, **KW)
    for p, op in enumerate(ops):
        assert np.array_equal(pop["Kpop"][p], op.K)                           # pfr_combine_batch: exact by construction
    nlane = f.size
    assert np.isnan(pop["fr"][nlane]) and (pop["jc"] is None or np.isnan(pop["jc"][nlane].view(np.float64)).all()), \
        "a lane past the sweep stored its results"
    assert not np.isnan(pop["fr"][:nlane]).any()
    assert pop["jc"] is None or not np.isnan(pop["jc"][:nlane].view(np.float64)).any()
    assert np.all(pop["flags"] == 0)
    for p, op in enumerate(ops):
        one = sp.run_member(op, sym, f, max_batch=mb, mode=mode, jac=jac, **KW)
        sel = np.repeat(member == p, 64)
        assert sel.sum() == nlane // P
        sp.same_lanes(pop, one, sel)
    return pop, (f, member, valid), ops, sym


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("shape", ["A", "F0", "T"])
def test_member_lanes_equal_the_single_theta_jacobian_sweep(shape, layout, mode):
    """T: every kernel class and the level chain; F0: k_front0; A: the SMALL off-diagonal forms.  All three have
    Dirichlet nodes (k_dirichlet_rhs / k_dirichlet_post)."""
    _slot(shape, layout, mode)


def test_one_chunk_of_2048_lanes():
    """2 members x 1,024 frequencies in one chunk of 2,048 lanes: the wide launches (the L21 kernel without the
    pipelined prefix, the bottom-up chain without the right-looking pivot blocks), two members inside the chunk."""
    _slot("T", (2, np.linspace(40.0, 600.0, 1024), 2048), DEFAULT)


ROUTES = [("T", {"PFR_CONTRACT_WALK": "0"}), ("T", {"PFR_SCALE_CORR": "0"}), ("T", {"PFR_FN_DOT": "0"}),
          ("T", {"PFR_LS_RL": "0"}), ("T", {"PFR_US2_NAR": "0"}), ("F0", {"PFR_FRONT0": "0"})]


@pytest.mark.parametrize("shape,env", ROUTES, ids=[",".join(f"{k[4:]}={v}" for k, v in e.items()) for _, e in ROUTES])
def test_launch_routes(shape, env, monkeypatch):
    """The knobs (read when a solver is created, so both sweeps take the same route) that select the other
    instantiations: the walk without the contraction, the unscaled finish, the functional from the solution (the
    single-slice bottom-up solves, RHS 5), the left-looking and the wide forms of the bottom-up chain, and level 0
    through the four class kernels."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _slot(shape, "5x40-b128", DEFAULT)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_member_order_permuted(layout):
    """The members moved to other lane blocks: each member's rows are the same bits."""
    P, freqs, _ = LAYOUTS[layout]
    a, (_, ma, _), _, _ = _slot("T", layout, DEFAULT)
    order = np.roll(np.arange(P), 2)
    b, (_, mb, _), _, _ = _slot("T", layout, DEFAULT, order=order)
    for p in range(P):
        sa, sb = np.repeat(ma == p, 64), np.repeat(mb == p, 64)
        assert not np.array_equal(sa, sb)
        for k in ("fr", "jc", "berr"):
            x, y = (a[k][:-1], b[k][:-1]) if k != "berr" else (a[k], b[k])
            assert np.array_equal(x[sa], y[sb], equal_nan=True), (p, k)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_forward_sweep_equals_the_single_theta_forward_sweep(layout, mode):
    """jc NULL: the forward sweep (unpaired solves in the raw mode: k_lsolve_level's population forms)."""
    _slot("T", layout, mode, jac=False)


@pytest.mark.parametrize("symmetric,mode", [(True, DEFAULT), (False, RAW), (False, DEFAULT)],
                         ids=["symmetric-default", "general-raw", "general-default"])
def test_forward_sweep_fr_equals_the_jacobian_run(symmetric, mode):
    """jc NULL: fr equals the jc run's fr, bitwise (see the module docstring for the modes)."""
    P, freqs, mb = LAYOUTS["5x40-b128"]
    base, ops = sp.members("T", P)
    sym = sy.symbolic("T", symmetric=symmetric)
    f, member, _ = sp.lanes(P, freqs)
    a = sp.run_population(base, ops, sym, f, member, max_batch=mb, mode=mode, jac=True, **KW)
    b = sp.run_population(base, ops, sym, f, member, max_batch=mb, mode=mode, jac=False, solver=a["solver"], **KW)
    assert np.array_equal(a["fr"], b["fr"], equal_nan=True)
    assert np.array_equal(a["flags"], b["flags"])


@pytest.mark.parametrize("correct", [0, _native.PFR_CHECK_CORRECT], ids=["mode7", "mode15"])
def test_refined_sweep(correct):
    """PFR_CHECK_REFINE on A: the unpaired solves with one refinement step each (the Dirichlet and residual kernels'
    vector forms)."""
    _slot("A", "5x40-b128", RAW | _native.PFR_CHECK_REFINE | correct)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_general_analysis(mode):
    _slot("T", "5x40-b128", mode, symmetric=False)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_18_stiffness_matrices(mode):
    _slot("T", "5x40-b128", mode, n_stiff=18)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_member_against_the_reference(mode):
    """Member 1 on T against sy.reference of that member's operator, at 10 x max(e_model, e_dense, 1e-14) with the
    model run for that member here (the bound of test_gpu_synthetic_jacobian.py)."""
    P, freqs, mb = LAYOUTS["3x130-b64"]
    base, ops = sp.members("T", P)
    sym = sy.symbolic("T")
    f, member, valid = sp.lanes(P, freqs)
    pop = sp.run_population(base, ops, sym, f, member, max_batch=mb, mode=mode, **KW)
    sel = np.repeat(member == 1, 64) & valid
    op = ops[1]
    refc = sy.reference(op, freqs)
    b, em, ed = _jac_bounds(op, sym, freqs, correct=bool(mode & _native.PFR_CHECK_CORRECT))
    err = {"jc": sj.row_errors(pop["jc"][:-1][sel], sj.jacobian_reference(refc)),
           "fr": float(np.max(np.abs(pop["fr"][:-1][sel].astype(sy.LD) / refc.fr - 1)))}
    print(f"T member 1 mode {mode}: " + " ".join(f"{k}={v:.2e}/{b[k]:.1e}" for k, v in err.items()))
    assert np.all(np.isfinite(pop["berr"][sel])) and pop["berr"][sel].max() <= sy.BERR_MAX
    for k, v in err.items():
        assert v <= b[k], (k, v, b[k], em[k], ed[k])


# ----------------------------------------------------------------------------- state
def _population_between(solver, mode):
    P, freqs, _ = LAYOUTS["3x130-b64"]
    base, ops = sp.members("T", P)
    f, member, _ = sp.lanes(P, freqs)
    sp.run_population(base, ops, sy.symbolic("T"), f, member, max_batch=64, mode=mode, solver=solver, **KW)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_loss_sweep_is_unchanged_by_a_population_sweep_between(mode):
    """A loss sweep, a population sweep, the same loss sweep again on one solver: bit-identical."""
    _, op = sy.case("T")
    sym = sy.symbolic("T")
    first = run_sweep(op, sym, sy.FREQS, mode=mode, vectors=False)
    _population_between(first["solver"], mode)
    second = run_sweep(op, sym, sy.FREQS, mode=mode, vectors=False, solver=first["solver"])
    _same(first, second)


@pytest.mark.parametrize("mode", [RAW, DEFAULT], ids=["raw", "default"])
def test_loss_sweep_graph_is_not_replayed_past_a_population_sweep(mode, monkeypatch):
    """PFR_GRAPH=1: three loss sweeps with the same arguments (the third replayed from the graph), the population
    sweep, then the same loss sweep: bit-identical and run directly.  On a stream of its own (the default stream
    cannot be captured)."""
    monkeypatch.setenv("PFR_GRAPH", "1")
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        _, op = sy.case("T")
        sym = sy.symbolic("T")
        first = run_sweep(op, sym, sy.FREQS, mode=mode, vectors=False)
        sv, _ = first["solver"]
        nf = sy.FREQS.size
        berr = torch.full((nf, 2), float("nan"), dtype=torch.float64, device=DEV)
        ft, rt = _t(sy.FREQS), torch.view_as_real(_t(first["refc"].ref))
        fr = torch.zeros(nf, dtype=torch.float64, device=DEV)
        loss = torch.zeros(1, dtype=torch.float64, device=DEV)
        w = torch.zeros(op.n_stiff, dtype=torch.complex128, device=DEV)
        flags = torch.zeros(nf, dtype=torch.int32, device=DEV)

        def sweep():
            sv.set_check(mode, sy.BERR_MAX, berr)
            loss.zero_()
            w.zero_()
            flags.zero_()
            sv.sweep(ft, _native.LOSS_MSE_LOG_AFC, ref=rt, scale=first["scale"], fr=fr, loss=loss,
                     w=torch.view_as_real(w), flags=flags)
            torch.cuda.synchronize()
            return dict(fr=fr.cpu().numpy(), loss=float(loss.cpu()[0]), w=w.cpu().numpy(), berr=berr.cpu().numpy(),
                        flags=flags.cpu().numpy())

        for _ in range(3):
            before = sweep()
        replayed = sv.graph_launches()
        assert replayed >= 1
        _same(first, before)
        _population_between(first["solver"], mode)
        after = sweep()
        assert sv.graph_launches() == replayed
        _same(before, after)


# ----------------------------------------------------------------------------- errors
def _refused(mode, nlane, member, n_members=3):
    base, ops = sp.members("T", 3)
    sv, _ = make_solver(base, sy.symbolic("T"), 64)
    Kpop = torch.zeros((3, base.pat.nnz), dtype=torch.complex128, device=DEV)
    sv.set_check(mode, sy.BERR_MAX, None)
    fr = torch.full((256,), float("nan"), dtype=torch.float64, device=DEV)
    jc = torch.full((256, base.n_stiff), complex(float("nan"), float("nan")), dtype=torch.complex128, device=DEV)
    with pytest.raises(_native.NativeError):
        sv.population_sweep(_t(np.resize(sy.FREQS, nlane)), np.asarray(member, dtype=np.int32),
                            torch.view_as_real(Kpop), np.ones(n_members, dtype=np.complex128), fr,
                            jc=torch.view_as_real(jc))
    torch.cuda.synchronize()
    assert torch.isnan(fr).all() and torch.isnan(torch.view_as_real(jc)).all(), "a refused sweep wrote its outputs"


def test_selective_refinement_is_refused():
    _refused(DEFAULT | _native.PFR_CHECK_REFINE_ADJ, 128, [0, 1])


@pytest.mark.parametrize("member", [[0, 3], [-1, 0]], ids=["past-the-end", "negative"])
def test_member_index_out_of_range_is_refused(member):
    _refused(DEFAULT, 128, member)


def test_lane_count_not_a_multiple_of_64_is_refused():
    _refused(DEFAULT, 65, [0, 1])
