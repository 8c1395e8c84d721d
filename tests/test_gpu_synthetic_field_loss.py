"""GPU: pfr_field_loss_sweep (include/pfr.h) through the C ABI on the synthetic fronts of tests/synthetic.py, chunks of
64 -- a loss on the solution's rows against full-field data, its adjoint seed written into G by k_field_terms /
k_field_finish / k_field_seed, the adjoint over every front and the contraction.

What is asserted, and against what (tests/synthetic_fieldloss.py: the extended-precision reference; every bound is
10 x max(e_model, e_dense, synthetic.FLOOR) of the fp64 multifrontal model and the unrefined dense LU on a sample of
the sweep's frequencies -- from the CPU, never from the GPU):
  accuracy      T, F0, A at synthetic.FREQS, modes 3 and 7, the three losses and FCOTANGENT, every row and a partial
                selection, unit and non-uniform weights: the loss sum and w over the 130 frequencies, and the adjoint
                (pfr_debug_solution(1, lane)) of a three-frequency sweep at the first, middle and last of them
  edges         selections of 1, 31, 32, 33, 65 and n rows (descending, holding the Dirichlet rows) at 1, 63, 64 and 65
                frequencies: the call with the list and the all-rows call with 0 / 1 weights marking it, both within
                the bound of the same reference.  Not bit for bit: a tile sums its rows in the order the waves take
                them and the tiles are added in ascending order, so where a row falls changes the rounding
                (DESIGN.md section 5.5).  The explicit list 0 .. n - 1 gives the bits of the NULL list
  consistency   FCOTANGENT with the seed of FIELD_MSE (formed on the host from a field sweep's out) gives FIELD_MSE's w
  field output  out_dev given: the bits of pfr_field_sweep in the same mode; NaN-patterned guard bands around out, ref
                and w stay intact; loss and w are the bits of the call without out
  pruning       forest AC with C unloaded: loss and w bit for bit those of pfr_set_prune(0); XA on C's rows exact +0.0
                after the pruned sweep of every loss, FCOTANGENT's seed on C included, although a completed
                cotangent adjoint had filled them just before (read with pruning switched off after the sweep: the
                views are dropped, XA stays, the accessor completes nothing); the whole adjoint from the accessor
                (which completes the unloaded tree for the seed left in G) within the bound; the next pruned loss
                sweep the bits of a fresh solver's
  variants      a general analysis, 18 matrices, and modes 11 / 27 giving the bits of mode 3
  neighbours    a loss sweep after the field-loss sweep is bit-identical to one without it, also with PFR_GRAPH=1
  refusals      every PFR_ERR_ARG / PFR_ERR_STATE of the header, each leaving the next call unharmed
"""
import ctypes as C

import numpy as np
import pytest
import torch

import synthetic as sy
import synthetic_fieldloss as sf
from helpers import report
from plate_inverse_problem_amd import _native
from test_gpu_synthetic import DEFAULT, DEV, RAW, _t, make_solver, run_sweep
from test_gpu_synthetic_field import GUARD, NAN_BITS, _bits, _same_loss, run_field, same_bits

pytestmark = pytest.mark.gpu
REFINE = _native.PFR_CHECK_REFINE
ERR_ARG, ERR_STATE = 1, 5


def _guarded(n_doubles, fill=None):
    """A float64 device buffer of n_doubles between two guard bands of one NaN bit pattern: (whole, inner view)."""
    whole = torch.as_tensor(np.full(n_doubles + 4 * GUARD, NAN_BITS).view(np.float64), device=DEV)
    inner = whole[2 * GUARD:2 * GUARD + n_doubles]
    if fill is not None:
        inner.copy_(torch.as_tensor(np.ascontiguousarray(fill).view(np.float64).reshape(-1), device=DEV))
    return whole, inner


def _guards_intact(whole, n_doubles):
    host = _bits(whole.cpu().numpy())
    return bool(np.all(host[:2 * GUARD] == NAN_BITS) and np.all(host[2 * GUARD + n_doubles:] == NAN_BITS))


def run_floss(sv, freqs, ref, loss_type, rows=None, weights=None, mode=RAW, scale=None, want_out=False, fresh=False,
              prefill=(0.0, 0.0)):
    """One pfr_field_loss_sweep; ref, w and (when asked) out inside guard bands that are checked.  Returns the
    results on the host."""
    nf = len(freqs)
    n_sel = sv.sym.n if rows is None else len(rows)
    n_stiff = sv_n_stiff(sv)
    assert ref.shape == (nf, n_sel)
    berr = torch.full((nf, 2), float("nan"), dtype=torch.float64, device=DEV)
    sv.set_check(mode, sy.BERR_MAX, berr)
    scale = 1.0 / nf if scale is None else scale
    ref_whole, ref_in = _guarded(2 * nf * n_sel, ref.astype(np.complex128))
    w_whole, w_in = _guarded(2 * n_stiff, np.full(n_stiff, prefill[1], dtype=np.complex128))
    out_whole, out_in = _guarded(2 * nf * n_sel) if want_out else (None, None)
    loss = torch.full((1,), prefill[0], dtype=torch.float64, device=DEV)
    flags = torch.zeros(nf, dtype=torch.int32, device=DEV)
    sv.field_loss_sweep(_t(freqs), sf.LOSS_ID[loss_type], ref_in, w_in, rows=rows, weights=weights, scale=scale,
                        out=out_in, loss=loss, flags=flags, fresh=fresh)
    torch.cuda.synchronize()
    sv.set_check(mode, sy.BERR_MAX)
    assert _guards_intact(ref_whole, 2 * nf * n_sel), "guard band of ref written"
    assert same_bits(ref_in.cpu().numpy().view(np.complex128).reshape(nf, n_sel), ref.astype(np.complex128))
    assert _guards_intact(w_whole, 2 * n_stiff), "guard band of w written"
    res = dict(loss=float(loss.cpu()[0]), w=w_in.cpu().numpy().view(np.complex128), flags=flags.cpu().numpy(),
               berr=berr.cpu().numpy(), scale=scale)
    if want_out:
        assert _guards_intact(out_whole, 2 * nf * n_sel), "guard band of out written"
        res["out"] = out_in.cpu().numpy().view(np.complex128).reshape(nf, n_sel)
        assert not np.any(_bits(res["out"]) == NAN_BITS), "an entry of out was not written"
    return res


def sv_n_stiff(sv):
    return int(sv._keep["stiff"].shape[1])                      # the (nnz, n_stiff) tensor make_solver set


solver_for = make_solver


def adjoints(sv, lanes):
    return {q: sv.debug_solution(1, q) for q in lanes}


def raw_adjoints(sv, lanes):
    """pfr_debug_solution(1, lane) through the C ABI directly, (len(lanes), n) complex: the doubles as the accessor
    wrote them (Solver.debug_solution adds the parts, which turns a -0.0 into +0.0)."""
    raw = np.zeros((len(lanes), 2 * sv.sym.n), dtype=np.float64)
    for i, lane in enumerate(lanes):
        _native.check(_native.lib().pfr_debug_solution(sv._h, 1, lane, raw[i].ctypes.data_as(C.POINTER(C.c_double))),
                      "pfr_debug_solution")
    return raw.view(np.complex128)


_BOUNDS = {}


def fbounds(op, sym, freqs, rows, v, refine=False, symmetric=True, every=False, loss_types=sf.ALL):
    """{loss_type: bound per quantity} for a sweep over ``freqs``: the models on its sample (all of a short one)."""
    key = (id(op), id(sym), np.asarray(freqs).tobytes(), None if rows is None else rows.tobytes(),
           None if v is None else v.tobytes(), refine, symmetric, tuple(loss_types))
    if key not in _BOUNDS:
        sel = list(range(len(freqs))) if every or len(freqs) <= 4 else sf.model_sample(len(freqs))
        me = sf.model_errors(op, sym, np.asarray(freqs)[sel], rows, v, loss_types=tuple(loss_types),
                             symmetric=symmetric, refine=refine)
        _BOUNDS[key] = {lt: sf.bounds(*e) for lt, e in me.items()}
    return _BOUNDS[key]


def check_floss(name, fref, lt, got, bound, lam=None, lam_sel=None):
    """The loss sum and w of a sweep over all of fref's frequencies against the reference (and the adjoints ``lam`` of
    the frequencies ``lam_sel`` of another, shorter sweep's reference, checked by the caller)."""
    every = np.arange(fref.refc.freqs.size)
    # the device's loss carries scale; the reference's terms do not
    err = sf.errors(fref, lt, every, terms=None if lt == "FCOTANGENT" else [got["loss"] / got["scale"]], w=got["w"],
                    scale=got["scale"])
    be = got["berr"]
    print(name, lt, " ".join(f"{k}={v:.2e}/{bound[k]:.1e}" for k, v in sorted(err.items())),
          f"berr={np.nanmax(be):.1e}")
    report("field_loss::" + name + "::" + lt, berr=float(np.nanmax(be)), **err)
    assert np.all(got["flags"] == 0), got["flags"]
    assert np.all(np.isfinite(be)) and be.max() <= sy.BERR_MAX, be.max()      # forward and adjoint checked
    for k, v in err.items():
        assert v <= bound[k], (name, lt, k, v, bound[k])
    return err


# ----------------------------------------------------------------------------- accuracy
VARIANTS = [(False, False), (False, True), (True, False), (True, True)]


@pytest.mark.parametrize("some,weighted", VARIANTS, ids=["all-unit", "all-weighted", "some-unit", "some-weighted"])
@pytest.mark.parametrize("mode", [RAW, RAW | REFINE], ids=["mode3", "mode7"])
@pytest.mark.parametrize("shape", ["T", "F0", "A"])
def test_accuracy(shape, mode, some, weighted):
    pat, op = sy.case(shape)
    sym = sy.symbolic(shape)
    rows = sf.selection(pat.n, some)
    n_sel = pat.n if rows is None else rows.size
    v = sf.weights(n_sel) if weighted else None
    refine = bool(mode & REFINE)
    fref = sf.reference(op, sy.FREQS, rows, v)
    bound = fbounds(op, sym, sy.FREQS, rows, v, refine=refine)
    three = sy.three(sy.FREQS)
    f3 = sy.FREQS[three]
    fref3 = sf.reference(op, f3, rows, v)
    bound3 = fbounds(op, sym, f3, rows, v, refine=refine)
    sv, _ = solver_for(op, sym)
    for lt in sf.ALL:
        wt = fref.weights_for(lt)
        got = run_floss(sv, sy.FREQS, fref.sweep_ref(lt), lt, rows=rows, weights=wt, mode=mode)
        assert bound[lt]["w"] >= 10 * sy.FLOOR
        check_floss(f"{shape}-mode{mode}-{n_sel}{'w' if weighted else ''}", fref, lt, got, bound[lt])
        if lt == "FCOTANGENT":
            assert got["loss"] == 0.0                                          # left alone
        # the adjoint itself: a sweep over the first, middle and last frequency, every lane read back
        g3 = run_floss(sv, f3, fref3.sweep_ref(lt), lt, rows=rows, weights=wt, mode=mode)
        lam = adjoints(sv, range(3))
        e3 = sf.errors(fref3, lt, [0, 1, 2], terms=None if lt == "FCOTANGENT" else [g3["loss"] / g3["scale"]],
                       w=g3["w"], lam=lam, scale=g3["scale"])
        print(f"   three: " + " ".join(f"{k}={x:.2e}/{bound3[lt][k]:.1e}" for k, x in sorted(e3.items())))
        for k, x in e3.items():
            assert x <= bound3[lt][k], (shape, mode, lt, k, x, bound3[lt][k])


# ----------------------------------------------------------------------------- edges of the transpose and of the partials
@pytest.mark.parametrize("nfreq", [1, 63, 64, 65])
def test_tile_and_chunk_edges(nfreq):
    pat, op = sy.case("A")
    sym = sy.symbolic("A")
    sv, _ = solver_for(op, sym)
    n = pat.n
    assert _native.field_tile_rows() == 32 and 65 < n
    freqs = sy.FREQS[:nfreq]
    for k in sf.EDGE_SIZES + (n,):
        rows = sf.edge_selection(pat, k)
        fref = sf.reference(op, freqs, rows, None)
        # MAC of a single row is 1 identically: the term is all cancellation and its seed zero -- not run, not modelled
        losses = tuple(lt for lt in sf.ALL if not (lt == "FIELD_MAC" and k == 1))
        bound = fbounds(op, sym, freqs, rows, None, loss_types=losses)
        mask = np.zeros(n)
        mask[rows] = 1.0
        full_ref = np.zeros((nfreq, n), dtype=np.complex128)
        for lt in losses:
            sub = run_floss(sv, freqs, fref.sweep_ref(lt), lt, rows=rows)
            check_floss(f"edge-{nfreq}x{k}", fref, lt, sub, bound[lt])
            # the same loss as an all-rows call: 0 / 1 weights mark the selection (FCOTANGENT: a zero cotangent elsewhere)
            full_ref[:] = 0
            full_ref[:, rows] = fref.sweep_ref(lt)
            if lt == "FCOTANGENT":
                full = run_floss(sv, freqs, full_ref, lt)
            else:
                # off the selection the data is irrelevant under a zero weight: give it finite, non-zero values
                full_ref[:, mask == 0] = 0.5 - 0.25j
                full = run_floss(sv, freqs, full_ref, lt, weights=mask)
            check_floss(f"edge-{nfreq}x{k}-masked", fref, lt, full, bound[lt])
    # the explicit list of every row in order is the NULL list, bit for bit
    fall = sf.reference(op, freqs, None, None)
    for lt in ("FIELD_MSE", "FIELD_MAC"):
        a = run_floss(sv, freqs, fall.data, lt)
        b = run_floss(sv, freqs, fall.data, lt, rows=np.arange(n, dtype=np.int32))
        assert np.float64(a["loss"]).view(np.uint64) == np.float64(b["loss"]).view(np.uint64)
        assert same_bits(a["w"], b["w"])


# ----------------------------------------------------------------------------- consistency, the field output
@pytest.mark.parametrize("mode", [RAW, RAW | REFINE], ids=["mode3", "mode7"])
def test_cotangent_of_the_mse_seed_and_the_field_output(mode):
    pat, op = sy.case("T")
    sym = sy.symbolic("T")
    rows = sf.selection(pat.n, True)
    v = sf.weights(rows.size)
    fref = sf.reference(op, sy.FREQS, rows, v)
    bound = fbounds(op, sym, sy.FREQS, rows, v, refine=bool(mode & REFINE))["FIELD_MSE"]
    sv, _ = solver_for(op, sym)
    field = run_field(sv, sy.FREQS, rows=rows, mode=mode)
    plain = run_floss(sv, sy.FREQS, fref.data, "FIELD_MSE", rows=rows, weights=v, mode=mode)
    with_out = run_floss(sv, sy.FREQS, fref.data, "FIELD_MSE", rows=rows, weights=v, mode=mode, want_out=True)
    assert same_bits(with_out["out"], field["out"])                            # the field sweep's bits
    assert with_out["loss"] == plain["loss"] and same_bits(with_out["w"], plain["w"])
    assert np.array_equal(with_out["flags"], field["flags"])
    assert same_bits(with_out["berr"][:, 0], field["berr"][:, 0])
    # the seed of FIELD_MSE on the host, from the device's own field: g = 2 v conj(x - r)
    g = 2 * v * np.conj(field["out"] - fref.data)
    cot = run_floss(sv, sy.FREQS, g, "FCOTANGENT", rows=rows, mode=mode)
    every = np.arange(len(sy.FREQS))
    err = sf.errors(fref, "FIELD_MSE", every, w=cot["w"], scale=cot["scale"])["w"]
    print(f"cotangent of the MSE seed, mode {mode}: w={err:.2e}/{bound['w']:.1e}")
    assert err <= bound["w"]
    # every row, fresh outputs over garbage: the same values as accumulation from zero
    allref = sf.reference(op, sy.FREQS, None, None)
    a = run_floss(sv, sy.FREQS, allref.data, "FIELD_RMSE", mode=mode, want_out=True)
    b = run_floss(sv, sy.FREQS, allref.data, "FIELD_RMSE", mode=mode, fresh=True, prefill=(7.0, 3.0 - 2.0j))
    assert a["loss"] == b["loss"] and same_bits(a["w"], b["w"])
    assert same_bits(a["out"], run_field(sv, sy.FREQS, mode=mode)["out"])
    # ... and without fresh the call accumulates: each of the three chunks adds its part to what is there, so the
    # sum is the prefill plus the total up to one rounding per chunk
    c = run_floss(sv, sy.FREQS, allref.data, "FIELD_RMSE", mode=mode, prefill=(7.0, 3.0 - 2.0j))
    eps = np.finfo(np.float64).eps
    assert abs(c["loss"] - (7.0 + a["loss"])) <= 3 * eps * 8.0
    assert np.max(np.abs(c["w"] - ((3.0 - 2.0j) + a["w"]))) <= 3 * eps * (abs(3.0 - 2.0j) + np.max(np.abs(a["w"])))


# ----------------------------------------------------------------------------- pruning
def test_pruned_sweep_gives_the_bits_of_the_full_one():
    forest, load = "AC", (0,)
    assert (forest, load) in sy.FOREST_CASES
    pat, op = sy.case(forest, load=load)
    sym = sy.symbolic(forest)
    off = sy.component_rows(pat, [k for k in range(len(pat.parts)) if k not in load])
    assert off.size
    fref = sf.reference(op, sy.FREQS, None, None)
    assert np.all(fref.refc.x[:, off] == 0) and np.all(fref.data[:, off] == 0)
    three = sy.three(sy.FREQS)
    f3 = sy.FREQS[three]
    fref3 = sf.reference(op, f3, None, None)
    bound3 = fbounds(op, sym, f3, None, None)
    pruned_k = solver_for(op, sym, prune=True)
    pruned = pruned_k[0]
    assert 0 < pruned.active_fronts().sum() < pruned.active_fronts().size
    plain, _ = solver_for(op, sym, prune=False)
    kw = dict(mode=DEFAULT, vectors=False, fresh=True)
    want = run_sweep(op, sym, sy.FREQS, solver=solver_for(op, sym, prune=True), **kw)
    on = sy.component_rows(pat, load)
    run_field(pruned, sy.FREQS, mode=RAW | REFINE)           # a full-view sweep first: the unloaded rows of X dirty
    for lt in sf.ALL:
        # FCOTANGENT: a seed on every row, the unloaded tree's included
        a = run_floss(pruned, sy.FREQS, fref.sweep_ref(lt), lt, mode=DEFAULT, want_out=True)
        b = run_floss(plain, sy.FREQS, fref.sweep_ref(lt), lt, mode=DEFAULT, want_out=True)
        assert a["loss"] == b["loss"] and same_bits(a["w"], b["w"]), lt
        assert np.all(_bits(a["out"][:, off]) == 0)                            # x = +0.0 on the unloaded tree
        assert np.all(a["flags"] == 0) and np.all(b["flags"] == 0)
        # XA on the unloaded tree is +0.0 after the pruned sweep.  First its rows made non-zero: a cotangent sweep
        # (seed on C's rows) completed by the accessor.  Then the pruned sweep of this loss; then pruning switched
        # off, which drops the views and leaves XA alone, so that the accessor has nothing to complete and returns
        # the last chunk's XA as the sweep left it
        run_floss(pruned, f3, fref3.cot, "FCOTANGENT", mode=DEFAULT)
        assert all(np.any(l[off] != 0) for l in adjoints(pruned, range(3)).values())
        run_floss(pruned, f3, fref3.sweep_ref(lt), lt, mode=DEFAULT)
        pruned.set_prune(False)
        assert pruned.active_fronts().all()
        raw = raw_adjoints(pruned, range(3))
        assert np.all(_bits(raw[:, off]) == 0), lt                              # +0.0 in both parts, sign bit clear
        assert all(np.any(raw[q, on] != 0) for q in range(3))
        pruned.set_prune(True)
        assert 0 < pruned.active_fronts().sum() < pruned.active_fronts().size
        # the whole adjoint for the field seed: the accessor completes the unloaded tree from the seed left in G
        run_floss(pruned, f3, fref3.sweep_ref(lt), lt, mode=DEFAULT)
        lam = adjoints(pruned, range(3))
        assert np.array_equal(np.array([lam[q][on] for q in range(3)]), raw[:, on])    # the loaded rows: the sweep's
        if lt == "FCOTANGENT":
            assert all(np.any(l[off] != 0) for l in lam.values())
        e = sf.errors(fref3, lt, [0, 1, 2], lam=lam, scale=1.0 / 3)["lam"]
        print(f"pruned {lt}: lam={e:.2e}/{bound3[lt]['lam']:.1e}")
        assert e <= bound3[lt]["lam"]
        # the next pruned loss sweep (which zeroes the completed rows again): the bits of a fresh solver's
        after = run_sweep(op, sym, sy.FREQS, solver=pruned_k, **kw)
        assert _same_loss(after, want), lt


# ----------------------------------------------------------------------------- variants
def test_general_analysis():
    shape = sorted(sy.GENERAL_SHAPES)[0]
    pat, op = sy.case(shape)
    sym = sy.symbolic(shape, symmetric=False)
    freqs = np.linspace(40.0, 600.0, 66)                        # one full chunk and a 2-lane tail
    rows = sf.selection(pat.n, True)
    v = sf.weights(rows.size)
    fref = sf.reference(op, freqs, rows, v)
    bound = fbounds(op, sym, freqs, rows, v, symmetric=False)
    sv, _ = solver_for(op, sym)
    for lt in sf.ALL:
        got = run_floss(sv, freqs, fref.sweep_ref(lt), lt, rows=rows, weights=fref.weights_for(lt))
        check_floss(f"general-{shape}", fref, lt, got, bound[lt])


@pytest.mark.parametrize("mode", [RAW, RAW | REFINE], ids=["mode3", "mode7"])
def test_18_stiffness_matrices(mode):
    pat, op = sy.case("A", n_stiff=18)
    sym = sy.symbolic("A")
    fref = sf.reference(op, sy.FREQS, None, None)
    bound = fbounds(op, sym, sy.FREQS, None, None, refine=bool(mode & REFINE))
    sv, _ = solver_for(op, sym)
    for lt in sf.ALL:
        got = run_floss(sv, sy.FREQS, fref.sweep_ref(lt), lt, mode=mode)
        assert got["w"].size == 18
        check_floss(f"A18-mode{mode}", fref, lt, got, bound[lt])


def test_ignored_mode_bits():
    pat, op = sy.case("T")
    sym = sy.symbolic("T")
    rows = sf.selection(pat.n, True)
    fref = sf.reference(op, sy.FREQS, rows, None)
    sv, _ = solver_for(op, sym)
    want = run_floss(sv, sy.FREQS, fref.data, "FIELD_MAC", rows=rows, mode=RAW, want_out=True)
    for mode in (DEFAULT, DEFAULT | _native.PFR_CHECK_REFINE_ADJ):           # 11 and 27
        got = run_floss(sv, sy.FREQS, fref.data, "FIELD_MAC", rows=rows, mode=mode, want_out=True)
        assert got["loss"] == want["loss"] and same_bits(got["w"], want["w"]) and same_bits(got["out"], want["out"])
        assert np.array_equal(got["flags"], want["flags"]) and same_bits(got["berr"], want["berr"])
    assert not np.any(np.isnan(want["berr"]))                   # both checks ran in mode 3


# ----------------------------------------------------------------------------- the next loss sweep, graphs
@pytest.mark.parametrize("graph", ["0", "1"])
def test_loss_sweep_after_a_field_loss_sweep(graph, monkeypatch):
    monkeypatch.setenv("PFR_GRAPH", graph)                      # read in pfr_solver_create
    pat, op = sy.case("T")
    sym = sy.symbolic("T")
    fref = sf.reference(op, sy.FREQS, None, None)
    kw = dict(mode=DEFAULT, vectors=False, fresh=True)
    want = run_sweep(op, sym, sy.FREQS, **kw)
    ref_sv, _ = solver_for(op, sym)
    want_fl = run_floss(ref_sv, sy.FREQS, fref.data, "FIELD_MAC", mode=DEFAULT)
    solver = solver_for(op, sym)
    sv = solver[0]
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(DEV)):             # a stream that can be captured (not the default one)
        first = run_sweep(op, sym, sy.FREQS, solver=solver, calls=3, **kw)     # direct, captured, replayed
        assert _same_loss(first, want)
        launches = sv.graph_launches()
        assert (launches > 0) == (graph == "1")
        got = run_floss(sv, sy.FREQS, fref.data, "FIELD_MAC", mode=DEFAULT)
        assert got["loss"] == want_fl["loss"] and same_bits(got["w"], want_fl["w"])
        assert sv.graph_launches() == launches                  # never part of the graph
        after = run_sweep(op, sym, sy.FREQS, solver=solver, calls=3, **kw)     # direct, captured again, replayed
        assert _same_loss(after, want)
        assert (sv.graph_launches() > launches) == (graph == "1")


# ----------------------------------------------------------------------------- refusals
def test_argument_errors():
    pat, op = sy.case("F0")
    sym = sy.symbolic("F0")
    sv, _ = solver_for(op, sym)
    sv.set_check(RAW, sy.BERR_MAX)
    n, nf = sym.n, 65
    fref = sf.reference(op, sy.FREQS[:nf], None, None)
    good = run_floss(sv, sy.FREQS[:nf], fref.data, "FIELD_MSE")
    freqs = _t(sy.FREQS[:nf])
    ref = _t(fref.data)
    w = torch.zeros(op.n_stiff, dtype=torch.complex128, device=DEV)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    L = _native.lib()
    st = torch.cuda.current_stream(DEV).cuda_stream

    def call(rows=None, n_rows=0, weights=None, lt=32, ref_t=ref, w_t=w, loss_t=loss, handle=None):
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        rp = None if r is None else r.ctypes.data_as(C.POINTER(C.c_int32))
        wt = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        wp = None if wt is None else wt.ctypes.data_as(C.POINTER(C.c_double))
        ptr = lambda t: None if t is None else t.data_ptr()       # noqa: E731
        return L.pfr_field_loss_sweep(sv._h if handle is None else handle, nf, freqs.data_ptr(), n_rows, rp, wp, lt,
                                      ptr(ref_t), 1.0 / nf, None, ptr(loss_t), ptr(w_t), None, 0, st)

    ones = np.ones(n)
    refusals = [
        dict(ref_t=None), dict(w_t=None), dict(loss_t=None),
        dict(lt=31), dict(lt=36), dict(lt=0), dict(lt=16), dict(lt=-1),
        dict(weights=np.where(np.arange(n) == 3, -1.0, 1.0)), dict(weights=np.where(np.arange(n) == 3, np.nan, 1.0)),
        dict(weights=np.where(np.arange(n) == 0, np.inf, 1.0)), dict(weights=np.zeros(n)),
        dict(weights=ones, lt=35),
        dict(rows=[0, n], n_rows=2), dict(rows=[3, -1, 2], n_rows=3), dict(rows=[0, 1], n_rows=0),
        dict(rows=[0, 1], n_rows=-4), dict(rows=[4, 2, 4], n_rows=3), dict(rows=[0, 1], n_rows=2, weights=[0.0, 0.0]),
    ]
    for kw in refusals:
        assert call(**kw) == ERR_ARG, kw
        assert L.pfr_last_error()
    assert call(rows=[4, 2, 4], n_rows=3) == ERR_ARG and b"repeats" in L.pfr_last_error()
    assert call(loss_t=None, lt=35) == 0                        # FCOTANGENT takes no loss
    torch.cuda.synchronize()
    w.zero_()
    with pytest.raises(_native.NativeError):
        sv.field_loss_sweep(freqs, 32, ref, torch.view_as_real(w), rows=[1, 1], loss=loss)
    with pytest.raises(ValueError):
        sv.field_loss_sweep(freqs, 32, ref[:, :3], torch.view_as_real(w), rows=[0, 1, 2, 3], loss=loss)
    with pytest.raises(ValueError):
        sv.field_loss_sweep(freqs, 32, ref, torch.view_as_real(w), weights=[1.0, 2.0], loss=loss)
    torch.cuda.synchronize()
    assert loss.item() == 0.0 and not w.cpu().numpy().any()     # nothing was launched by a refused call
    # PFR_ERR_STATE as in the reverse sweeps: no stiffness set
    bare = _native.Solver(sym, 0, 64)
    K = torch.empty(op.pat.nnz, dtype=torch.complex128, device=DEV)
    K.copy_(_t(op.K))
    bare.set_operator(torch.view_as_real(K), _t(op.M))
    bare.set_rhs(op.rhs, op.beta, op.mass_sum)
    bare.set_functional(op.sup, op.a3, op.ts)
    assert call(handle=bare._h) == ERR_STATE and b"stiffness" in L.pfr_last_error()
    # the next call is unharmed
    again = run_floss(sv, sy.FREQS[:nf], fref.data, "FIELD_MSE")
    assert again["loss"] == good["loss"] and same_bits(again["w"], good["w"])
