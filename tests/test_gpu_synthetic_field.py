"""GPU: pfr_field_sweep (include/pfr.h) through the C ABI on the synthetic fronts of tests/synthetic.py -- the solution
itself, gathered from the chunk's frequency-minor, permuted X into caller-numbered, frequency-major output by
k_field_gather (tiles of 64 frequencies x pfr_field_tile_rows() selected rows through LDS).

What is asserted, and against what:
  bitwise       every row of `out` equals pfr_debug_solution(0, lane) -- the strided copy of the same X -- of a
                pfr_sweep(PFR_LOSS_NONE) in the same check mode on a second solver, truncated to 64, 128 and 130
                frequencies so that every chunk is "the last" once; the field sweep's own last chunk equals its own
                accessor; fr, the flags and berr[2 q] equal that sweep's, berr[2 q + 1] keeps its NaN
  reference     x over every frequency against the extended-precision dense reference, at the bound
                tests/test_gpu_synthetic.py applies to its x: 10 x max(e_model, e_dense, synthetic.FLOOR) from the fp64
                multifrontal model and the unrefined dense solve (test_gpu_synthetic._bounds), never from the GPU
  tile edges    selections of 1, R - 1, R, R + 1, 2 R + 1 and n rows, and one with repeats, descending, holding the
                Dirichlet rows, at 1, 63, 64 and 65 frequencies: the matching columns of the all-rows result, bit for bit
  guard bands   `out` lies inside a larger buffer of one NaN bit pattern; the bands on both sides (and the whole
                buffer's entries outside nfreq x n_sel) keep it
  pruning       rows of unloaded trees exact +0.0 (sign bit clear), every other row the bits of pfr_set_prune(0)
  ignored bits  mode 11 (the engine's default) gives the bits of mode 3; a loss sweep after a field sweep gives the
                bits of one without it, also with PFR_GRAPH=1 once the graph is captured
  refusals      row n, row -1, n_rows = 0 with a list, a null out: PFR_ERR_ARG, and the next valid call is unharmed
  general       a general (non-symmetric) analysis on operator data, within its bound of the reference
"""
import ctypes as C

import numpy as np
import pytest
import torch

import synthetic as sy
from plate_inverse_problem_amd import _native
from test_gpu_synthetic import DEFAULT, DEV, LOSS_ID, RAW, _bounds, _t, make_solver, run_sweep

pytestmark = pytest.mark.gpu
REFINE = _native.PFR_CHECK_REFINE
GUARD = 4096                                   # complex entries on either side of `out`
NAN_BITS = np.uint64(0x7FF8DEAD0000BEEF)       # the guard pattern (a quiet NaN with a payload)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def run_field(sv, freqs, rows=None, mode=RAW, want_fr=True, n=None):
    """One pfr_field_sweep into a guarded buffer.  Returns out (nfreq, n_sel), fr, flags, berr on the host after
    checking that nothing but out's entries was written."""
    nf = len(freqs)
    n_sel = (n if n is not None else sv.sym.n) if rows is None else len(rows)
    berr = torch.full((nf, 2), float("nan"), dtype=torch.float64, device=DEV)
    sv.set_check(mode, sy.BERR_MAX, berr)
    fill = torch.as_tensor(np.full(2 * (nf * n_sel + 2 * GUARD), NAN_BITS).view(np.float64), device=DEV)
    buf = torch.view_as_complex(fill.view(-1, 2))
    out = buf[GUARD:GUARD + nf * n_sel].view(nf, n_sel)
    fr = torch.zeros(nf, dtype=torch.float64, device=DEV) if want_fr else None
    flags = torch.zeros(nf, dtype=torch.int32, device=DEV)
    sv.field_sweep(_t(freqs), out, rows=rows, fr=fr, flags=flags)
    torch.cuda.synchronize()
    host = _bits(torch.view_as_real(buf).cpu().numpy()).reshape(-1, 2)
    assert np.all(host[:GUARD] == NAN_BITS) and np.all(host[GUARD + nf * n_sel:] == NAN_BITS), "guard band written"
    res = out.cpu().numpy()
    sv.set_check(mode, sy.BERR_MAX)                             # berr is this call's: not left registered
    assert not np.any(_bits(res) == NAN_BITS), "an entry of out was not written"
    return dict(out=res, fr=None if fr is None else fr.cpu().numpy(), flags=flags.cpu().numpy(),
                berr=berr.cpu().numpy())


def last_chunk(sv, nf):
    """pfr_debug_solution(0, lane) of every lane of the last chunk of an nf-frequency call: (first frequency, rows).
    Through the C ABI directly: the doubles as the accessor wrote them (Solver.debug_solution adds the parts, which
    turns a -0.0 into +0.0)."""
    q0 = (nf - 1) // sv.max_batch * sv.max_batch
    raw = np.zeros((nf - q0, 2 * sv.sym.n), dtype=np.float64)
    for lane in range(nf - q0):
        _native.check(_native.lib().pfr_debug_solution(sv._h, 0, lane, raw[lane].ctypes.data_as(C.POINTER(C.c_double))),
                      "pfr_debug_solution")
    return q0, raw.view(np.complex128)


def run_none(sv, freqs, mode):
    """pfr_sweep(PFR_LOSS_NONE) in ``mode``: fr, flags, berr and the last chunk's solution rows."""
    nf = len(freqs)
    berr = torch.full((nf, 2), float("nan"), dtype=torch.float64, device=DEV)
    sv.set_check(mode, sy.BERR_MAX, berr)
    fr = torch.zeros(nf, dtype=torch.float64, device=DEV)
    flags = torch.zeros(nf, dtype=torch.int32, device=DEV)
    sv.sweep(_t(freqs), LOSS_ID["NONE"], fr=fr, flags=flags)
    torch.cuda.synchronize()
    sv.set_check(mode, sy.BERR_MAX)
    q0, x = last_chunk(sv, nf)
    return dict(fr=fr.cpu().numpy(), flags=flags.cpu().numpy(), berr=berr.cpu().numpy(), q0=q0, x=x)


_FIELD = {}


def field_case(shape, mode):
    """The all-rows field sweep of a shape over synthetic.FREQS, once per (shape, mode)."""
    if (shape, mode) not in _FIELD:
        _, op = sy.case(shape)
        sym = sy.symbolic(shape)
        sv, _ = make_solver(op, sym)
        got = run_field(sv, sy.FREQS, mode=mode)
        got["own_last"] = last_chunk(sv, len(sy.FREQS))
        _FIELD[shape, mode] = (op, sym, got)
    return _FIELD[shape, mode]


# ----------------------------------------------------------------------------- bitwise against the accessor
@pytest.mark.parametrize("mode", [RAW, RAW | REFINE], ids=["mode3", "mode7"])
@pytest.mark.parametrize("shape", ["T", "F0", "A"])
def test_bitwise_against_the_accessor(shape, mode):
    op, sym, got = field_case(shape, mode)
    nf = len(sy.FREQS)
    q0, rows = got["own_last"]
    assert same_bits(got["out"][q0:], rows)
    other, _ = make_solver(op, sym)
    for cut in (64, 128, nf):                                   # every chunk the last one once
        ref = run_none(other, sy.FREQS[:cut], mode)
        c0 = ref["q0"]
        assert c0 == (cut - 1) // 64 * 64 and ref["x"].shape[0] == cut - c0
        assert same_bits(got["out"][c0:cut], ref["x"]), (shape, mode, cut)
        assert same_bits(got["fr"][:cut], ref["fr"])
        assert np.array_equal(got["flags"][:cut], ref["flags"])
        assert same_bits(got["berr"][:cut, 0], ref["berr"][:, 0])
    assert np.all(np.isnan(got["berr"][:, 1]))                  # no adjoint: slot 2 q + 1 left alone
    assert np.all(got["flags"] == 0) and got["berr"][:, 0].max() <= sy.BERR_MAX


# ----------------------------------------------------------------------------- against the extended-precision reference
@pytest.mark.parametrize("mode", [RAW, RAW | REFINE], ids=["mode3", "mode7"])
@pytest.mark.parametrize("shape", ["T", "F0", "A"])
def test_against_the_reference(shape, mode):
    op, sym, got = field_case(shape, mode)
    bound = _bounds(op, sym, sy.FREQS, "NONE", **({"refine": True} if mode & REFINE else {}))
    refc = sy.reference(op, sy.FREQS)
    every = np.arange(len(sy.FREQS))
    err = sy.errors(refc, "MSE_LOG_AFC", every, x=got["out"], fr=got["fr"])
    print(f"field-{shape}-mode{mode} x={err['x']:.2e}/{bound['x']:.1e} fr={err['fr']:.2e}/{bound['fr']:.1e}")
    assert bound["x"] >= 10 * sy.FLOOR
    assert err["x"] <= bound["x"], (err, bound)
    assert err["fr"] <= bound["fr"], (err, bound)


# ----------------------------------------------------------------------------- tile and chunk edges
@pytest.mark.parametrize("nfreq", [1, 63, 64, 65])
def test_tile_and_chunk_edges(nfreq):
    pat, op = sy.case("A")
    sym = sy.symbolic("A")
    sv, _ = make_solver(op, sym)
    n, R = pat.n, _native.field_tile_rows()
    assert 2 * R + 1 < n
    freqs = sy.FREQS[:nfreq]
    full = run_field(sv, freqs)
    rng = np.random.default_rng(7000 + nfreq)
    picks = [rng.permutation(n)[:k].astype(np.int32) for k in (1, R - 1, R, R + 1, 2 * R + 1)]
    picks.append(np.arange(n, dtype=np.int32))
    # repeats, descending order, the Dirichlet rows among them
    d = np.asarray(pat.dirichlet, dtype=np.int32)
    picks.append(np.sort(np.concatenate([d, d, rng.permutation(n)[:R + 5], [0, 0, n - 1]]))[::-1].astype(np.int32))
    assert np.all(np.isin(d, picks[-1])) and np.any(np.diff(picks[-1]) == 0)
    for rows in picks:
        sub = run_field(sv, freqs, rows=rows, want_fr=rows.size % 2 == 0)
        assert sub["out"].shape == (nfreq, rows.size)
        assert same_bits(sub["out"], full["out"][:, rows]), (nfreq, rows.size)
        assert np.array_equal(sub["flags"], full["flags"]) and same_bits(sub["berr"][:, 0], full["berr"][:, 0])
        if sub["fr"] is not None:
            assert same_bits(sub["fr"], full["fr"])
    # the explicit list of every row is the NULL list
    assert same_bits(run_field(sv, freqs, rows=np.arange(n, dtype=np.int32))["out"], full["out"])


# ----------------------------------------------------------------------------- pruning
def test_pruned_rows_are_positive_zero():
    forest, load = "AC", (0,)
    assert (forest, load) in sy.FOREST_CASES
    pat, op = sy.case(forest, load=load)
    sym = sy.symbolic(forest)
    off = sy.component_rows(pat, [k for k in range(len(pat.parts)) if k not in load])
    on = sy.component_rows(pat, load)
    assert off.size and on.size
    pruned, _ = make_solver(op, sym, prune=True)
    assert 0 < pruned.active_fronts().sum() < pruned.active_fronts().size
    plain, _ = make_solver(op, sym, prune=False)
    # a full-view sweep first leaves non-zero bits in the unloaded rows of X (mode 7 keeps the full plan): they must be
    # cleared again before the pruned field sweep
    run_field(pruned, sy.FREQS, mode=RAW | REFINE)
    a = run_field(pruned, sy.FREQS, mode=DEFAULT)
    b = run_field(plain, sy.FREQS, mode=DEFAULT)
    assert np.all(_bits(a["out"][:, off]) == 0)                 # +0.0 in both parts, sign bit clear
    assert same_bits(a["out"][:, on], b["out"][:, on])
    assert np.all(a["flags"] == 0) and np.all(b["flags"] == 0)
    sel = np.concatenate([off[:3], on[:3], off[-2:]]).astype(np.int32)
    assert same_bits(run_field(pruned, sy.FREQS, rows=sel, mode=DEFAULT)["out"], a["out"][:, sel])


# ----------------------------------------------------------------------------- ignored bits, the next loss sweep, graphs
def test_mode_11_gives_the_bits_of_mode_3():
    op, sym, got = field_case("T", RAW)
    sv, _ = make_solver(op, sym)
    for mode in (DEFAULT, DEFAULT | _native.PFR_CHECK_REFINE_ADJ, _native.PFR_CHECK_FORWARD):
        other = run_field(sv, sy.FREQS, mode=mode)
        for k in ("out", "fr"):
            assert same_bits(other[k], got[k]), (mode, k)
        assert np.array_equal(other["flags"], got["flags"])
        assert same_bits(other["berr"][:, 0], got["berr"][:, 0]) and np.all(np.isnan(other["berr"][:, 1]))


def _loss_bits(out):
    return (np.float64(out["loss"]).view(np.uint64), _bits(out["w"]).copy(), _bits(out["fr"]).copy(),
            out["flags"].copy(), _bits(out["berr"]).copy())


def _same_loss(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_loss_bits(a), _loss_bits(b)))


@pytest.mark.parametrize("graph", ["0", "1"])
def test_loss_sweep_after_a_field_sweep(graph, monkeypatch):
    monkeypatch.setenv("PFR_GRAPH", graph)                      # read in pfr_solver_create
    _, op = sy.case("T")
    sym = sy.symbolic("T")
    kw = dict(mode=DEFAULT, vectors=False, fresh=True)
    want = run_sweep(op, sym, sy.FREQS, **kw)
    solver = make_solver(op, sym)
    sv = solver[0]
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(DEV)):             # a stream that can be captured (not the default one)
        # the same arguments three times (same tensors: run_sweep's `calls`): direct, captured, replayed
        first = run_sweep(op, sym, sy.FREQS, solver=solver, calls=3, **kw)
        assert _same_loss(first, want)
        launches = sv.graph_launches()
        assert (launches > 0) == (graph == "1")
        field = run_field(sv, sy.FREQS, mode=DEFAULT)
        assert same_bits(field["out"], field_case("T", RAW)[2]["out"])
        assert sv.graph_launches() == launches                  # never part of the graph
        after = run_sweep(op, sym, sy.FREQS, solver=solver, calls=3, **kw)   # direct, captured again, replayed
        assert _same_loss(after, want)
        assert (sv.graph_launches() > launches) == (graph == "1")


# ----------------------------------------------------------------------------- refusals
def test_argument_errors():
    op, sym, got = field_case("F0", RAW)
    sv, _ = make_solver(op, sym)
    sv.set_check(RAW, sy.BERR_MAX)
    n, nf = sym.n, 65
    freqs = _t(sy.FREQS[:nf])
    out = torch.zeros((nf, n), dtype=torch.complex128, device=DEV)
    L = _native.lib()

    def call(rows, n_rows, out_t):
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        rp = None if r is None else r.ctypes.data_as(C.POINTER(C.c_int32))
        return L.pfr_field_sweep(sv._h, nf, freqs.data_ptr(), n_rows, rp, None if out_t is None else out_t.data_ptr(),
                                 None, None, torch.cuda.current_stream(DEV).cuda_stream)

    ERR_ARG = 1
    assert call([0, n], 2, out) == ERR_ARG and b"outside" in L.pfr_last_error()
    assert call([3, -1, 2], 3, out) == ERR_ARG
    assert call([0, 1], 0, out) == ERR_ARG
    assert call([0, 1], -4, out) == ERR_ARG
    assert call(None, 0, None) == ERR_ARG
    assert call([0, 1], 2, None) == ERR_ARG
    torch.cuda.synchronize()
    assert not out.cpu().numpy().any()                          # nothing was launched
    with pytest.raises(_native.NativeError):
        sv.field_sweep(freqs, out, rows=[n])
    with pytest.raises(ValueError):
        sv.field_sweep(freqs, out[:, :3], rows=[0, 1, 2, 3])    # out too small for nfreq x n_sel
    good = run_field(sv, sy.FREQS[:nf])
    assert same_bits(good["out"], got["out"][:nf])
    assert call(None, -7, out) == 0                             # a NULL list: n_rows ignored
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), got["out"][:nf])


# ----------------------------------------------------------------------------- a general analysis
def test_general_analysis():
    shape = sorted(sy.GENERAL_SHAPES)[0]
    _, op = sy.case(shape)
    sym = sy.symbolic(shape, symmetric=False)
    freqs = np.linspace(40.0, 600.0, 66)                        # one full chunk and a 2-lane tail
    bound = _bounds(op, sym, freqs, "NONE", symmetric=False)
    sv, _ = make_solver(op, sym)
    got = run_field(sv, freqs)
    refc = sy.reference(op, freqs)
    err = sy.errors(refc, "MSE_LOG_AFC", np.arange(freqs.size), x=got["out"], fr=got["fr"])
    print(f"field-general-{shape} x={err['x']:.2e}/{bound['x']:.1e} fr={err['fr']:.2e}/{bound['fr']:.1e}")
    assert err["x"] <= bound["x"] and err["fr"] <= bound["fr"], (err, bound)
    assert np.all(got["flags"] == 0) and got["berr"][:, 0].max() <= sy.BERR_MAX
    q0, rows = last_chunk(sv, freqs.size)
    assert same_bits(got["out"][q0:], rows)
