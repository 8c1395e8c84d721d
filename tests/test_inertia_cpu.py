"""CPU: the inertia sweep's interface, its reference rows and identities, the plan's compacted mass list and the host
chain rule from (rho, h, acc_mass) to the inertia constants and the laminate coefficients (no GPU)."""
import dataclasses

import numpy as np
import pytest

import synthetic as sy
import synthetic_inertia as si
from plate_inverse_problem_amd import _native

FREQS4 = np.linspace(40.0, 600.0, 4)


# ----------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_bound_and_exported():
    for name in ("pfr_set_inertia", "pfr_inertia_sweep", "pfr_symbolic_mass_list", "pfr_solver_mass_list"):
        assert name in _native.header_symbols()
        assert name in _native._PROTOS
        assert hasattr(_native.lib(), name)
    assert set(_native.header_symbols()) == set(_native._PROTOS)
    assert hasattr(_native.Solver, "set_inertia") and hasattr(_native.Solver, "inertia_sweep")


def test_null_solver_is_an_argument_error():
    L = _native.lib()
    assert L.pfr_inertia_sweep(None, 4, None, None, None, None, None, None, None) == 1     # PFR_ERR_ARG
    assert b"inertia" in L.pfr_last_error()
    assert L.pfr_set_inertia(None, 4, None, None) == 1
    assert b"inertia" in L.pfr_last_error()
    assert L.pfr_solver_mass_list(None, None) == -1


# ----------------------------------------------------------------------------- the split
@pytest.mark.parametrize("n_mass", [1, 3, 4])
def test_split_recombines_to_the_operator(n_mass):
    """The fp64 sum in the engine's order IS the operator's M and mass_sum (split asserts that the sums carry no
    rounding at all); the components are symmetric where M is."""
    _, op = sy.case("T")
    ins = si.split(op, n_mass=n_mass)
    assert ins.G.shape == (n_mass, op.pat.nnz) and ins.op is not op and not ins.op._cache
    assert np.array_equal(si.recombine(ins.I, ins.G), ins.op.M)
    assert ins.op.mass_sum == float(si.recombine(ins.I, ins.d[:, None])[0])
    np.testing.assert_allclose(ins.op.M, op.M, rtol=0, atol=2.0 ** -(si.GRID - 3))
    assert abs(ins.op.mass_sum - op.mass_sum) <= 2.0 ** -(si.GRID - 3)
    for G in ins.G:
        D = ins.op.pat.dense(G)
        sym = np.ones(op.pat.n, bool)
        sym[op.pat.dirichlet] = False
        assert np.array_equal(D[np.ix_(sym, sym)], D[np.ix_(sym, sym)].T)
    assert si.split(op, n_mass=n_mass) is ins


# ----------------------------------------------------------------------------- the reference rows
@pytest.mark.parametrize("shape", ["A", "T"])
def test_reference_rows_match_finite_differences(shape):
    """Re jm[q][j] against central differences (t = 1e-7 relative to I_j, extended precision) of fr in each I_j,
    4 frequencies; the bound 1e-9 of test_jacobian_cpu's comparison of jc by the same construction."""
    _, op = sy.case(shape)
    ins = si.split(op)
    _, _, jm = si.reference(ins, FREQS4)
    I = ins.I.astype(sy.LD)
    t = sy.LD(1e-7)
    fd = []
    for j in range(ins.n_mass):
        dI = np.zeros(ins.n_mass, dtype=sy.LD)
        dI[j] = t * I[j]
        fd.append((si.response_at(ins, FREQS4, I + dI) - si.response_at(ins, FREQS4, I - dI)) / (2 * dI[j]))
    fd = np.stack(fd, axis=1)
    err = float(np.max(np.max(np.abs(jm.real - fd), axis=1) / np.max(np.abs(jm.real), axis=1)))
    print(f"{shape}: |Re jm - fd| / max|Re jm| = {err:.1e}")
    assert err <= 1e-9


def test_complex_reference_rows_match_finite_differences():
    """The complex response along (0.6, 0.8, 1): dH / dI_j = jm[q][j], no real part taken."""
    _, op = sy.case("T")
    ins = si.split(op)
    axis = (0.6, 0.8, 1.0)
    _, _, jm = si.reference(ins, FREQS4, axis)
    I = ins.I.astype(sy.LD)
    t = sy.LD(1e-7)
    fd = []
    for j in range(ins.n_mass):
        dI = np.zeros(ins.n_mass, dtype=sy.LD)
        dI[j] = t * I[j]
        fd.append((si.response_at(ins, FREQS4, I + dI, axis) - si.response_at(ins, FREQS4, I - dI, axis)) / (2 * dI[j]))
    fd = np.stack(fd, axis=1)
    err = float(np.max(np.max(np.abs(jm - fd), axis=1) / np.max(np.abs(jm), axis=1)))
    print(f"T complex: |jm - fd| / max|jm| = {err:.1e}")
    assert err <= 1e-9


@pytest.mark.parametrize("axis", [None, (0.6, 0.8, 1.0)], ids=["fr", "H"])
@pytest.mark.parametrize("shape", ["A", "T"])
def test_reference_is_homogeneous(shape, axis):
    """sum_k c_k jc_k + sum_j I_j jm_j = 0 for the reference rows, relative to the largest term: the split, K and beta
    are exact, so what is left is the error of the refined solves, cond x a few extended-precision roundings --
    COND_MAX x 10 x 1.1e-19 = 1e-14 = synthetic.FLOOR."""
    _, op = sy.case(shape)
    ins = si.split(op)
    _, jc, jm = si.reference(ins, FREQS4, axis)
    res = si.homogeneity(ins, jc, jm)
    print(f"{shape} {'fr' if axis is None else 'H'}: homogeneity residual {res.max():.1e}")
    assert res.max() <= sy.FLOOR


@pytest.mark.parametrize("shape", ["A", "T"])
def test_slope_identity_matches_finite_differences_in_f(shape):
    """d fr / d f = (2 / f) Re sum_j I_j jm_j against central differences of fr in f (t = 1e-7 f), at 1e-9."""
    _, op = sy.case(shape)
    ins = si.split(op)
    _, _, jm = si.reference(ins, FREQS4)
    s = si.slope(ins, FREQS4, jm).real
    f = FREQS4.astype(sy.LD)
    t = sy.LD(1e-7)
    I = ins.I.astype(sy.LD)
    fd = (si.response_at(ins, f * (1 + t), I) - si.response_at(ins, f * (1 - t), I)) / (2 * t * f)
    err = float(np.max(np.abs(s - fd) / np.abs(s)))
    print(f"{shape}: |slope - fd| / |slope| = {err:.1e}")
    assert err <= 1e-9


def test_model_rows_sit_at_rounding_level():
    """model_errors on A, both analyses, raw and corrected: the fp64 sequences agree with the reference to rounding
    (the bounds of the GPU tests are 10 x these), and so does their homogeneity residual."""
    _, op = sy.case("A")
    ins = si.split(op)
    freqs = sy.FREQS[sy.three(sy.FREQS)]
    for symmetric in (True, False):
        for correct in (False, True):
            em, ed = si.model_errors(ins, sy.symbolic("A", symmetric=symmetric), freqs, symmetric=symmetric,
                                     correct=correct)
            print(f"A symmetric={symmetric} correct={correct}: e_model {em} e_dense {ed}")
            assert max(max(e[k] for k in ("jm", "jc", "resp", "hom")) for e in (em, ed)) < 1e-11


# ----------------------------------------------------------------------------- the plan's compacted list
def _list_case(shape, ins, prune, load=None):
    sym = sy.symbolic(shape)
    op = ins.op
    lst, ptr, n_list, ent = sym.mass_list(ins.G.T, rhs=op.rhs, prune=prune)
    on = ins.G.any(axis=0)
    row_on = None
    if prune:
        mask = sym.prune(64, op.rhs, op.sup)[0].astype(bool)
        fr = sym.export("FRONTS")
        row_on = np.zeros(op.pat.n, bool)
        for t in np.nonzero(mask)[0]:
            row_on[fr[t, 3]:fr[t, 3] + fr[t, 0]] = True            # the front's pivot rows: col0 .. col0 + ns
    wave_of = si.check_mass_list(lst, ptr, n_list, ent, on, row_on)
    return lst, n_list, ent, row_on, wave_of


@pytest.mark.parametrize("shape", ["A", "T", "F0"])
def test_mass_list_full(shape):
    """Every entry with a non-zero component once, in the entries' order, each wave's run padded to batches of 4."""
    _, op = sy.case(shape)
    ins = si.split(op)
    lst, n_list, ent, _, _ = _list_case(shape, ins, False)
    iperm = sy.symbolic(shape).export("IPERM")
    # the entries themselves: row starts and pattern entries in the permuted numbering
    real = ent[:, 1] >= 0
    assert np.array_equal(np.sort(ent[real, 1]), np.arange(op.pat.nnz))
    assert np.array_equal(iperm[op.pat.rows[ent[real, 1]]], ent[real, 3])
    assert np.array_equal(iperm[op.pat.cols[ent[real, 1]]], ent[real, 0])
    assert n_list == np.count_nonzero(ins.G.any(axis=0))


@pytest.mark.parametrize("entries", [1, 5])
def test_mass_list_tail(entries):
    """Components masked to exactly 1 and 5 entries: most waves own none, the others a padded batch or two."""
    _, op = sy.case("T")
    ins = si.split(op, n_mass=1, entries=entries)
    lst, n_list, _, _, wave_of = _list_case("T", ins, False)
    assert n_list == entries and 4 * len(set(wave_of.values())) <= lst.size <= 4 * (len(set(wave_of.values())) + 1)
    assert np.count_nonzero(lst == -1) > 0


def test_mass_list_of_a_zero_table_is_empty():
    _, op = sy.case("T")
    ins = si.split(op, n_mass=1, zero=(0,))
    lst, n_list, _, _, _ = _list_case("T", ins, False)
    assert n_list == 0 and lst.size == 0


@pytest.mark.parametrize("forest,load", sy.FOREST_CASES[:6], ids=[sy.forest_id(f, l) for f, l in sy.FOREST_CASES[:6]])
def test_mass_list_of_a_view_lists_only_its_rows(forest, load):
    """Under pruning the list holds the entries on the loaded trees' pivot rows only -- and all of those -- and every
    one of them on the wave that owns it in the full list (what makes a view's rows equal the full walk's bits)."""
    _, op = sy.case(forest, load=load)
    ins = si.split(op)
    full = _list_case(forest, ins, False)
    lst, n_list, ent, row_on, wave_of = _list_case(forest, ins, True)
    assert 0 < n_list < full[1]
    assert np.all(row_on[ent[lst[lst >= 0], 3]])
    assert all(full[4][e] == w for e, w in wave_of.items())


def test_mass_list_rejects_bad_arguments():
    _, op = sy.case("A")
    sym = sy.symbolic("A")
    with pytest.raises(_native.NativeError):
        sym.mass_list(np.zeros((op.pat.nnz, 5)))
    with pytest.raises(_native.NativeError):
        sy.symbolic("A", symmetric=False).mass_list(np.zeros((op.pat.nnz, 2)), rhs=op.rhs, prune=True)


# ----------------------------------------------------------------------------- the host chain rule
FIXTURES = [("isotropic", 3), ("orthotropic", 4), ("sol", 3)]


def _problem(material, ny):
    from helpers import make_problem
    return make_problem(material, ny=ny)


@pytest.mark.parametrize("material,ny", FIXTURES)
def test_inertia_constants_are_the_problems_bits(material, ny):
    from plate_inverse_problem_amd.Problem import inertia_constants
    p = _problem(material, ny)
    I, dI = inertia_constants(p.rho, p.geometry.height, p.accelerometer)
    assert I.shape == (4,) and dI.shape == (4, 3)
    assert I.tolist() == [p.I0, p.I0Corr, p.I2, p.I2Corr]                      # equal as bits (no NaN, no -0.0 here)
    assert np.array_equal(p.extendedParameters(("h", "rho")),
                          np.concatenate([p.parameters, [p.geometry.height, p.rho]]))


def test_inertia_constants_derivatives():
    """dI against central differences (relative step 1e-6: truncation ~1e-12, rounding ~1e-10 of a cubic)."""
    from plate_inverse_problem_amd.Problem import EXTRA_NAMES, inertia_constants
    p = _problem("orthotropic", 4)
    acc = p.accelerometer
    x0 = np.array([p.rho, p.geometry.height, acc.mass])
    assert EXTRA_NAMES == ("rho", "h", "acc_mass")
    _, dI = inertia_constants(*x0[:2], acc, x0[2])
    for i in range(3):
        step = 1e-6 * x0[i]
        xp, xm = x0.copy(), x0.copy()
        xp[i] += step
        xm[i] -= step
        fd = (inertia_constants(xp[0], xp[1], acc, xp[2])[0] - inertia_constants(xm[0], xm[1], acc, xm[2])[0]) / (2 * step)
        scale = np.abs(dI[:, i]).max()
        assert np.max(np.abs(dI[:, i] - fd)) <= 1e-8 * scale, (i, dI[:, i], fd)
    assert np.all(dI[[0, 2], 2] == 0) and np.all(dI[1, :2] == 0) and dI[3, 0] == 0


@pytest.mark.parametrize("material,ny", FIXTURES)
def test_thickness_scales_the_coefficient_blocks(material, ny):
    """c(h') = c(h0) (h' / h0)^(1, 2, 3) on the A, B, D blocks: against the package's transform and the oracle's
    coeffs18 evaluated at h0 (1 +- t), to rounding."""
    from oracle.plate_oracle import coeffs18
    from plate_inverse_problem_amd._abd_jet import abd_and_jacobian
    from plate_inverse_problem_amd.Problem import thickness_scaling
    p = _problem(material, ny)
    h0, theta = p.geometry.height, np.asarray(p.parameters, dtype=np.float64)
    c0 = abd_and_jacobian(p.material, h0, theta)[0]
    assert np.array_equal(thickness_scaling(h0, h0), np.ones(18))
    for t in (-0.02, 0.05):
        h = h0 * (1 + t)
        want = c0 * thickness_scaling(h, h0)
        scale = np.repeat(np.abs(want).reshape(3, 6).max(axis=1), 6)
        for got in (abd_and_jacobian(p.material, h, theta)[0],
                    coeffs18(p.material.atype, h, theta, getattr(p.material, "angles", None))):
            assert np.max(np.abs(got - want) / np.where(scale > 0, scale, 1.0)) <= 1e-14
            assert np.all(got[scale == 0] == 0)


def _oracle_rows(orc, acc, rho, freqs, theta, acc_mass=None):
    """(fr, d fr / d (rho, h, acc_mass, f), jc) from the oracle's own refined forward and adjoint solves:
    jm_j = om2 (mu^T G_j x - mu^T rhs), jc_k = -mu^T S_k x + e_k mu^T rhs, then the host chain rule."""
    import scipy.sparse as sp
    from oracle.plate_oracle import RHS_WEIGHTS_D, refined_solve
    from plate_inverse_problem_amd.Problem import inertia_constants
    m = orc.mats
    G = [m[18] + m[20] + m[22], m[19] + m[21] + m[23], m[24], m[25]]
    e = np.concatenate([np.zeros(12), RHS_WEIGHTS_D])
    c = orc.coefficients(theta)
    I, dI = inertia_constants(rho, orc.h, acc, acc_mass)
    assert np.allclose(I, orc.I, rtol=1e-15)
    dcdh = np.repeat([1.0, 2.0, 3.0], 6) / orc.h * c
    aU, aV, aW = orc.averaging_vectors()
    ts2 = orc.acc_ts ** 2
    frs, rows, jcs = [], [], []
    for f in freqs:
        x, lu, A = orc.solve(f, theta)
        U, V, W = orc.uvw(x)
        fr = orc.fr_from_sol(x)
        g = (ts2 * np.conj(U) * aU + ts2 * np.conj(V) * aV + np.conj(W) * aW) / fr
        mu = refined_solve(lu, A, g, trans=True)
        P = mu[orc.rows] * x[orc.cols]
        t = mu @ orc.rhs_vec
        om2 = (2 * np.pi * f) ** 2
        jm = om2 * (np.array([Gj @ P for Gj in G]) - t)
        jc = -(m[:18] @ P) + e * t
        frs.append(fr)
        rows.append(np.concatenate([np.real(jm @ dI), [0.0]]))
        rows[-1][1] += np.real(jc @ dcdh)
        rows[-1][3] = 2.0 / f * np.real(jm @ I)
        jcs.append(jc)
    return np.array(frs), np.array(rows), np.array(jcs)


def test_oracle_rows_match_its_finite_differences():
    """On the ny = 3 orthotropic oracle, 6 frequencies: the columns d fr / d (rho, h, acc_mass, f) from the formula
    against 4th-order central differences of the oracle's own fr (dataclasses.replace(orc, I=..., h=...)), relative
    steps 1e-3 and 2e-3.  The differences' own error -- the two step sizes against each other, per column max_q |d| /
    max_q |ref| -- measured 1.7e-08, 5.0e-08, 1.1e-08, 8.0e-09 (rho, h, acc_mass, f: the rounding of the oracle's
    solves over the step, not truncation); the formula is asserted within 10 x that of the finer differences, and
    came out at 8.3e-09, 4.0e-09, 1.0e-08, 3.7e-09."""
    from helpers import oracle_for
    from oracle.plate_oracle import inertia
    p = _problem("orthotropic", 3)
    orc, acc = oracle_for(p), p.accelerometer
    theta = np.asarray(p.parameters, dtype=np.float64)
    freqs = np.linspace(40.0, 600.0, 6)
    x0 = np.array([p.rho, p.geometry.height, acc.mass])
    _, rows, _ = _oracle_rows(orc, acc, p.rho, freqs, theta)

    def fr_at(x, f):
        o = dataclasses.replace(orc, I=inertia(x[1], x[0], x[2], acc.radius, acc.height), h=x[1])
        return o.fr(f, theta)

    def fd(rel):
        cols = []
        for i in range(4):
            vals = []
            for k in (-2, -1, 1, 2):
                x, f = x0.copy(), freqs.copy()
                if i < 3:
                    x[i] *= 1 + k * rel
                else:
                    f = f * (1 + k * rel)
                vals.append(fr_at(x, f))
            step = rel * (x0[i] if i < 3 else freqs)
            cols.append((vals[0] - 8 * vals[1] + 8 * vals[2] - vals[3]) / (12 * step))
        return np.stack(cols, axis=1)

    fine, coarse = fd(1e-3), fd(2e-3)
    scale = np.max(np.abs(fine), axis=0)
    own = np.max(np.abs(fine - coarse), axis=0) / scale
    err = np.max(np.abs(rows - fine), axis=0) / scale
    print("finite differences' own error", own, "formula against them", err)
    assert np.all(err <= 10 * own), (err, own)
