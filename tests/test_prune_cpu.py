"""Host side of pruning (include/pfr.h, pfr_set_prune): which elimination trees the load reaches, and the views of
the plan and schedule over them and over the rest -- built and checked without a device (pfr_symbolic_prune runs
check_plan and check_schedule on both views and fails on the first violation)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg

from helpers import make_problem
from plate_inverse_problem_amd import _native
from plate_inverse_problem_amd.Problem import decoupled_symmetric

FC = 128


def _engine_pattern(p):
    """The pattern, values (26 x nnz) and CSC arrays the engine factorises (Problem._Engine)."""
    active = [k for k in range(26) if not (p.material.is_mps and 6 <= k < 12)]
    keep = p.present[active].any(0) & (p.mats[active] != 0).any(0)
    idx = np.nonzero(keep)[0]
    rows, cols = p.rows[idx], p.cols[idx]
    colptr = np.zeros(p.mat_size + 1, np.int64)
    np.add.at(colptr, cols.astype(np.int64) + 1, 1)
    vals = p.mats[:, idx]
    assert decoupled_symmetric(rows, cols, vals, p.mat_size)
    return rows.astype(np.int32), cols.astype(np.int32), np.cumsum(colptr).astype(np.int32), vals


def _support(p):
    aU, aV, aW = p.averaging_vectors()
    return np.nonzero((aU != 0) | (aV != 0) | (aW != 0))[0].astype(np.int32)


@pytest.fixture(scope="module")
def ortho():
    p = make_problem("orthotropic", ny=6)
    rows, cols, colptr, vals = _engine_pattern(p)
    sym = _native.Symbolic(p.mat_size, colptr, rows, leaf_size=200, symmetric=True)
    mask, act, rest, full = sym.prune(FC, p.vec, _support(p))     # raises if a view's plan or schedule fails a check
    return p, rows, cols, vals, sym, mask.astype(bool), act, rest, full


def _components(p, rows, cols, sym):
    """Per node the connected component of the pattern, and the rows that carry load: a non-zero entry of the
    right-hand side vector, or a coupled row of a Dirichlet node with one."""
    n = p.mat_size
    dirs = sym.export("DIRICHLET")
    cpl = sym.export("COUPLING")
    perm = sym.export("PERM")
    dnode = perm[dirs[:, 0]] if len(dirs) else np.zeros(0, np.int64)
    G = sp.coo_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))
    _, comp = csg.connected_components(G, directed=False)
    loaded = set(np.nonzero(p.vec != 0)[0].tolist())
    for prow, dslot, _ in cpl:
        if p.vec[dnode[dslot]] != 0:
            loaded.add(int(perm[prow]))
    return comp, sorted(loaded)


def test_active_mask_is_the_loaded_components(ortho):
    p, rows, cols, vals, sym, mask, act, rest, full = ortho
    fr = sym.export("FRONTS")
    perm = sym.export("PERM")
    comp, loaded = _components(p, rows, cols, sym)
    loaded_comp = np.zeros(comp.max() + 1, bool)
    loaded_comp[comp[loaded]] = True
    for t, (ns, f, row0, col0, parent, level, off, wv) in enumerate(fr):
        piv = perm[col0:col0 + ns]
        assert len(set(comp[piv])) == 1
        assert mask[t] == loaded_comp[comp[piv[0]]], t
    assert mask.sum() == 255 and len(fr) == 382          # leaf 200: the count of the issue
    # no unloaded tree holds a loaded row; whole trees
    front_of = np.zeros(p.mat_size, np.int64)
    for t, (ns, f, row0, col0, *_r) in enumerate(fr):
        front_of[perm[col0:col0 + ns]] = t
    assert mask[front_of[loaded]].all()
    par = fr[:, 4]
    assert np.array_equal(mask[par >= 0], mask[par[par >= 0]])


def test_views_partition_the_fronts(ortho):
    p, rows, cols, vals, sym, mask, act, rest, full = ortho
    for name in ("factor", "pair", "solve_all"):
        assert np.array_equal(act[name]["nf"] + rest[name]["nf"], full[name]["nf"]), name
    for col in ("nasm", "nitems", "nblocks", "ntiles"):
        # assembly records are padded to 8 per level and view
        if col == "nasm":
            assert np.all(act["factor"][col] + rest["factor"][col] >= full["factor"][col])
        else:
            assert np.array_equal(act["factor"][col] + rest["factor"][col], full["factor"][col]), col
    assert act["factor"]["nf"].sum() == mask.sum()
    # the complement carries no load: no forward reach; the sensor rows on loaded trees stay in the active view
    assert rest["chain"]["nf0"].sum() == 0 and rest["solve_reach0"]["nf"].sum() == 0
    assert act["chain"]["nf1"].sum() > 0 and rest["chain"]["nf1"].sum() > 0


def test_sol_skips_nothing():
    p = make_problem("sol", ny=6)
    rows, cols, colptr, vals = _engine_pattern(p)
    sym = _native.Symbolic(p.mat_size, colptr, rows, leaf_size=200, symmetric=True)
    mask, act, rest, full = sym.prune(FC, p.vec, _support(p))
    assert mask.all()
    today = sym.schedule(FC)
    # every front in the active view: its records are the full plan's, and those that do not depend on the reaches
    # are today's (pfr_symbolic_schedule takes every front as reached)
    for name in act:
        assert np.array_equal(act[name], full[name]), name
    for name in ("factor", "pair", "solve_all"):
        assert np.array_equal(act[name], today[name]), name
    assert rest["factor"]["nf"].sum() == 0


def _forest():
    """Three trees: two 6-node chains and one 5-node chain, block diagonal, tridiagonal blocks."""
    sizes = (6, 6, 5)
    n = sum(sizes)
    r, c = [], []
    o = 0
    for m in sizes:
        for i in range(m):
            for j in (i - 1, i, i + 1):
                if 0 <= j < m:
                    r.append(o + i)
                    c.append(o + j)
        o += m
    order = np.lexsort((r, c))
    r, c = np.asarray(r)[order], np.asarray(c)[order]
    colptr = np.zeros(n + 1, np.int64)
    np.add.at(colptr, c + 1, 1)
    return n, sizes, r.astype(np.int32), c.astype(np.int32), np.cumsum(colptr).astype(np.int32)


def test_synthetic_forest_load_in_one_tree_sensors_in_two():
    n, sizes, r, c, colptr = _forest()
    sym = _native.Symbolic(n, colptr, r, leaf_size=4, symmetric=True)
    rhs = np.zeros(n)
    rhs[2] = 1.0                                   # load on tree 0
    support = np.array([1, 4, 7], np.int32)        # sensor rows on trees 0 and 1
    mask, act, rest, full = sym.prune(64, rhs, support)
    fr = sym.export("FRONTS")
    perm = sym.export("PERM")
    tree = np.repeat(np.arange(3), sizes)
    for t, (ns, f, row0, col0, *_r) in enumerate(fr):
        assert mask[t] == (tree[perm[col0]] == 0), t
    # reach 1 keeps only the loaded tree's rows: its fronts are those holding rows 1 and 4 and their ancestors
    front_of = np.zeros(n, np.int64)
    for t, (ns, f, row0, col0, *_r) in enumerate(fr):
        front_of[perm[col0:col0 + ns]] = t
    want = set()
    for row in (1, 4):
        t = front_of[row]
        while t >= 0:
            want.add(int(t))
            t = fr[t, 4]
    assert act["chain"]["nf1"].sum() == len(want)
    other = set()
    t = front_of[7]
    while t >= 0:
        other.add(int(t))
        t = fr[t, 4]
    assert rest["chain"]["nf1"].sum() == len(other) and rest["chain"]["nf0"].sum() == 0


COUNTS = {"factor": ("nf", "f0_small", "nasm", "nitems", "nblocks", "ntiles"), "pair": ("nf",),
          "chain": ("nf0", "nf1", "nmax", "nsum"), "solve_all": ("nf",), "solve_reach0": ("nf",), "solve_reach1": ("nf",)}


def test_view_takes_the_full_plan_launch_decisions(ortho):
    """On every level it has fronts on, a view's records equal the full plan's in every column but the counts: each
    loaded front runs the kernel form, split and wave count it runs with pruning off."""
    p, rows, cols, vals, sym, mask, act, rest, full = ortho
    assert np.array_equal(full["factor"], sym.schedule(FC)["factor"])
    for view in (act, rest):
        for name, skip in COUNTS.items():
            lv = view[name]["nmax" if name == "chain" else "nf"] > 0
            assert lv.any() or (view is rest and name == "solve_reach0")     # the rest carries no load
            for col in view[name].dtype.names:
                if col not in skip:
                    assert np.array_equal(view[name][col][lv], full[name][col][lv]), (name, col)


def _assert_views_agree(act, rest, full):
    for view in (act, rest):
        for name, skip in COUNTS.items():
            lv = view[name]["nmax" if name == "chain" else "nf"] > 0
            for col in view[name].dtype.names:
                if col not in skip:
                    assert np.array_equal(view[name][col][lv], full[name][col][lv]), (name, col)


@pytest.mark.parametrize("forest", ["F0F0", "F0T"])
@pytest.mark.parametrize("loaded", [0, 1])
def test_fused_bottom_level_is_the_full_plans(forest, loaded):
    """Forests of tests/synthetic.py whose first tree's leaves all fit the fused bottom level (k_front0) and whose second
    tree's do not: the full plan does not fuse level 0, and neither view may, whichever tree the load is on -- the
    bottom level is decided for the whole analysis, a view only lists its own fronts."""
    import synthetic as sy
    pat, op = sy.case(forest, load=(loaded,))
    sym = sy.symbolic(forest)
    for Fc in (64, FC):
        mask, act, rest, full = sym.prune(Fc, op.rhs, op.sup)
        assert 0 < mask.sum() < mask.size
        assert not full["factor"]["fused0"].any()
        assert not act["factor"]["fused0"].any() and not rest["factor"]["fused0"].any()
        _assert_views_agree(act, rest, full)


def test_deep_tree_takes_the_full_plan_launch_decisions(ortho):
    """ny = 6 on the deep tree (leaf 10,000, tests/test_gpu_prune.py::test_views_with_empty_levels): the bending trees'
    leaves all fit the fused bottom level, an in-plane leaf of 6 pivots does not -- no view fuses level 0."""
    p, rows, cols, vals, *_ = ortho
    colptr = np.zeros(p.mat_size + 1, np.int64)
    np.add.at(colptr, cols.astype(np.int64) + 1, 1)
    sym = _native.Symbolic(p.mat_size, np.cumsum(colptr).astype(np.int32), rows, leaf_size=10000, symmetric=True)
    mask, act, rest, full = sym.prune(FC, p.vec, _support(p))
    assert 0 < mask.sum() < mask.size and full["factor"]["maxns"][0] > 4
    assert not full["factor"]["fused0"].any() and not act["factor"]["fused0"].any()
    _assert_views_agree(act, rest, full)


def test_rank_block_shape_takes_the_full_plan_launch_decisions():
    """C3 on the 512-frequency tree (leaf 2,000, chunk 512: C4's rank block), where the loaded trees' L21 item counts
    fall below the pipelined-prefix threshold on levels whose full counts do not: the prefix, like every other shape,
    is decided for the full plan's counts."""
    import bench
    p = bench.build_problem(25, "cpu")
    rows, cols, colptr, vals = _engine_pattern(p)
    sym = _native.Symbolic(p.mat_size, colptr, rows, leaf_size=2000, symmetric=True)
    mask, act, rest, full = sym.prune(512, p.vec, _support(p))
    assert (rest["factor"]["nf"] == 0).any() and (rest["factor"]["nf"] > 0).any()     # a view with empty levels
    for view in (act, rest):
        for name, skip in COUNTS.items():
            lv = view[name]["nmax" if name == "chain" else "nf"] > 0
            for col in view[name].dtype.names:
                if col not in skip:
                    assert np.array_equal(view[name][col][lv], full[name][col][lv]), (name, col)
