"""CPU: the synthetic forests of tests/synthetic.py (block-diagonal unions of its shapes) and the views pruning builds
over them (include/pfr.h, pfr_set_prune; csrc/plan.cpp build_plan with a front mask) -- which launch class every level
of the loaded trees' view and of the rest's view runs, for every forest and load tests/test_gpu_synthetic_prune.py
sweeps, read from the library's own ``Symbolic.prune`` (which also runs check_plan and check_schedule on both views).

A line of the tables below is one level of one view (synthetic.class_line): the view's front count, the factor
classes that are on (fused0 = k_front0, lds = k_factor_sym_lds, G4 = k_factor_sym<4>, blk = 16 x 16 Schur blocks,
tiles = 4 x 4 Schur tiles, pu3 = the pipelined L21 prefix), the paired top-down form / its update part and the bottom-up
chain's form / update rows; "-" is a level the view holds no front on.

Together the active views reach every class synthetic.dispatch_classes distinguishes on the single shapes
(test_active_views_reach_every_class), with one exception that cannot be built: a non-empty view with an empty level 0.
A front's level is its height above its deepest leaf, so every tree has a level-0 front; the only view without one is
the empty view (an unloaded solver's active view, or the rest of a fully loaded one), which launches nothing at all and
is asserted on the host only (test_edge_masks).

On the parent of the commit that added this file, F0F0 and F0T failed test_views_take_the_full_plan_decisions: a view
decided the fused bottom level from its own fronts.  Only the pinned component is ordered with ``last``: the pinned F0's
leaves fit k_front0 (at most 4 pivots and 10 update rows), the other component's (the twin ordered freely, or T) do
not, so the full plan does not fuse level 0 -- but the view holding the pinned F0 alone did.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg

import synthetic as sy

FC = 64
N = {"AC": 277, "ETF0": 560, "BFA4": 456, "FA8": 288, "F0F0": 52, "F0T": 232, "F0G": 48, "A4A4": 96, "A8A8": 110,
     "DA8T": 499}

# (active view, rest view) per forest and load, level 0 first, default knobs, 64-frequency chunks
VIEWS = {
    "AC-load0": (                  # load on A: 9 + 1 of the 12 + 2 fronts
        ["9 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"],
        ["3 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"]),
    "AC-load1": (
        ["3 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"],
        ["9 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"]),
    "ETF0-load0": (                # load on E: the 256-pivot root chain; the active view ends at level 2
        ["4 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 blk pu3 level_big/updc plain/rows_z",
         "1 lds G2 pu3 rl/updc rl/rows_zc", "-", "-", "-", "-"],
        ["15 lds G2 blk tiles pu3 rl/updc rl/rows_zc", "3 G4 blk pu3 level_big/updc plain/rows_z",
         "1 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G2 blk pu2 rl/updc rl/rows_zc", "1 G2 blk pu2 rl/updc rl/rows_zc",
         "1 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 rl/updc rl/rows_zc"]),
    "ETF0-load1": (                # load on T: the rest is empty on levels 3-6
        ["9 lds G2 blk pu3 rl/updc rl/rows_zc", "2 G4 blk pu3 level_big/updc plain/rows_z",
         "1 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G2 blk pu2 rl/updc rl/rows_zc", "1 G2 blk pu2 rl/updc rl/rows_zc",
         "1 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 rl/updc rl/rows_zc"],
        ["10 lds G2 blk tiles pu3 rl/updc rl/rows_zc", "2 G4 blk pu3 level_big/updc plain/rows_z",
         "1 lds G2 pu3 rl/updc rl/rows_zc", "-", "-", "-", "-"]),
    "ETF0-load2": (                # load on F0: 4 x 4 Schur tiles; the active view is empty from level 2 up
        ["6 lds G2 tiles pu3 rl/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z", "-", "-", "-", "-", "-"],
        ["13 lds G2 blk pu3 rl/updc rl/rows_zc", "3 G4 blk pu3 level_big/updc plain/rows_z",
         "2 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G2 blk pu2 rl/updc rl/rows_zc", "1 G2 blk pu2 rl/updc rl/rows_zc",
         "1 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 rl/updc rl/rows_zc"]),
    "BFA4-load02": (               # two loaded components (B, A4), one unloaded (F)
        ["13 lds G2 blk pu3 rl/updc rl/rows_zc", "2 G4 pu3 level_big/updc plain/rows_z"],
        ["3 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"]),
    "FA8-load0": (                 # 112 pivots on level 0 (the chain's narrow forms fit), 113 at the root (plain)
        ["4 G4 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 rl/updc plain/rows_z"],
        ["5 G4 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 rl/updc plain/rows_z"]),
    "FA8-load1": (
        ["5 G4 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 rl/updc plain/rows_z"],
        ["4 G4 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 rl/updc plain/rows_z"]),
    "F0F0-load0": (                # the unpinned twin's leaves do not fit k_front0: no fused level in any view
        ["6 G2 tiles pu2 rl/updc rl/rows_zc", "1 lds G2 pu3 rl/updc rl/rows_zc"],
        ["6 G2 tiles pu2 rl/updc rl/rows_zc", "1 lds G2 pu3 rl/updc rl/rows_zc"]),
    "F0F0-load1": (
        ["6 G2 tiles pu2 rl/updc rl/rows_zc", "1 lds G2 pu3 rl/updc rl/rows_zc"],
        ["6 G2 tiles pu2 rl/updc rl/rows_zc", "1 lds G2 pu3 rl/updc rl/rows_zc"]),
    "F0G-load0": (                 # fused in the full plan and in both views
        ["6 fused0 G2 tiles pu2 rl/updc rl/rows_zc", "1 G2 pu3 rl/updc rl/rows_zc"],
        ["6 fused0 G2 tiles pu2 rl/updc rl/rows_zc", "1 G2 pu3 rl/updc rl/rows_zc"]),
    "F0G-load1": (
        ["6 fused0 G2 tiles pu2 rl/updc rl/rows_zc", "1 G2 pu3 rl/updc rl/rows_zc"],
        ["6 fused0 G2 tiles pu2 rl/updc rl/rows_zc", "1 G2 pu3 rl/updc rl/rows_zc"]),
    "A4A4-load0": (
        ["6 G2 blk pu2 rl/updc rl/rows_zc", "1 lds G2 pu3 rl/updc rl/rows_zc"],
        ["6 G2 blk pu2 rl/updc rl/rows_zc", "1 lds G2 pu3 rl/updc rl/rows_zc"]),
    "A8A8-load1": (
        ["5 G2 blk pu2 rl/updc rl/rows_zc", "1 lds G2 pu3 rl/updc rl/rows_zc"],
        ["5 G2 blk pu2 rl/updc rl/rows_zc", "1 lds G2 pu3 rl/updc rl/rows_zc"]),
    "DA8T-load2": (                # load on T (pinned, last in node order): level 3's front is on neither reach
        ["10 lds G2 blk pu3 rl/updc rl/rows_zc", "2 G4 blk pu3 level_big/updc plain/rows_z",
         "2 G2 blk pu3 rl/updc rl/rows_zc", "1 lds G2 blk pu3 rl/updc none/none", "1 G4 pu3 rl/updc rl/rows_zc"],
        ["8 lds G2 blk pu3 rl/updc rl/rows_zc", "2 G4 pu3 level_big/updc plain/rows_z", "-", "-", "-"]),
    "DA8T-load0": (
        ["3 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z", "-", "-", "-"],
        ["15 lds G2 blk pu3 rl/updc rl/rows_zc", "3 G4 blk pu3 level_big/updc plain/rows_z",
         "2 G2 blk pu3 rl/updc rl/rows_zc", "1 lds G2 blk pu3 rl/updc none/none", "1 G4 pu3 rl/updc rl/rows_zc"]),
}

# the active view under the knob variants of synthetic.FOREST_KNOBS (tests/test_gpu_synthetic_prune.py::test_knob_on_off)
KNOB_VIEWS = {
    "F0G-load0-FRONT0=0": ["6 G2 tiles pu2 rl/updc rl/rows_zc", "1 G2 pu3 rl/updc rl/rows_zc"],
    "AC-load1-US2_RL=0": ["3 lds G2 blk pu3 level_big/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"],
    "AC-load1-LS_RL=0": ["3 lds G2 blk pu3 rl/updc nar/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"],
    "AC-load1-US2_RL=0,LS_RL=0": ["3 lds G2 blk pu3 level_big/updc nar/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"],
    "AC-load1-US2_NAR=0": ["3 lds G2 blk pu3 level_big/upd plain/rows_z", "1 G4 pu3 level_big/upd plain/rows_z"],
    "AC-load1-US2_NAR=1000000000": ["3 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"],
    "FA8-load0-US2_RL=0": ["4 G4 blk pu3 level_big/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"],
    "FA8-load0-LS_RL=0": ["4 G4 blk pu3 rl/updc nar/rows_zc", "1 G4 pu3 rl/updc plain/rows_z"],
    "FA8-load0-US2_RL=0,LS_RL=0": ["4 G4 blk pu3 level_big/updc nar/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"],
    "FA8-load0-US2_NAR=0": ["4 G4 blk pu3 level_big/upd plain/rows_z", "1 G4 pu3 level_big/upd plain/rows_z"],
    "FA8-load0-US2_NAR=1000000000": ["4 G4 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 rl/updc plain/rows_z"],
    "AC-load0-SCHUR_BLK_MIN=0": ["9 lds G2 tiles pu3 rl/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"],
    "AC-load0-SCHUR_BLK_MIN=4": ["9 lds G2 blk pu3 rl/updc rl/rows_zc", "1 G4 pu3 level_big/updc plain/rows_z"],
    "A4A4-load0-US2_NAR=0,SOLVE_SPLIT=0": ["6 G2 blk pu2 tiny4/none plain/none", "1 lds G2 pu3 level_small/none plain/none"],
    "A4A4-load0-US2_NAR=0,SOLVE_SPLIT=0,US2_TINY=0": ["6 G2 blk pu2 level_small/none plain/none",
                                                     "1 lds G2 pu3 level_small/none plain/none"],
    "A4A4-load0-US2_NAR=0,SOLVE_SPLIT=0,US2_TINY=4": ["6 G2 blk pu2 tiny4/none plain/none",
                                                     "1 lds G2 pu3 level_small/none plain/none"],
    "A8A8-load1-US2_NAR=0,SOLVE_SPLIT=0": ["5 G2 blk pu2 tiny8/none plain/none", "1 lds G2 pu3 level_small/none plain/none"],
    "A8A8-load1-US2_NAR=0,SOLVE_SPLIT=0,US2_TINY=0": ["5 G2 blk pu2 level_small/none plain/none",
                                                     "1 lds G2 pu3 level_small/none plain/none"],
    "A8A8-load1-US2_NAR=0,SOLVE_SPLIT=0,US2_TINY=4": ["5 G2 blk pu2 level_small/none plain/none",
                                                     "1 lds G2 pu3 level_small/none plain/none"],
}


def _prune(forest, load, Fc=FC):
    _, op = sy.case(forest, load=load)
    return sy.symbolic(forest).prune(Fc, op.rhs, op.sup)


def _component_of_front(forest):
    """Per front of the forest's analysis the component (index into FORESTS[forest]) its pivots belong to."""
    pat, sym = sy.pattern(forest), sy.symbolic(forest)
    comp = np.zeros(pat.n, np.int64)
    for k, (_, _, _, nodes) in enumerate(pat.components()):
        comp[nodes] = k
    fr, perm = sym.export("FRONTS"), sym.export("PERM")
    out = []
    for ns, f, row0, col0, *_r in fr:
        c = set(comp[perm[col0:col0 + ns]])
        assert len(c) == 1                               # no front spans two components
        out.append(c.pop())
    return np.array(out)


@pytest.mark.parametrize("forest", sorted(sy.FORESTS))
def test_forest_patterns(forest):
    """Block diagonal in CSC order, one connected component per part (each with its Dirichlet nodes), every tree
    analysed apart: no front spans two components, and only the pinned component's border is the analysis' ``last``."""
    pat = sy.pattern(forest)
    parts, pin = sy.FORESTS[forest]
    assert pat.n == N[forest] == sum(p.n for _, p in pat.parts) and len(pat.parts) == len(parts)
    key = pat.cols.astype(np.int64) * pat.n + pat.rows
    assert np.all(np.diff(key) > 0) and np.array_equal(np.diff(pat.colptr), np.bincount(pat.cols, minlength=pat.n))
    G = sp.coo_matrix((np.ones(pat.nnz), (pat.rows, pat.cols)), shape=(pat.n, pat.n))
    ncomp, comp = csg.connected_components(G, directed=False)
    assert ncomp == len(parts)
    for k, (leaf_cliques, dirs, border, nodes) in enumerate(pat.components()):
        assert len(set(comp[nodes])) == 1 and comp[nodes[0]] == k
        assert np.isin(dirs, pat.dirichlet).all() and np.isin(np.concatenate(leaf_cliques), nodes).all()
    assert np.array_equal(pat.border, pat.components()[pin][2])
    assert pat.dirichlet.size == sum(p.dirichlet.size for _, p in pat.parts)
    assert len(pat.leaves) == sum(len(p.leaves) for _, p in pat.parts)
    of_front = _component_of_front(forest)
    assert set(of_front) == set(range(len(parts)))
    roots = sy.symbolic(forest).export("FRONTS")[:, 4] < 0
    assert roots.sum() >= len(parts)                     # one tree per component, and one per Dirichlet 1 x 1 front


@pytest.mark.parametrize("forest,load", sy.FOREST_CASES, ids=[sy.forest_id(f, l) for f, l in sy.FOREST_CASES])
def test_forest_operators_qualify(forest, load):
    """The load on the named components only, sensor rows on every component, the symmetric analysis' condition on the
    values, and cond_2 <= COND_MAX (every eighth frequency here; synthetic.reference asserts it on every frequency it
    is built for)."""
    from plate_inverse_problem_amd.Problem import decoupled_symmetric
    pat, op = sy.case(forest, load=load)
    assert decoupled_symmetric(pat.rows, pat.cols, np.vstack([op.S, op.M[None], op.K.real[None], op.K.imag[None]]),
                               pat.n)
    comps = pat.components()
    for k, (_, dirs, _, nodes) in enumerate(comps):
        assert np.any(op.rhs[nodes] != 0) == (k in load)
        assert (op.rhs[dirs[0]] != 0) == (k in load)                 # a loaded Dirichlet node on every loaded component
        assert np.isin(op.sup, nodes).sum() == 4
    assert not np.isin(op.sup, pat.dirichlet).any()
    if load == (0,):                                                 # the default load is component 0's
        assert np.array_equal(sy.case(forest)[1].rhs, op.rhs)
    cond = sy.check_cond([op.matrix_ld(f) for f in sy.FREQS[::8]], forest)
    assert cond.max() <= sy.COND_MAX


@pytest.mark.parametrize("forest,load", sy.FOREST_CASES, ids=[sy.forest_id(f, l) for f, l in sy.FOREST_CASES])
def test_view_classes(forest, load):
    """The table above, and the mask: exactly the loaded components' fronts."""
    mask, act, rest, full = _prune(forest, load)
    assert np.array_equal(mask.astype(bool), np.isin(_component_of_front(forest), load))
    want_act, want_rest = VIEWS[sy.forest_id(forest, load)]
    assert [sy.class_line(d) for d in sy.schedule_classes(act)] == want_act
    assert [sy.class_line(d) for d in sy.schedule_classes(rest)] == want_rest
    assert np.array_equal(act["factor"]["nf"] + rest["factor"]["nf"], full["factor"]["nf"])
    # the rest carries no load; the sensor rows of each side stay with it
    assert rest["chain"]["nf0"].sum() == 0 and act["chain"]["nf0"].sum() > 0
    assert act["chain"]["nf1"].sum() > 0 and rest["chain"]["nf1"].sum() > 0
    assert np.array_equal(act["chain"]["nf1"] + rest["chain"]["nf1"], full["chain"]["nf1"])


def test_the_views_own_fused_lists():
    """F0G: fused in the full plan and in both views, each view listing its own level-0 fronts (4 of the 8 of at most 2
    pivots); F0F0 and F0T: the unpinned component's leaves do not fit (module docstring), so nothing is fused anywhere,
    although the pinned F0's leaves all fit."""
    for forest in ("F0F0", "F0T"):
        fr = sy.symbolic(forest).export("FRONTS")
        leaf = fr[:, 5] == 0
        fits = (fr[:, 0] <= 4) & (fr[:, 1] - fr[:, 0] <= 10)
        of_front = _component_of_front(forest)
        assert fits[leaf & (of_front == 0)].all() and not fits[leaf & (of_front == 1)].all()
        for load in ((0,), (1,)):
            for v in _prune(forest, load)[1:]:
                assert not v["factor"]["fused0"].any()
    for load in ((0,), (1,)):
        mask, act, rest, full = _prune("F0G", load)
        for v, small in ((act, 4), (rest, 4), (full, 8)):
            assert v["factor"]["fused0"][0] == 1 and v["factor"]["f0_small"][0] == small and v["pair"]["tiny"][0] == 4
            assert not v["factor"]["fused0"][1:].any()


@pytest.mark.parametrize("forest,load,env", sy.FOREST_KNOBS, ids=[sy.knob_id(*c) for c in sy.FOREST_KNOBS])
def test_knob_view_classes(forest, load, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mask, act, rest, full = _prune(forest, load)
    assert [sy.class_line(d) for d in sy.schedule_classes(act)] == KNOB_VIEWS[sy.knob_id(forest, load, env)]
    for view in (act, rest):
        assert sy.schedule_disagreements(view, full) == []


def test_active_views_reach_every_class(monkeypatch):
    """Over the GPU cases (default knobs and knob variants) the ACTIVE views run every class dispatch_classes
    distinguishes on the single shapes.  Not reachable: a non-empty view without a level-0 front (module docstring)."""
    seen = []
    for forest, load in sy.FOREST_CASES:
        seen += [d for d in sy.schedule_classes(_prune(forest, load)[1])]
    for forest, load, env in sy.FOREST_KNOBS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            seen += [d for d in sy.schedule_classes(_prune(forest, load)[1])]
    assert any(d is None for d in seen)                                        # a view with an empty (top) level
    seen = [d for d in seen if d is not None]
    for key in ("fused0", "fac_lds_auto", "fac_big", "blk", "tiles"):
        assert {d[key] for d in seen} == {False, True}, key
    assert {d["pair"] for d in seen} == {"tiny4", "tiny8", "rl", "level_small", "level_big"}
    assert {d["pair_upd"] for d in seen} == {"none", "upd", "updc"}
    assert {d["chain"] for d in seen if "chain" in d} == {"plain", "nar", "rl"}
    assert {d["rows"] for d in seen if "rows" in d} == {"none", "rows_z", "rows_zc"}
    assert {d["off_pu"] for d in seen} == {2, 3}
    assert any(d["split_L"] > 1 for d in seen) and any(d["split_U"] > 1 for d in seen)
    assert any(d["split_L"] == 1 for d in seen)
    # every tree has a level-0 front: no non-empty view is empty there
    for forest, load in sy.FOREST_CASES:
        mask, act, rest, full = _prune(forest, load)
        assert act["factor"]["nf"][0] > 0 and rest["factor"]["nf"][0] > 0


_ENVS = ({}, {"PFR_US2_NAR": "0", "PFR_SOLVE_SPLIT": "0"}, {"PFR_US2_RL": "0", "PFR_LS_RL": "0"},
         {"PFR_SCHUR_BLK_MIN": "0"})
_ALL_LOADS = [(f, (k,)) for f in sorted(sy.FORESTS) for k in range(len(sy.FORESTS[f][0]))] + [("BFA4", (0, 2))]


@pytest.mark.parametrize("forest,load", _ALL_LOADS, ids=[sy.forest_id(f, l) for f, l in _ALL_LOADS])
def test_views_take_the_full_plan_decisions(forest, load, monkeypatch):
    """Every forest (F0T included), loaded on each component in turn: both views agree with the full schedule in every
    column that is not a count, under four sets of launch knobs and at chunks of 64 and 128 frequencies."""
    for env in _ENVS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            for Fc in (64, 128):
                mask, act, rest, full = _prune(forest, load, Fc)
                assert 0 < mask.sum() < mask.size
                assert np.array_equal(full["factor"], sy.symbolic(forest).schedule(Fc)["factor"])
                for name, view in (("active", act), ("rest", rest)):
                    assert sy.schedule_disagreements(view, full) == [], (env, Fc, name)


def test_edge_masks():
    pat, sym = sy.pattern("AC"), sy.symbolic("AC")
    of_front = _component_of_front("AC")
    comps = pat.components()
    sup = sy.forest_support(pat)
    # a load on a Dirichlet node of component 1 only: its column reaches C's trees, and nothing of A
    rhs = np.zeros(pat.n)
    rhs[comps[1][1][0]] = 0.7
    mask, act, rest, full = sym.prune(FC, rhs, sup)
    assert mask[of_front == 1].all() and not mask[of_front == 0].any()
    assert mask.sum() == 4 == (of_front == 1).sum()
    # a load on every component: all ones, the active schedule is the full plan's, the rest is empty
    _, op = sy.case("AC", load=(0, 1))
    mask, act, rest, full = sym.prune(FC, op.rhs, sup)
    assert mask.all()
    for name in act:
        assert np.array_equal(act[name], full[name]), name
    assert rest["factor"]["nf"].sum() == 0 and all(d is None for d in sy.schedule_classes(rest))
    # no load at all: nothing is active, the active schedule launches nothing on any level (host only: never swept)
    mask, act, rest, full = sym.prune(FC, np.zeros(pat.n), sup)
    assert not mask.any()
    for name in ("factor", "pair", "solve_all", "solve_reach0", "solve_reach1"):
        assert not act[name]["nf"].any(), name
    assert not act["chain"]["nmax"].any() and all(d is None for d in sy.schedule_classes(act))
    assert np.array_equal(rest["factor"]["nf"], full["factor"]["nf"])


MODEL_SANE = 1e-10          # tests/test_synthetic_cpu.py


@pytest.mark.parametrize("forest,load", [("F0F0", (1,)), ("AC", (1,)), ("BFA4", (0, 2))])
def test_model_and_reference_on_a_forest(forest, load):
    """The reference and the fp64 multifrontal model take a forest as any pattern: rounding-level errors, and x exactly
    zero on the unloaded components in both (their blocks see a zero right-hand side), the adjoint not."""
    pat, op = sy.case(forest, load=load)
    freqs = sy.FREQS[sy.three(sy.FREQS)]
    e_model, e_dense = sy.model_errors(op, sy.symbolic(forest), freqs)
    for k in e_model:
        assert e_model[k] < MODEL_SANE and e_dense[k] < MODEL_SANE, (k, e_model[k], e_dense[k])
    refc = sy.reference(op, freqs)
    off = sy.component_rows(pat, [k for k in range(len(pat.parts)) if k not in load])
    assert off.size and np.all(refc.x[:, off] == 0) and np.all(refc.x_dense[:, off] == 0)
    assert np.any(refc.loss()["lam"][:, off] != 0)
