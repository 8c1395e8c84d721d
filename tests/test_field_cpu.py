"""No GPU: the host side of the field sweep (include/pfr.h, pfr_field_sweep) -- ``Problem.vertex_rows`` on a small
strip, the C ABI's declaration against the ctypes signature table, and the symbol in the built library."""
import os
import re

import numpy as np
import pytest

from helpers import make_geometry, make_material, make_problem
from plate_inverse_problem_amd import _native


def _dirichlet_rows(p):
    """Rows of the system that hold only their diagonal entry in every matrix (the tgv = -1 rows)."""
    off = (p.mats != 0).any(axis=0) & (p.rows != p.cols)
    has_off = np.zeros(p.mat_size, dtype=bool)
    has_off[p.rows[off]] = True
    return np.nonzero(~has_off)[0]


def test_vertex_rows_on_a_strip():
    p = make_problem("orthotropic", ny=3)
    vr = p.vertex_rows()
    V, n, L = p.mesh.n_vertices, p.mat_size, p.Lh_size
    assert vr.shape == (3, V) and n == 2 * L + p.Mh_size
    assert np.unique(vr).size == 3 * V and vr.min() >= 0 and vr.max() < n
    # each component inside its own block of [u (Lh); v (Lh); w (Mh)]
    assert np.all(vr[0] < L) and np.all((vr[1] >= L) & (vr[1] < 2 * L)) and np.all(vr[2] >= 2 * L)
    # the clamped side x = Lx: its vertices are Dirichlet rows of all three blocks, and no other vertex is
    xy = np.asarray(p.mesh.vertices)
    clamped = np.isclose(xy[:, 0], p.geometry.length)
    assert 0 < clamped.sum() < V
    dirichlet = _dirichlet_rows(p)
    for k in range(3):
        assert np.all(np.isin(vr[k][clamped], dirichlet)), k
        assert not np.any(np.isin(vr[k][~clamped], dirichlet)), k
    # the load sits on the clamped w vertex values (the base excitation)
    assert np.all(p.vec[vr[2][clamped]] != 0) and not np.any(p.vec[vr[2][~clamped]])


def test_vertex_rows_refuses_a_freefem_geometry():
    from plate_inverse_problem_amd.fem import freefem as ffio
    from plate_inverse_problem_amd.fem import plate_varfs, strip_mesh
    from plate_inverse_problem_amd.Geometry import Geometry
    from plate_inverse_problem_amd.Problem import Problem
    geom, acc = make_geometry(ny=3)
    mesh = strip_mesh(geom.length, geom.width, geom.nx, geom.ny)
    ff = plate_varfs(mesh, (geom.accel_x, geom.accel_y), geom.accel_r)
    ff["xtest"], ff["ytest"], ff["tgv"] = geom.accel_x, geom.accel_y, -1.0
    text = ffio.format_plate_output(ff, ffio.to_freefem_mesh(mesh))
    g2 = Geometry.from_freefem_output(text, height=geom.height, accelerometer=acc)
    p2 = Problem(g2, make_material("orthotropic"), acc)
    with pytest.raises(NotImplementedError, match="FreeFEM"):
        p2.vertex_rows()
    with pytest.raises(NotImplementedError):
        p2.solveForwardShapes([100.0])


def test_mode_picture_refuses_freefem_plotting():
    p = make_problem("orthotropic", ny=3)
    with pytest.raises(NotImplementedError, match="FreeFem"):
        p.getModePicture(100.0, use_freefem=True)


def test_field_requests_are_checked_on_the_host():
    p = make_problem("orthotropic", ny=3)
    for bad in ([], [p.mat_size], [-1], [0.5]):
        with pytest.raises(ValueError):
            p.solveForwardField([100.0], dofs=bad)


def _declared_arity(name):
    with open(_native.HEADER_PATH) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"PFR_API\s+[\w\s\*]+?\b" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m, name + " is not declared in include/pfr.h"
    args = m.group(1).strip()
    return 0 if args in ("", "void") else len(args.split(","))


def test_header_and_signature_table_agree():
    assert "pfr_field_sweep" in _native.header_symbols()
    assert _declared_arity("pfr_field_sweep") == 9 == len(_native._PROTOS["pfr_field_sweep"][1])
    assert _declared_arity("pfr_field_tile_rows") == 0 == len(_native._PROTOS["pfr_field_tile_rows"][1])
    assert callable(_native.Solver.field_sweep)
    from plate_inverse_problem_amd.Problem import _LANE_CALLS, _Engine
    assert _LANE_CALLS["field", False][0] == "field_sweep" and callable(_Engine.field_sweep)
    with open(_native.HEADER_PATH) as f:
        txt = f.read()
    for limit in ("gradients through the field", "a loss on field data", "the adjoint field", "a population form",
                  "complex-axis form", "across ranks"):
        assert limit in " ".join(txt.split()).replace(" * ", " "), limit


def test_symbol_resolves_when_the_library_loads():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("libpfr.so is not built")
    try:
        L = _native.lib()
    except OSError as e:              # no HIP runtime to load against on this machine
        pytest.skip(f"libpfr.so does not load without a device runtime: {e}")
    assert L.pfr_field_sweep is not None
    with open(os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc", "launch.hpp")) as f:
        R = int(re.search(r"constexpr int FIELD_R = (\d+);", f.read()).group(1))
    assert _native.field_tile_rows() == R > 0
    # refused before anything touches a device: a null solver
    assert L.pfr_field_sweep(None, 1, None, 0, None, None, None, None, None) == 1
