"""Population sweeps (pfr_combine_batch, pfr_population_sweep) on the synthetic fronts of ``synthetic.py`` (test
infrastructure, not a test): the members of a population, its lane layout and the two runs the GPU tests compare --
the population sweep, and the ordinary pfr_jacobian_sweep / pfr_sweep of ONE member over the same lanes.

A member is a copy of ``sy.case(shape)``'s operator whose coefficients' real and imaginary parts are each scaled by
``1 + d`` with ``d`` a multiple of 2^-6 in [-1/16, 1/16] (fixed seed).  The coefficients are multiples of 2^-10 and the
stiffness values of 2^-8 (synthetic.make_operator), so every product is a multiple of 2^-24 of magnitude O(1) and
``K = coef @ S`` and ``beta = e @ coef`` stay exact in fp64, as for the base operator; both that and cond_2 <=
COND_MAX of every member's matrices (sy.check_cond; measured <= 35 on A, B, D, T, F0) are asserted here.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

import synthetic as sy
from plate_inverse_problem_amd.Problem import population_layout

COND_EVERY = 13        # check_cond on every 13th of the sweep's frequencies (10 of 130) per member


@functools.lru_cache(maxsize=None)
def members(shape, n_members=3, n_stiff=12, seed=0, load=None):
    """The base operator of ``sy.case(shape)`` (``load``: of a forest, the loaded components) and ``n_members`` member
    operators (a tuple)."""
    _, op = sy.case(shape, n_stiff=n_stiff, load=load)
    rng = np.random.default_rng(7000 + seed)
    out = []
    for p in range(n_members):
        d = rng.integers(-4, 5, size=(2, n_stiff)) / 64.0
        d[0, 0] = (p % 4 + 1) / 64.0                                          # no member equals the base operator
        coef = op.coef.real * (1 + d[0]) + 1j * op.coef.imag * (1 + d[1])
        K = coef @ op.S
        exact = (coef.astype(sy.CLD) @ op.S.astype(sy.LD))
        assert np.array_equal(K.astype(sy.CLD), exact), f"{shape} member {p}: coef @ S is not exact in fp64"
        beta = complex(op.e @ coef)
        assert sy.CLD(beta) == op.e.astype(sy.LD) @ coef.astype(sy.CLD), f"{shape} member {p}: beta is not exact"
        m = dataclasses.replace(op, coef=coef, K=K, beta=beta, _cache={})
        sy.check_cond([m.matrix_ld(f) for f in sy.FREQS[::COND_EVERY]], f"{shape} member {p}")
        out.append(m)
    return op, tuple(out)


def lanes(n_members, freqs, order=None):
    """(lane frequencies (P Fpad,), group table int32, valid mask) of ``population_layout``; ``order``: the member
    owning each block of Fpad lanes (default 0 .. P - 1; a permutation moves the members to other blocks)."""
    index, member, valid = population_layout(n_members, len(freqs))
    if order is not None:
        member = np.asarray(order, dtype=np.int32)[member]
    return np.asarray(freqs, dtype=np.float64)[index], member, valid


def _outputs(nlane, n_stiff, dev, jac):
    nan = float("nan")
    return dict(berr=torch.full((nlane, 2), nan, dtype=torch.float64, device=dev),
                fr=torch.full((nlane + 1,), nan, dtype=torch.float64, device=dev),
                jc=torch.full((nlane + 1, n_stiff), complex(nan, nan), dtype=torch.complex128, device=dev) if jac
                else None,
                flags=torch.zeros(nlane, dtype=torch.int32, device=dev))


def _host(o):
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in o.items()}


def run_population(base, ops, sym, lane_freqs, member, *, max_batch, mode, make_solver, t, jac=True, solver=None):
    """One population sweep through the C ABI on a solver whose own operator and rhs scale are the BASE operator's
    (which no member shares: the sweep must not read them).  fr and jc have one row more than the sweep has lanes,
    prefilled with NaN.  Returns the host copies, ``Kpop`` and the solver."""
    dev = torch.device("cuda", 0)
    nlane = lane_freqs.size
    sv, K = solver or make_solver(base, sym, max_batch)
    Kpop = torch.empty((len(ops), base.pat.nnz), dtype=torch.complex128, device=dev)
    sv.combine_batch(np.stack([m.coef for m in ops]), torch.view_as_real(Kpop))
    o = _outputs(nlane, base.n_stiff, dev, jac)
    sv.set_check(mode, sy.BERR_MAX, o["berr"])
    sv.population_sweep(t(lane_freqs), member, torch.view_as_real(Kpop), np.array([m.beta for m in ops]), o["fr"],
                        jc=None if o["jc"] is None else torch.view_as_real(o["jc"]), flags=o["flags"])
    out = _host(o)
    out.update(Kpop=Kpop.cpu().numpy(), solver=(sv, K))
    return out


def run_member(op, sym, lane_freqs, *, max_batch, mode, make_solver, t, jac=True):
    """The existing single-theta sweep of member ``op`` over the same lanes on a solver of the same max_batch:
    pfr_jacobian_sweep (``jac``) or the forward pfr_sweep."""
    dev = torch.device("cuda", 0)
    sv, _ = make_solver(op, sym, max_batch)
    o = _outputs(lane_freqs.size, op.n_stiff, dev, jac)
    sv.set_check(mode, sy.BERR_MAX, o["berr"])
    if jac:
        sv.jacobian_sweep(t(lane_freqs), torch.view_as_real(o["jc"]), fr=o["fr"], flags=o["flags"])
    else:
        sv.sweep(t(lane_freqs), fr=o["fr"], flags=o["flags"])
    return _host(o)


def same_lanes(pop, one, sel, what=("fr", "jc", "flags", "berr")):
    """Bitwise equality of the population sweep's and the single-theta sweep's results at the lanes ``sel``."""
    for k in what:
        if pop[k] is None:
            continue
        a, b = pop[k][:-1] if k in ("fr", "jc") else pop[k], one[k][:-1] if k in ("fr", "jc") else one[k]
        assert np.array_equal(a[sel], b[sel], equal_nan=True), k
        if k in ("fr", "jc"):
            assert not np.isnan(a[sel].view(np.float64)).any(), k
