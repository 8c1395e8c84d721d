"""GPU: what the seven sweep entry points refuse, in which order, and that a refusal leaves nothing behind.

On a fresh solver (shape T of tests/synthetic.py, 64 frequencies, the default check mode) the operator-form state is
set one piece at a time -- operator, rhs, functional, stiffness.  Before each piece the entry point is called with
valid arguments: it returns PFR_ERR_STATE with the message of the first piece that is missing, and every output
buffer (the response, loss, w, jc, h, flags and the pfr_set_check backward errors), filled with a sentinel before,
still holds the sentinel.  After the last piece the same call succeeds, and its outputs are bit for bit those of a
second solver whose state was set in the usual order (make_solver) and that was never refused anything.

Every refused call returns before its first launch, so nothing here runs a kernel on unset state.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import synthetic as sy
from plate_inverse_problem_amd import _native
from test_gpu_synthetic import DEFAULT, DEV, _t, make_solver

pytestmark = pytest.mark.gpu
PFR_ERR_STATE = 5
NF = 64
FREQS = sy.FREQS[:NF]
AXIS = np.array([0.3, -0.2, 1.0])
SENTINEL, FLAG_SENTINEL = -7.25, -77

NO_OP = "operator not set (pfr_set_operator)"
NO_RHS = "rhs not set (pfr_set_rhs)"
NO_FN = "functional not set (pfr_set_functional)"
# per entry point: the message while the operator, the rhs, the functional, the stiffness is the first piece missing
REFUSALS = {
    "pfr_sweep": (NO_OP, NO_RHS, NO_FN, "reverse pass needs pfr_set_stiffness and w_dev"),
    "pfr_sweep_fresh": (NO_OP, NO_RHS, NO_FN, "reverse pass needs pfr_set_stiffness and w_dev"),
    "pfr_jacobian_sweep": (NO_OP, NO_RHS, NO_FN, "jacobian sweep needs pfr_set_stiffness"),
    "pfr_sweep_complex": (NO_OP, NO_RHS, NO_FN, "reverse pass needs pfr_set_stiffness"),
    "pfr_jacobian_sweep_complex": (NO_OP, NO_RHS, NO_FN, "reverse pass needs pfr_set_stiffness"),
    "pfr_population_sweep": ("mass matrix not set (pfr_set_operator)", NO_RHS, NO_FN,
                             "population jacobian sweep needs pfr_set_stiffness"),
    "pfr_hessian_sweep": (NO_OP, NO_RHS, NO_FN, "pfr_set_stiffness not called"),
}


def _buffers(op, value, flag, berr):
    def full(shape, v, dtype):
        return torch.full(shape, v, dtype=dtype, device=DEV)
    c = complex(value, value)
    return dict(fr=full((NF,), value, torch.float64), h=full((NF,), c, torch.complex128),
                loss=full((1,), value, torch.float64), w=full((op.n_stiff,), c, torch.complex128),
                jc=full((NF, op.n_stiff), c, torch.complex128), hess=full((1, op.n_stiff), c, torch.complex128),
                flags=full((NF,), flag, torch.int32), berr=full((NF, 2), berr, torch.float64))


def _host(bufs):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


class _Inputs:
    """The arguments every call shares (kept alive for the calls)."""

    def __init__(self, op, K):
        self.freqs = _t(FREQS)
        self.ref = _t((1.0 + 0.25 * np.arange(NF)) * (1.0 + 0.5j))       # any non-zero reference: the bits are compared
        self.axis = np.ascontiguousarray(AXIS)
        self.member = np.zeros(1, dtype=np.int32)
        self.beta = np.array([op.beta], dtype=np.complex128)
        self.dcoef = np.ascontiguousarray((op.coef * (1.0 + 0.125 * np.arange(op.n_stiff)))[None, :])
        self.Kpop = K
        self.scale = 1.0 / NF


def _call(entry, sv, b, i):
    """The entry point with valid arguments on buffers ``b``; returns (status, pfr_last_error)."""
    L = _native.lib()
    st = torch.cuda.current_stream(DEV).cuda_stream
    dp = lambda a: a.ctypes.data_as(_native._DP)
    f, ref = i.freqs.data_ptr(), i.ref.data_ptr()
    p = {k: v.data_ptr() for k, v in b.items()}
    mse_log, cmse = _native.LOSS_MSE_LOG_AFC, _native.LOSS_CMSE
    if entry in ("pfr_sweep", "pfr_sweep_fresh"):
        rc = getattr(L, entry)(sv._h, NF, f, mse_log, ref, i.scale, p["fr"], p["loss"], p["w"], p["flags"], st)
    elif entry == "pfr_jacobian_sweep":
        rc = L.pfr_jacobian_sweep(sv._h, NF, f, p["fr"], p["jc"], p["flags"], st)
    elif entry == "pfr_sweep_complex":
        rc = L.pfr_sweep_complex(sv._h, NF, f, dp(i.axis), cmse, ref, i.scale, p["h"], p["loss"], p["w"], p["flags"], 0,
                                 st)
    elif entry == "pfr_jacobian_sweep_complex":
        rc = L.pfr_jacobian_sweep_complex(sv._h, NF, f, dp(i.axis), p["h"], p["jc"], p["flags"], st)
    elif entry == "pfr_population_sweep":
        rc = L.pfr_population_sweep(sv._h, NF, f, i.member.ctypes.data_as(_native._I32P), 1, i.Kpop.data_ptr(),
                                    dp(i.beta.view(np.float64)), p["fr"], p["jc"], p["flags"], st)
    else:
        rc = L.pfr_hessian_sweep(sv._h, NF, f, mse_log, ref, i.scale, 1, i.dcoef.ctypes.data_as(C.c_void_p), p["loss"],
                                 p["w"], p["hess"], p["flags"], st)
    return rc, L.pfr_last_error().decode()


def _run(entry, sv, op, inputs):
    """One successful call into fresh outputs (accumulated ones 0, backward errors NaN), read back."""
    b = _buffers(op, 0.0, 0, float("nan"))
    sv.set_check(DEFAULT, sy.BERR_MAX, b["berr"])
    rc, msg = _call(entry, sv, b, inputs)
    assert rc == _native.PFR_OK, (entry, rc, msg)
    out = _host(b)
    sv.set_check(DEFAULT, sy.BERR_MAX, None)
    return out


@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_refused_until_the_state_is_complete(entry):
    _, op = sy.case("T")
    sym = sy.symbolic("T")
    usual, K = make_solver(op, sym, 64)                       # stiffness, operator, rhs, functional
    inputs = _Inputs(op, K)
    want = _run(entry, usual, op, inputs)

    sv = _native.Solver(sym, 0, 64)
    bufs = _buffers(op, SENTINEL, FLAG_SENTINEL, SENTINEL)
    untouched = _host(bufs)
    sv.set_check(DEFAULT, sy.BERR_MAX, bufs["berr"])
    M = _t(op.M)
    pieces = (lambda: sv.set_operator(torch.view_as_real(K), M),
              lambda: sv.set_rhs(op.rhs, op.beta, op.mass_sum),
              lambda: sv.set_functional(op.sup, op.a3, op.ts),
              lambda: sv.set_stiffness(_t(op.S.T), op.e))
    for message, set_piece in zip(REFUSALS[entry], pieces):
        rc, msg = _call(entry, sv, bufs, inputs)
        assert (rc, msg) == (PFR_ERR_STATE, message), (entry, message, rc, msg)
        now = _host(bufs)
        for k, v in untouched.items():
            assert np.array_equal(now[k], v), (entry, message, k)
        set_piece()
    got = _run(entry, sv, op, inputs)
    for k, v in want.items():
        assert np.array_equal(got[k], v, equal_nan=True), (entry, k)
    assert np.all(got["flags"] == 0), got["flags"]
