"""A BaseException on the caller's lane must not desynchronise the lane threads (the ``_Engine._run`` item).

``_run`` issues lane 0's sweep on the calling thread while lanes 1.. issue theirs on their own threads and answer
through a queue.  If lane 0 raised something that is no ``Exception`` (a KeyboardInterrupt in an optimiser loop), the
other lanes' answers used to stay in their queues: the NEXT step then took the stale answer for its own, ordered the
current stream after a lane that had not issued its sweep yet and copied the result buffer before that lane had
written it -- a silently wrong loss and gradient.  Here the step after such an interrupt must equal a fresh engine's,
bit for bit.  Nothing faults: the exception is raised in Python after an ordinary sweep has been issued.

ny = 4 with 512 frequencies: two lanes of 256, a second or two in all.  In the steps under test lane 1 starts issuing
only when lane 0's native call has returned, so that a caller which does not wait for lane 1 is ahead of it by a whole
sweep's enqueue time, and the step buffers are poisoned before the step that is compared, so that a result copied
early cannot equal the right one by having been left there by an earlier step.
"""
import gc
import threading

import numpy as np
import pytest
import torch

from helpers import make_problem

pytestmark = pytest.mark.gpu

N = 512


class _Interrupt(BaseException):
    """Private stand-in for KeyboardInterrupt (which pytest treats specially)."""


def _stepper(p):
    from plate_inverse_problem_amd import _native
    from plate_inverse_problem_amd.Problem import _coeffs18
    freqs = np.linspace(40.0, 600.0, N)
    eng = p.engine(N)
    eng.set_coefficients(_coeffs18(p._transform(), torch.as_tensor(p.parameters * 1.05)).detach().numpy())
    f = torch.as_tensor(freqs, device=eng.device)
    ref = torch.view_as_real(torch.as_tensor((1.0 + 0.0j) * np.linspace(1.0, 2.0, N), device=eng.device))
    return eng, lambda: eng.loss_step(f, _native.LOSS_MSE_LOG_AFC, ref, 1.0 / N)


def test_step_after_an_interrupted_step_equals_a_fresh_engine():
    p, q = (make_problem("orthotropic", ny=4, device="cuda:0") for _ in range(2))
    try:
        _, fresh_step = _stepper(q)
        want_loss, want_w, _, want_flagged = fresh_step()
        eng, step = _stepper(p)
        assert eng.n_lanes == 2 and eng._pool is not None        # lane 1 issues from its own thread
        native = [sv.sweep for sv in eng.solvers]
        state = {"interrupt": True, "lane0_issued": threading.Event()}

        def lane0(*a, **k):
            try:
                native[0](*a, **k)                               # an ordinary sweep ...
            finally:
                state["lane0_issued"].set()
            if state.pop("interrupt", False):
                raise _Interrupt()                               # ... and then, once, the interrupt

        def lane1(*a, **k):
            assert state["lane0_issued"].wait(60)
            native[1](*a, **k)
        eng.solvers[0].sweep, eng.solvers[1].sweep = lane0, lane1
        with pytest.raises(_Interrupt):
            step()
        torch.cuda.synchronize()
        for buf in eng._step_bufs.values():                      # poison the step's result buffer
            buf[0].fill_(1e300)
            buf[2].fill_(7)
        state["lane0_issued"] = threading.Event()
        loss, w, _, flagged = step()
        assert flagged == want_flagged
        assert loss == want_loss
        assert np.array_equal(w, want_w)
    finally:
        p._engine = q._engine = None
        del p, q
        gc.collect()
        torch.cuda.empty_cache()
