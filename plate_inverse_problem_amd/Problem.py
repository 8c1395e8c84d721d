"""``Problem``: differentiable plate frequency response on MI355X.

Mirrors ``source/jax_plate/Problem.py`` (constructor semantics, ``getFRFunction``,
``solveForward``, ``getLossFunction``, ``solveInverse``) -- the unsymmetric
(accelerometer) branch, which is the reference's only live branch (SURVEY.md
§2).  The reference's JAX ``jit(vmap(_solve))`` + UMFPACK-callback hot path is
replaced by one fused HIP sweep per frequency chunk (``_native.Solver.sweep``):

    assemble K(theta) - omega^2 M -> static-pivot multifrontal LU -> L/U solves
    -> FR functional [-> loss cotangent -> U^T/L^T adjoint solves ->
    stiffness contraction]

Autodiff: the sweep is a ``torch.autograd.Function`` of the 18 complex laminate
coefficients ``c = (A, B, D)``; torch autograd carries the gradient through the
material transform to ``theta``.  Gradients are exact adjoints (no finite
differences), with the reference's non-conjugate transpose (``Sparse.py:211-219``).
"""
from __future__ import annotations

import json
import os
import warnings
import weakref
from types import SimpleNamespace
from typing import Callable

import numpy as np
import scipy.sparse as sp
import torch

from . import _native
from ._abd_jet import coeffs18 as _jet_coeffs18, _cached_abd
from .Accelerometer import Accelerometer, AccelerometerParams
from .Geometry import Geometry, GeometryParams
from .Material import Material, get_material
from .fem.layout import load_matrices_unsymm, union_pattern

RHS_WEIGHTS_D = np.array([1.0, 2.0, 4.0, 1.0, 4.0, 4.0])   # Problem.py:447-448
KB_SLICE = slice(6, 12)                                     # the 6 coupling (B) matrices
_PKG_DIR = os.path.dirname(os.path.abspath(__file__))


def _default_device():
    if not torch.cuda.is_available():
        raise _native.NativeError("the plate solver runs on a ROCm GPU; torch.cuda.is_available() is False "
                                  "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def decoupled_symmetric(rows, cols, vals, n, rtol=1e-10) -> bool:
    """True when every matrix ``vals[k]`` on the (rows, cols) pattern is complex symmetric
    once the Dirichlet rows -- rows holding only their diagonal entry, the ``tgv = -1`` rows
    of pyFFInterface.py:176 -- and their columns are taken out (the condition of the
    symmetric analysis, include/pfr.h ``pfr_symbolic_options.symmetric``)."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    off = rows != cols
    isdir = np.zeros(n, dtype=bool)
    isdir[rows[~off]] = True
    isdir[rows[off]] = False
    keep = ~isdir[rows] & ~isdir[cols]
    r, c = rows[keep], cols[keep]
    for v in np.atleast_2d(vals):
        A = sp.csr_matrix((np.asarray(v)[keep], (r, c)), shape=(n, n))
        amax = abs(A).max() if A.nnz else 0.0
        if amax > 0 and abs(A - A.T).max() > rtol * amax:
            return False
    return True


class _LaneThread:
    """One solver lane's host thread: the lane's launches are issued here while the caller's thread issues lane 0's
    (the C calls release the GIL).  A queue pair instead of a ThreadPoolExecutor: submit is one C-level put (the
    executor's submit took ~15 us of the step-to-step turnaround before lane 0's first launch)."""

    def __init__(self):
        import queue
        import threading
        self._in, self._out = queue.SimpleQueue(), queue.SimpleQueue()
        self._th = threading.Thread(target=_LaneThread._loop, args=(self._in, self._out), name="pfr-lane",
                                    daemon=True)
        self._th.start()
        # the thread holds the queues only: an engine dropped without close() ends its lane threads
        weakref.finalize(self, self._in.put, None)

    @staticmethod
    def _loop(qin, qout):
        while True:
            item = qin.get()
            if item is None:
                return
            fn, arg = item
            try:
                fn(arg)
                qout.put(None)
            except BaseException as e:       # noqa: BLE001 -- handed to the caller's result()
                qout.put(e)
            del fn, arg, item

    def submit(self, fn, arg):
        self._in.put((fn, arg))

    def result(self):
        """The exception the submitted call raised, or None; waits for it."""
        return self._out.get()

    def close(self):
        self._in.put(None)
        self._th.join()


# (kind of sweep, sensing axis given) -> (the _native.Solver method of a lane's call, its keyword for the response);
# a new kind of sweep is one more row here and one public _Engine method that states its request (_lane_request)
_LANE_CALLS = {("sweep", False): ("sweep", "fr"), ("sweep", True): ("sweep_complex", "h"),
               ("jacobian", False): ("jacobian_sweep", "fr"), ("jacobian", True): ("jacobian_sweep_complex", "h"),
               ("population", False): ("population_sweep", "fr"), ("hessian", False): ("hessian_sweep", None),
               ("field", False): ("field_sweep", "fr"), ("field_loss", False): ("field_loss_sweep", None),
               ("inertia", False): ("inertia_sweep", "resp"), ("inertia", True): ("inertia_sweep", "resp")}
_NO_ARGS = {}


class _Engine:
    """Device state of one Problem: symbolic analysis, operator data and ``lanes``
    solvers, each with its own workspace and HIP stream.  A sweep splits its
    frequencies into one contiguous block per lane and runs the lanes
    concurrently; their kernels share the CUs (measured at C3: 2 lanes x 2,048
    frequencies 4 % faster than 1 lane x 4,096, 3-4 lanes slower)."""

    def __init__(self, prob: "Problem", device, n_freqs: int, max_batch: int | None, lanes: int | None = None,
                 symmetric: bool | None = None):
        self.device = device
        mats = prob.mats
        # structural pattern of the matrices that can be non-zero: for a mid-plane
        # symmetric material the B coefficients are identically zero, the KB
        # entries carry exact zeros and are dropped from the factorised pattern.
        active = [k for k in range(26) if not (prob.material.is_mps and KB_SLICE.start <= k < KB_SLICE.stop)]
        # entries that are exactly zero in every active matrix (explicit zeros of the FE layout)
        # are left out too: they change nothing, and with them out the Dirichlet rows hold
        # only their diagonal entry
        keep = prob.present[active].any(axis=0) & (mats[active] != 0).any(axis=0)
        self.keep = np.nonzero(keep)[0]
        rows, cols = prob.rows[self.keep], prob.cols[self.keep]
        n = prob.mat_size
        colptr = np.zeros(n + 1, dtype=np.int64)
        np.add.at(colptr, cols.astype(np.int64) + 1, 1)
        colptr = np.cumsum(colptr).astype(np.int32)
        vals = mats[:, self.keep]
        if symmetric is None:
            symmetric = os.environ.get("PFR_SYMMETRIC", "1") != "0"
        # symmetric mode when every matrix is complex symmetric away from the Dirichlet rows
        # (checked on the values): only L is formed, U = diag(U) L^T
        self.symmetric = bool(symmetric) and decoupled_symmetric(rows, cols, vals, n)
        # tuning knobs of the symbolic analysis (defaults in include/pfr.h): PFR_LEAF_SIZE,
        # PFR_RELAX="small,mid,big[,zmid,zbig]" (supernode amalgamation pivot limits and zero fractions), PFR_MAX_NS,
        # PFR_MD_DELTA, PFR_ORDERING (2: the exact-minimum-degree leaves of rounds 1-3, for A/B runs)
        env = lambda k: os.environ.get(k)  # noqa: E731
        self._sym_args = (n, colptr, rows.astype(np.int32))
        self._sym_kw = dict(symmetric=self.symmetric, ordering=int(env("PFR_ORDERING") or 0),
                            relax=tuple(float(v) for v in env("PFR_RELAX").split(",")) if env("PFR_RELAX") else None,
                            max_ns=int(env("PFR_MAX_NS")) if env("PFR_MAX_NS") else None,
                            md_delta=int(env("PFR_MD_DELTA")) if env("PFR_MD_DELTA") else None)
        self._leaf_env = int(env("PFR_LEAF_SIZE")) if env("PFR_LEAF_SIZE") else None
        self._syms, self.sym = {}, None
        self._use_symbolic(n_freqs)
        self._lanes_req = int(os.environ.get("PFR_LANES", "2")) if lanes is None else int(lanes)
        self._lane_freqs = max(64, int(os.environ.get("PFR_LANE_FREQS", "256")))   # frequencies per lane at least
        self._fixed_batch = max_batch
        self.solvers, self.streams, self._pool = [], [], None
        self._spin_wait = os.environ.get("PFR_STEP_WAIT", "spin") != "block"
        self.n_lanes = 0
        self._seeded = False
        self._sized_for = set()
        self._step_bufs, self._step_views = {}, {}      # loss_step's buffers and lane request: one shape at a time
        self._kidx_dev = (None, None)                   # expand's index on the device it was last used on
        # the coefficient matrices contracted for the gradient: all 18, or the 12 of A and D when the
        # coupling coefficients B vanish identically (mid-plane symmetric materials: dB/dtheta = 0, so
        # their gradient partials are exactly zero and need not be formed)
        self.kidx = np.r_[0:6, 12:18] if prob.material.is_mps else np.arange(18)
        self.n_stiff = int(self.kidx.size)
        self.stiff = torch.as_tensor(np.ascontiguousarray(vals[self.kidx].T), device=device)  # (nnz, n_stiff)
        I0, I0c, I2, I2c = prob.I0, prob.I0Corr, prob.I2, prob.I2Corr
        mass = I0 * (vals[18] + vals[20] + vals[22]) + I0c * (vals[19] + vals[21] + vals[23]) \
            + I2 * vals[24] + I2c * vals[25]                                                  # Problem.py:441-443
        self.mass = torch.as_tensor(np.ascontiguousarray(mass), device=device)
        self.mass_sum = I0 + I0c + I2 + I2c
        # inertia sweeps (set_inertia / inertia_sweep): the constants the operator holds now, the problem's own, and --
        # built at first use -- the four mass matrices G_j on the host and as the device table the lanes register
        self.inertia = self.own_inertia = (I0, I0c, I2, I2c)
        self._mats = prob.mats
        self._G = self._G_dev = None
        self._inertia_lanes = None     # the solvers pfr_set_inertia was called on
        self.K = torch.empty(self.keep.size, dtype=torch.complex128, device=device)
        self.e = np.concatenate([np.zeros(12), RHS_WEIGHTS_D])
        aU, aV, aW = prob.averaging_vectors()
        self._sup = np.nonzero((aU != 0) | (aV != 0) | (aW != 0))[0]
        self._a3 = np.stack([aU[self._sup], aV[self._sup], aW[self._sup]])
        self._ts = prob.accelerometer.transverse_sensitivity
        self.rhs = prob.vec
        self._coef_key = None
        self.last_berr = None          # (F, 2) componentwise backward errors of the last sweep (device; a loss
                                       # step's buffer is reused -- overwritten -- by the next loss step)
        self.last_flags = None         # its status flags (host)
        # backward-error checks of every solve (pfr_set_check) and the functional correction (fr to
        # second order in the solve's error, the accuracy of the reference's refined UMFPACK solves) by
        # default; PFR_CHECK=<PFR_CHECK_* bits> / PFR_CHECK_TOL override; refinement (bits 4, 16) off by default
        self.check_mode = int(os.environ.get("PFR_CHECK", str(_native.PFR_CHECK_FORWARD | _native.PFR_CHECK_ADJOINT
                                                              | _native.PFR_CHECK_CORRECT)))
        self.check_tol = float(os.environ.get("PFR_CHECK_TOL", "1e-10"))
        # the selective adjoint refinement's group threshold (first-order fr error estimate)
        self.refine_tol = float(os.environ.get("PFR_REFINE_TOL", "2e-8"))
        self.ensure(n_freqs)

    def leaf_size_for(self, n_freqs: int) -> int:
        """Nested-dissection leaf size of the ordering for a sweep of ``n_freqs`` frequencies (DESIGN.md
        section 8, round 3).  Parts of at most this many nodes are ordered by multiple minimum degree:
        10,000 (one dissection at C3) gives the least fill and Schur-complement traffic but a deep tree
        (38 levels), whose per-level chains cost nothing when each level has thousands of workgroups
        and dominate the sparse solve passes of narrow sweeps; those get the shallower trees of more
        dissection levels.  C3, freq-solves/s at leaf 96 / 500 / 3,000 / 10,000 (late round 3, with the
        functional from the bottom-up passes): 512 frequencies 32.7k / 33.0k / 31.3k / 30.5k, 1,024
        41.1k / 42.8k / 43.5k / 44.0k, 2,048 - / 49.8k / 51.4k / 52.7k.  Round 4 (current kernels, alternated
        runs, profiles/r04/experiments/leaf*.txt): 512 frequencies leaf 96 / 150 / 200 / 250 / 300: 32.2-33.4k /
        34.2k / 34.9-35.1k / 33.4k / 33.3-33.9k; 1,024 leaf 600 / 1,000 / 2,000 / 10,000: 43.2k / 45.8-46.1k / 46.7k /
        44.5-44.9k; 2,048 leaf 1,000 / 2,000 / 10,000: 53.0k / 55.2k / 55.4-55.8k; 4,096: 10,000 best.  Round 5, with
        512 frequencies on two lanes of 256: leaf 120 / 200 / 350 / 700 / 1,000 / 2,000 / 5,000 / 10,000: 36.1-36.2k /
        36.8-37.0k / 36.7-37.2k / 36.8-36.9k / 37.9-38.4k / 36.2-38.0k / 38.1-38.3k / 33.5k; 1,024 leaf 1,000 / 2,000 /
        5,000 / 10,000: 48.4-48.6k / 50.3-50.4k / 50.2-50.8k / 48.5k; 2,048: 5,000 = 10,000 (gpurun_out/r6_leaf*).
        Round 6, C4's rank block (tools/ab_proxy.sh, 7 alternations on two boxes): leaf 600 / 1,000 / 2,000 / 3,000
        40.7-41.7k / 41.3-42.9k / 41.5-43.4k / 40.6-41.2k, 2,000 ahead of 1,000 in 6 of 7 pairs (+0.8 %;
        gpurun_out/lf_p512, lf2_p512): 2,000 for up to 512 frequencies."""
        if self._leaf_env is not None:
            return self._leaf_env
        n_freqs = max(1, n_freqs)
        return 200 if n_freqs <= 256 else 2000 if n_freqs <= 1024 else 10000

    def _use_symbolic(self, n_freqs: int) -> bool:
        """Select (building once) the symbolic analysis for a sweep width; True if it changed."""
        leaf = self.leaf_size_for(n_freqs)
        if leaf not in self._syms:
            self._syms[leaf] = _native.Symbolic(*self._sym_args, leaf_size=leaf, **self._sym_kw)
        changed = self.sym is not self._syms[leaf]
        self.sym = self._syms[leaf]
        self.stats = self.sym.stats()
        return changed

    def _lanes_for(self, n_freqs: int) -> int:
        """Solver lanes for a sweep of ``n_freqs``: a lane per PFR_LANE_FREQS (256) frequencies at most.  Round 3
        kept 512 frequencies on one lane (27.1k against 26.4k freq-solves/s with two); with round 5's kernels two
        lanes of 256 overlap each other's narrow-level chains and kernel drains: 36.2-36.8k -> 36.6-37.6k over five
        alternations, four lanes of 128 27.5k (profiles/EXPERIMENTS.md, round 5).  Round 6, C4's rank block
        (tools/strong_proxy.py --one 512, three alternations): two lanes of 256 41.5-41.6k, one lane of 512
        40.6-40.7k (gpurun_out/r6u); 512 frequencies spread over the band favoured one lane (41.7-41.8k against
        41.1-41.2k, gpurun_out/r6k_e512) -- the rank block is the C4 workload."""
        return max(1, min(self._lanes_req, -(-max(1, n_freqs) // self._lane_freqs)))

    def _shape_for(self, n_freqs: int):
        """(lanes, frequencies per chunk) for a sweep of ``n_freqs``: up to ``lanes`` lanes of at
        least 64 frequencies; per lane as many frequencies per chunk as fit in its share of ~85 %
        of the free HBM (multiple of 64, <= 4096), in even chunks."""
        n_freqs = max(1, n_freqs)
        n_lanes = self._lanes_for(n_freqs)
        if self._fixed_batch:
            return n_lanes, int(self._fixed_batch)
        per_lane = -(-n_freqs // n_lanes)
        free, _ = torch.cuda.mem_get_info(self.device)
        n = self._sym_args[0]
        # ours, if rebuilt: the workspaces, and the refinement's seed vectors the solvers already hold
        free += sum(self.sym.workspace_bytes(sv.max_batch) + (n * sv.max_batch * 16 if self._seeded else 0)
                    for sv in self.solvers)
        per64 = self.sym.workspace_bytes(64)
        if self.check_mode & _native.PFR_CHECK_REFINE_ADJ:
            per64 += n * 64 * 16     # the refinement's fr seed vector (n x Fc), allocated on first use
        cap = max(64, min(4096, int(0.85 * free / n_lanes / per64) * 64))
        n_chunks = -(-per_lane // cap)
        return n_lanes, (-(-per_lane // n_chunks) + 63) // 64 * 64

    def ensure(self, n_freqs: int, refit: bool = False):
        """Size the lanes for a sweep of ``n_freqs`` frequencies.  The solvers are rebuilt only when
        the sweep needs more lanes or larger chunks than the current ones have (a small first call
        must not pin 1 lane and 64-frequency chunks on every later large sweep); smaller sweeps run
        on the existing solvers -- with their lanes and their ordering: the widest sweep so far fixes the
        elimination tree (a C4 rank, whose engine is first sized for its 512-frequency share, gets the
        shallow narrow-sweep tree; a 512-frequency sweep after a 4,096-frequency one runs on the deep
        tree, correct but slower)."""
        if self.solvers and not refit:
            per_lane = -(-max(1, n_freqs) // self.n_lanes)
            if n_freqs in self._sized_for or (self._lanes_for(n_freqs) <= self.n_lanes and per_lane <= self.max_batch):
                return
        self._sized_for.add(n_freqs)
        old = self.sym
        if self.solvers:
            self._use_symbolic(n_freqs)   # a rebuild for a wider sweep may take a deeper ordering
        lanes, batch = self._shape_for(n_freqs)
        if refit:
            # re-sized for what now has to fit beside the workspaces (set_check adding the refinement's seed
            # vectors): smaller chunks only when the current ones no longer fit
            if self.solvers and batch >= self.max_batch:
                return
            lanes = max(lanes, self.n_lanes)
        else:
            if self.solvers and lanes <= self.n_lanes and batch <= self.max_batch and self.sym is old:
                return
            lanes = max(lanes, self.n_lanes)
            batch = max(batch, self.max_batch if self.solvers else 0)
        if self.solvers:
            torch.cuda.synchronize(self.device)
        self.solvers, self.streams = [], []       # free the old workspaces before allocating
        if self._pool is not None:
            for t in self._pool:
                t.close()
            self._pool = None
        self.n_lanes = lanes
        self.solvers = [_native.Solver(self.sym, self.device.index, batch) for _ in range(lanes)]
        self._seeded = False           # no refinement seed vector allocated in the new solvers yet
        self.streams = [torch.cuda.Stream(self.device) for i in range(lanes)]
        if lanes > 1 and os.environ.get("PFR_PAR_LAUNCH", "1") != "0":
            self._pool = [_LaneThread() for _ in range(lanes - 1)]
        # pruning (include/pfr.h, pfr_set_prune; PFR_PRUNE=0: off): only the elimination trees the load reaches are
        # factorised and solved -- for a mid-plane-symmetric material the in-plane block carries none
        prune = self.symmetric and os.environ.get("PFR_PRUNE", "1") != "0"
        for sv in self.solvers:
            sv.set_stiffness(self.stiff, self.e[self.kidx])
            sv.set_operator(torch.view_as_real(self.K), self.mass)      # K(theta) shared by the lanes
            sv.set_functional(self._sup, self._a3, self._ts)
            if prune:
                sv.set_prune(True)
            sv.set_check(self.check_mode, self.check_tol)
            sv.set_refine_tol(self.refine_tol)
        self._coef_key = None          # new solvers: rhs scale not set yet

    def set_check(self, mode: int | None = None, tol: float | None = None):
        """Backward-error check mode (PFR_CHECK_* bits) and flag tolerance of every lane.  Turning on the
        selective adjoint refinement (PFR_CHECK_REFINE_ADJ) re-sizes the chunks when its seed vectors (n x chunk
        per lane, allocated on first use) would not fit beside the current workspaces."""
        adds_refine = mode is not None and bool(int(mode) & _native.PFR_CHECK_REFINE_ADJ) \
            and not (self.check_mode & _native.PFR_CHECK_REFINE_ADJ)
        if mode is not None:
            self.check_mode = int(mode)
        if tol is not None:
            self.check_tol = float(tol)
        for sv in self.solvers:
            sv.set_check(self.check_mode, self.check_tol)
        if adds_refine and self.solvers:
            self.ensure(max(self._sized_for) if self._sized_for else self.n_lanes * self.max_batch, refit=True)

    @property
    def solver(self):
        return self.solvers[0]

    @property
    def max_batch(self) -> int:
        return self.solver.max_batch

    def expand(self, v: torch.Tensor) -> torch.Tensor:
        """Partials over the contracted matrices (last axis n_stiff) -> over all 18 (zeros elsewhere)."""
        if self.n_stiff == 18:
            return v
        out = torch.zeros(v.shape[:-1] + (18,), dtype=v.dtype, device=v.device)
        # the index on the device once: a per-call host->device copy of it blocked the host until the
        # sweep had finished, so the small kernels after the sweep were only enqueued then
        key = str(v.device)
        if self._kidx_dev[0] != key:
            self._kidx_dev = (key, torch.as_tensor(self.kidx, device=v.device))
        out[..., self._kidx_dev[1]] = v
        return out

    def set_coefficients(self, c: np.ndarray):
        """Precombine K(theta) = sum_k c_k S_k on the device and the rhs scale."""
        key = c.tobytes()
        if key == self._coef_key:
            return
        self.solver.combine(np.asarray(c)[self.kidx], torch.view_as_real(self.K))
        beta = complex(self.e @ c)
        for sv in self.solvers:
            sv.set_rhs(self.rhs, beta, self.mass_sum)
        if self._coef_key is None:
            self._pruned_stats()
        self._coef_key = key

    def _pruned_stats(self):
        """``stats`` of what the sweeps factorise: under pruning the loaded trees' fronts (the whole pattern's
        figures beside them as ``*_full``); ``Symbolic.stats()`` itself is unchanged."""
        full = self.sym.stats()
        st = dict(full)
        mask = self.solver.active_fronts().astype(bool)
        if not mask.all():
            fr = self.sym.export("FRONTS")[mask]
            ns, f = fr[:, 0].astype(np.float64), fr[:, 1].astype(np.float64)
            # sum over the pivots k of a front of 8 m^2 + 8 m, m = f - k - 1 (symbolic.cpp)
            a, b = f - ns, f - 1.0          # m runs over a .. b
            s1 = (b * (b + 1) - (a - 1) * a) / 2.0
            s2 = (b * (b + 1) * (2 * b + 1) - (a - 1) * a * (2 * a - 1)) / 6.0
            part = dict(n_fronts=int(mask.sum()), total_rows=int(fr[:, 1].sum()),
                        factor_entries=int((fr[:, 1] ** 2).sum()),
                        nnz_lu=int((2 * fr[:, 0] * fr[:, 1] - fr[:, 0] ** 2).sum()),
                        factor_flops=float((8.0 * s2 + 8.0 * s1).sum()), max_front=int(fr[:, 1].max()))
            for k, v in part.items():
                st[k + "_full"] = full[k]
                st[k] = v
        self.stats = st

    def _split(self, n):
        """Contiguous frequency block of each lane (multiples of 64 but the last)."""
        per = (-(-n // self.n_lanes) + 63) // 64 * 64
        return [(min(n, i * per), min(n, (i + 1) * per)) for i in range(self.n_lanes)]

    def _run(self, call, n, accum, lane_bufs=None, raw=False):
        """``call(solver, lo, hi, bufs)`` on every lane's stream; per-lane ``accum``
        buffers (zeros like each given tensor) are summed into the given tensors -- or, with
        ``lane_bufs`` (the caller's zeroed per-lane buffers, one list per lane), accumulated there and
        left to the caller.  With several lanes each lane's launches are issued from its own host
        thread (the C calls release the GIL): issued one after the other, the second lane started a
        whole sweep's enqueue time (~9 ms) after the first and finished that much later.  ``raw``: ``call`` issues
        native work only and takes the lane's stream handle as a fifth argument (no torch device / stream context
        per lane on the step's critical path)."""
        cur = torch.cuda.current_stream(self.device)
        jobs = []
        spans = [(i, sv, st, lo, hi) for i, (sv, st, (lo, hi)) in
                 enumerate(zip(self.solvers, self.streams, self._split(n))) if hi > lo]
        # the lanes ordered after the current stream and it after them by pfr_stream_order (one C call each;
        # Stream.wait_stream makes and destroys an event per call: host time before the first launch)
        cur_h = cur.cuda_stream
        for i, sv, st, lo, hi in spans:
            # the lane's accumulation buffers are zero-filled on the current stream BEFORE the lane
            # stream is ordered after it (k_reduce accumulates into them with +=); one lane accumulates
            # straight into the given tensors
            if lane_bufs is not None:
                bufs = lane_bufs[i]
            else:
                bufs = list(accum) if len(spans) == 1 else [None if a is None else torch.zeros_like(a) for a in accum]
            _native.stream_order(st.cuda_stream, cur_h)
            jobs.append((i, sv, st, lo, hi, bufs))
        if _HT is not None:
            _HT("lanes_ordered")

        def lane(job):
            _, sv, st, lo, hi, bufs = job
            if raw:
                call(sv, lo, hi, bufs, st.cuda_stream)
                return
            with torch.cuda.device(self.device), torch.cuda.stream(st):
                call(sv, lo, hi, bufs)

        errs, waiting, mine = [], [], jobs
        try:
            if len(jobs) > 1 and self._pool is not None:
                # lanes 1.. on their threads, lane 0 on this thread meanwhile (one thread handoff less before the
                # first launch: the GPU idles from the previous step's result until then)
                mine = jobs[:1]
                for t, j in zip(self._pool, jobs[1:]):
                    t.submit(lane, j)
                    waiting.append(t)
                if _HT is not None:
                    _HT("submitted")
            for j in mine:
                try:
                    lane(j)
                except Exception as e:       # noqa: BLE001 -- re-raised once every lane is joined
                    errs.append(e)
                    break
        finally:
            # whatever this thread's lane raised -- a BaseException such as KeyboardInterrupt passes through here --
            # every submitted lane's result is collected (left in its queue it would answer the NEXT call's wait,
            # before that call's lane had issued anything): every lane has issued its work (or failed) ...
            errs += [e for e in [t.result() for t in waiting] if e is not None]
            for i, _, st, _, _, bufs in jobs:    # ... and the current stream is ordered after all of them
                _native.stream_order(cur_h, st.cuda_stream)
                for b in bufs:
                    if b is not None:
                        b.record_stream(cur)
        if errs:
            raise errs[0]
        if lane_bufs is not None:
            return
        for _, _, st, _, _, bufs in jobs:
            for a, b in zip(accum, bufs):
                if a is not None and b is not a:
                    a.add_(b)

    def _lane_request(self, kind, n, per_freq, axis=None, resp=None, berr=None, per_group=None, own=None, **fixed):
        """A sweep request as what each lane calls: ``(Solver method, {lo: (the lane's rows of berr, its keyword
        arguments)})`` over the lanes that sweep some of ``n`` frequencies.  ``kind`` and whether a sensing ``axis`` (3
        real numbers) is given pick the method (``_LANE_CALLS``).  This is the one place the per-frequency tensors --
        ``per_freq`` by the method's names, the response ``resp`` (float64, or complex128 with an axis) under the
        method's name for it, ``berr`` (n, 2); None stays None -- are cut into the lanes' ``[lo:hi]`` blocks, and
        ``per_group``'s host arrays (a population's member table) into their entries per 64-frequency group; the
        ``fixed`` arguments go to every lane as they are.  ``own`` (names, one buffer list per lane): the lanes'
        accumulators are the caller's; the arguments are then complete, with them and the lane's stream handle
        (``loss_step``, which keeps the request across steps: cutting costs host time on the turnaround)."""
        method, resp_name = _LANE_CALLS[kind, axis is not None]
        if resp is not None:
            per_freq = {**per_freq, resp_name: resp if axis is None else torch.view_as_real(resp)}
        if axis is not None:
            fixed["axis"] = axis
        cut = lambda t, lo, hi: None if t is None else t[lo:hi]              # noqa: E731
        lanes = {}
        for i, (lo, hi) in enumerate(self._split(n)):
            if hi > lo:
                kw = {**{k: cut(t, lo, hi) for k, t in per_freq.items()}, **fixed,
                      **{k: a[lo // 64:(hi + 63) // 64] for k, a in (per_group or {}).items()}}
                if own is not None:
                    kw.update(zip(own[0], own[1][i]), stream=self.streams[i].cuda_stream)
                lanes[lo] = (cut(berr, lo, hi), kw)
        return method, lanes

    def _sweep_lanes(self, request, n, accum, mode=None, lane_bufs=None):
        """Run a ``_lane_request`` on every lane -- every sweep of the engine goes through here.  ``accum`` ({name:
        tensor}) is accumulated over the lanes by ``_run``, unless the request came with the caller's own per-lane
        buffers ``lane_bufs``: the lanes then issue native work only (``_run``'s ``raw``).  A lane with rows of
        ``berr`` has its backward errors pointed at them, its solver checked in ``mode`` (default: the engine's), for
        this call only."""
        method, lanes = request
        mode = self.check_mode if mode is None else mode
        if mode & _native.PFR_CHECK_REFINE_ADJ and method != "hessian_sweep":
            self._seeded = True        # the lanes allocate their refinement seed vectors in this sweep
        names = tuple(accum)

        def call(sv, lo, hi, bufs, stream=None):
            vb, kw = lanes[lo]
            if vb is not None:
                sv.set_check(mode, self.check_tol, vb)
            try:
                getattr(sv, method)(**kw, **(_NO_ARGS if lane_bufs is not None else dict(zip(names, bufs))))
            finally:
                if vb is not None:
                    sv.set_check(self.check_mode, self.check_tol)
        if lane_bufs is None:
            self._run(call, n, [accum[k] for k in names])
        else:
            self._run(call, n, None, lane_bufs=lane_bufs, raw=True)

    def outputs(self, n, dtype=torch.float64, jc=False):
        """``(response, flags, berr, jc)`` of an ``n``-frequency sweep, on the device: the response (n,) of ``dtype``
        (float64: fr, complex128: H; None: none), the status flags (int32, zero), the backward errors (n, 2) (NaN:
        not checked) and, when asked, the Jacobian rows (n, n_stiff) complex (else None)."""
        dev = self.device
        return (None if dtype is None else torch.empty(n, dtype=dtype, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev),
                torch.full((n, 2), float('nan'), dtype=torch.float64, device=dev),
                torch.empty((n, self.n_stiff), dtype=torch.complex128, device=dev) if jc else None)

    def accumulators(self):
        """``(loss (1,) float64, w (n_stiff,) complex128)``, zero on the device: what a loss sweep accumulates into."""
        return (torch.zeros(1, dtype=torch.float64, device=self.device),
                torch.zeros(self.n_stiff, dtype=torch.complex128, device=self.device))

    def record(self, flags, berr, flagged=None):
        """A finished sweep's backward errors and flags become ``last_berr`` and ``last_flags`` (host; RuntimeWarning
        for the flagged frequencies, ``_check_flags``).  ``flagged``: their number where the caller has it on the
        host already -- the flags are copied only when it is not zero."""
        self.last_berr = berr
        if flags is None:
            self.last_flags = None
        elif flagged is not None and not flagged:
            self.last_flags = np.zeros(flags.numel(), np.int32)
        else:
            self.last_flags = _check_flags(flags)

    def loss_step(self, freqs, loss_type, ref, scale, axis=None):
        """One loss + gradient sweep with the step buffers reused across calls (the optimiser / bench loop:
        the host's step-to-step turnaround is GPU idle time).  Per lane, loss and the contracted partials
        accumulate into one slot of a single device buffer whose last entry receives the number of flagged
        frequencies; one fill per buffer, one device->host copy.  Returns (loss sum, w (18,) complex, flags
        device tensor, flagged count); the backward errors land in ``last_berr``.  ``axis`` (3 real numbers; None:
        the magnitude fr): the loss of the complex response along it (``Solver.sweep_complex``, a LOSS_C* id)."""
        n = freqs.numel()
        key = (n, self.n_lanes, id(self.solvers[0]))
        b = self._step_bufs.get(key)
        L, m = self.n_lanes, 2 + 2 * self.n_stiff
        if b is None:
            # the lanes' loss / w slots (float64) and the flags (int32) in one device buffer: one device->host
            # copy per step, the flagged count taken on the host (no count kernels after the sweep)
            raw = torch.empty(8 * L * m + 4 * n, dtype=torch.uint8, device=self.device)
            acc = raw[:8 * L * m].view(torch.float64)
            lanes = [[acc[l * m:l * m + 1], acc[l * m + 2:(l + 1) * m].view(self.n_stiff, 2)] for l in range(L)]
            b = (acc, lanes, raw[8 * L * m:].view(torch.int32),
                 torch.empty((n, 2), dtype=torch.float64, device=self.device), raw,
                 torch.empty(raw.numel(), dtype=torch.uint8, pin_memory=True), torch.cuda.Event())
            self._step_bufs = {key: b}            # one shape at a time (a new size replaces it)
        acc, lanes, flags, berr, raw, host, done = b
        # no fills here: every lane's sweep initialises its loss / w slots, flags and backward errors in its first
        # kernel (pfr_sweep_fresh)
        # the step's lane request, made once per (buffers, freqs, ref, loss, scale, axis): cutting the tensors and
        # putting a lane's arguments together costs host time on the step-to-step turnaround
        vkey = (key, freqs.data_ptr(), ref.data_ptr(), freqs.numel(), loss_type, scale,
                axis if axis is None else tuple(axis))
        views = self._step_views.get(vkey)
        if views is None:
            ran = [hi > lo for lo, hi in self._split(n)]
            views = (self._lane_request("sweep", n, dict(freqs=freqs, ref=ref, flags=flags), axis=axis, berr=berr,
                                        own=(("loss", "w"), lanes), loss_type=loss_type, scale=scale, fresh=True),
                     None if all(ran) else np.nonzero(ran)[0])
            self._step_views = {vkey: views}
        self._sweep_lanes(views[0], n, (), lane_bufs=lanes)
        # the result into pinned memory and the host polling for it: a blocking copy returned ~85 us after the copy
        # had finished on the GPU (the host thread woken from its sleep, gpurun_out/tl/timeline.txt) -- GPU idle
        # before the next step's first launch.  PFR_STEP_WAIT=block: the blocking copy.
        if self._spin_wait:
            host.copy_(raw, non_blocking=True)
            done.record(torch.cuda.current_stream(self.device))
            while not done.query():
                pass
            if _HT is not None:
                _HT("copy_done")
            hb = host.numpy()
        else:
            hb = raw.cpu().numpy()
        h = hb[:8 * L * m].view(np.float64).reshape(L, m)
        # summed over the lanes that swept (a lane with no frequencies ran nothing: its slot was never initialised);
        # a lane's slot: loss, (unused), then its n_stiff partials as complex pairs
        act = views[1]
        tot = h[act].sum(axis=0) if act is not None else h.sum(axis=0)
        wk = tot[2:].view(np.complex128)
        if wk.size == 18:
            w = wk.copy()
        else:
            w = np.zeros(18, dtype=np.complex128)
            w[self.kidx] = wk
        self.last_berr = berr
        return float(tot[0]), w, flags, int(np.count_nonzero(hb[8 * L * m:].view(np.int32)))

    def sweep(self, freqs, loss_type=_native.LOSS_NONE, ref=None, scale=1.0, fr=None, loss=None, w=None,
              flags=None, berr=None, axis=None):
        """``Solver.sweep`` over all lanes (fr / flags / berr (F, 2) written in place, loss / w
        accumulated).  ``axis`` (3 real numbers): ``Solver.sweep_complex`` instead, ``fr`` a complex128 tensor that
        receives the response H along the axis and ``loss_type`` one of the LOSS_C* ids."""
        n = freqs.numel()
        self._sweep_lanes(self._lane_request("sweep", n, dict(freqs=freqs, ref=ref, flags=flags), axis=axis, resp=fr,
                                             berr=berr, loss_type=loss_type, scale=scale), n, dict(loss=loss, w=w))

    def hessian_sweep(self, freqs, loss_type, ref, scale, dcoef, loss=None, w=None, h=None, flags=None):
        n = freqs.numel()
        self._sweep_lanes(self._lane_request("hessian", n, dict(freqs=freqs, ref=ref, flags=flags), loss_type=loss_type,
                                             scale=scale, dcoef=dcoef), n, dict(loss=loss, w=w, h=h))

    def jacobian_sweep(self, freqs, jc, fr=None, flags=None, berr=None, axis=None):
        """``Solver.jacobian_sweep`` over all lanes: every lane writes its own rows of ``jc`` (F, n_stiff) complex
        (and of fr / flags / berr (F, 2)); nothing is accumulated.  Sets ``last_berr`` and ``last_flags``.
        ``axis`` (3 real numbers): ``Solver.jacobian_sweep_complex``, ``fr`` a complex128 tensor for H."""
        n = freqs.numel()
        self._sweep_lanes(self._lane_request("jacobian", n, dict(freqs=freqs, jc=torch.view_as_real(jc), flags=flags),
                                             axis=axis, resp=fr, berr=berr), n, {})
        self.record(flags, berr)

    def set_inertia(self, I):
        """The inertia constants ``I = (I0, I0Corr, I2, I2Corr)`` of every later sweep: ``mass = sum_j I_j G_j``
        recombined on the host with the constructor's expression (at the problem's own constants: the same bits),
        uploaded into the lanes' mass buffer, ``mass_sum`` with it (the lanes' rhs scale follows at the next
        ``set_coefficients``).  No symbolic analysis, no new solver.  Memoised on the last ``I``."""
        I = tuple(float(v) for v in I)
        if len(I) != 4:
            raise ValueError('set_inertia takes (I0, I0Corr, I2, I2Corr)')
        if I == self.inertia:
            return
        I0, I0c, I2, I2c = I
        G = self._mass_parts()
        mass = I0 * G[0] + I0c * G[1] + I2 * G[2] + I2c * G[3]
        self.mass.copy_(torch.as_tensor(np.ascontiguousarray(mass)))
        self.mass_sum = I0 + I0c + I2 + I2c
        self.inertia = I
        for sv in self.solvers:
            sv.set_operator(torch.view_as_real(self.K), self.mass)
        self._coef_key = None          # set_rhs on every lane with the new mass_sum, at the next set_coefficients

    def _mass_parts(self):
        """G_0 .. G_3 (4, nnz) on the host: v18 + v20 + v22, v19 + v21 + v23, v24, v25 of the kept entries."""
        if self._G is None:
            v = self._mats[18:26][:, self.keep]
            self._G = np.stack([v[0] + v[2] + v[4], v[1] + v[3] + v[5], v[6], v[7]])
        return self._G

    def inertia_sweep(self, freqs, jm, jc=None, fr=None, flags=None, berr=None, axis=None):
        """``Solver.inertia_sweep`` over all lanes: the Jacobian sweep with the inertia rows ``jm`` (F, 4) complex,
        ``d fr_q / d I_j = Re jm[q, j]`` (``axis``: ``d H_q / d I_j = jm[q, j]``); ``jc`` (F, n_stiff) may be None.
        The lanes register the mass matrices (pfr_set_inertia, load weights 1) at the first call.  Sets ``last_berr``
        and ``last_flags``."""
        if self._inertia_lanes is not self.solvers:
            if self._G_dev is None:
                self._G_dev = torch.as_tensor(np.ascontiguousarray(self._mass_parts().T), device=self.device)
            for sv in self.solvers:
                sv.set_inertia(self._G_dev, np.ones(4))
            self._inertia_lanes = self.solvers
        n = freqs.numel()
        per_freq = dict(freqs=freqs, jm=torch.view_as_real(jm), jc=None if jc is None else torch.view_as_real(jc),
                        flags=flags)
        self._sweep_lanes(self._lane_request("inertia", n, per_freq, axis=axis, resp=fr, berr=berr), n, {})
        self.record(flags, berr)

    def field_sweep(self, freqs, rows=None, fr=None):
        """``Solver.field_sweep`` over all lanes: the solution's rows ``rows`` (host, caller numbering; None: every
        row) at every frequency as an (F, n_sel) complex128 device tensor -- frequency-major, so every lane writes
        its own block of rows of it, as of ``fr`` (F,), the flags and the backward errors; nothing is accumulated.
        The sweep honours the forward check and the refinement of the engine's check mode (pfr_field_sweep ignores
        the rest).  Sets ``last_berr`` (column 1 stays NaN: no adjoint) and ``last_flags``."""
        n = freqs.numel()
        if rows is not None:
            rows = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int32)
        n_sel = self._sym_args[0] if rows is None else int(rows.size)
        _, flags, berr, _ = self.outputs(n, dtype=None)
        out = torch.empty((n, n_sel), dtype=torch.complex128, device=self.device)
        # pfr_field_sweep reduces the mode itself; reduced here only so that _sweep_lanes does not count refinement
        # seed vectors (PFR_CHECK_REFINE_ADJ) that this sweep never allocates
        mode = self.check_mode & (_native.PFR_CHECK_FORWARD | _native.PFR_CHECK_REFINE)
        self._sweep_lanes(self._lane_request("field", n, dict(freqs=freqs, out=out, flags=flags), resp=fr, berr=berr,
                                             rows=rows), n, {}, mode=mode)
        self.record(flags, berr)
        return out

    def field_loss_step(self, freqs, rows, weights, loss_id, ref, scale, out=None):
        """``Solver.field_loss_sweep`` over all lanes: a loss on the solution's rows ``rows`` (host, caller numbering,
        no repeats; None: every row) with the host ``weights`` (None: all 1) against ``ref`` (F, n_sel) complex128 on
        the device -- frequency-major, so ``ref`` and the optional field ``out`` are cut into the lanes' frequency
        blocks like the field sweep's ``out``.  ``loss_id`` a LOSS_F* id (LOSS_FCOTANGENT: ``ref`` is the caller's
        dL/dx and the loss stays 0).  Returns ``(scale x the sum of the terms, w (18,) complex)`` on the host; the
        sweep honours the forward and adjoint checks and the refinement of the engine's check mode.  Sets
        ``last_berr`` and ``last_flags``."""
        n = freqs.numel()
        if rows is not None:
            rows = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int32)
        _, flags, berr, _ = self.outputs(n, dtype=None)
        loss, w = self.accumulators()
        # which bits the sweep honours is pfr_field_loss_sweep's business alone; the one bit taken out here is the
        # engine's own bookkeeping: _sweep_lanes counts refinement seed vectors (PFR_CHECK_REFINE_ADJ) as allocated
        # by any sweep that runs under that bit, and this one never allocates them
        self._sweep_lanes(self._lane_request("field_loss", n, dict(freqs=freqs, ref=ref, out=out, flags=flags),
                                             berr=berr, rows=rows, weights=weights, loss_type=loss_id, scale=scale),
                          n, dict(loss=loss, w=torch.view_as_real(w)),
                          mode=self.check_mode & ~_native.PFR_CHECK_REFINE_ADJ)
        self.record(flags, berr)
        return float(loss.item()), self.expand(w).cpu().numpy()

    def population_sweep(self, freqs, C, jac=True):
        """One sweep for a population of coefficient sets ``C`` (P, 18) complex over the same ``freqs`` (F,): a lane
        is a (member, frequency) pair in ``population_layout``'s order, every 64-lane group assembled from its
        member's operator (pfr_combine_batch, pfr_population_sweep); the engine is sized for the P Fpad lanes and they
        are split over the solver lanes as any sweep's frequencies.  Returns ``(fr (P, F), jc (P, F, n_stiff) complex
        or None without jac, flags (P, F) int32 host, berr (P, F, 2))``, the padded lanes dropped.  The selective
        adjoint refinement (PFR_CHECK_REFINE_ADJ) ranks the groups of a chunk against each other and is left out
        of the check mode here."""
        C = np.asarray(C, dtype=np.complex128)
        if C.ndim != 2 or C.shape[1] != 18:
            raise ValueError('population_sweep takes a (members, 18) coefficient array')
        P, F = C.shape[0], int(freqs.numel())
        index, member, valid = population_layout(P, F)
        L = index.size
        self.ensure(L)
        dev = self.device
        Kpop = torch.empty((P, self.keep.size), dtype=torch.complex128, device=dev)
        self.solver.combine_batch(C[:, self.kidx], torch.view_as_real(Kpop))
        beta = C @ self.e
        if self._coef_key is None:
            # the Dirichlet vector and the mass sum (the population sweep reads them, not this beta)
            for sv in self.solvers:
                sv.set_rhs(self.rhs, complex(beta[0]), self.mass_sum)
            self._pruned_stats()
        f = freqs[torch.as_tensor(index, device=dev)].contiguous()
        fr, flags, berr, jc = self.outputs(L, jc=jac)
        request = self._lane_request("population", L, dict(freqs=f, jc=None if jc is None else torch.view_as_real(jc),
                                                           flags=flags),
                                     resp=fr, berr=berr, per_group=dict(member=member), Kpop=torch.view_as_real(Kpop),
                                     beta=beta)
        self._sweep_lanes(request, L, {}, mode=self.check_mode & ~_native.PFR_CHECK_REFINE_ADJ)
        vm = torch.as_tensor(valid, device=dev)
        pick = lambda t: t[vm].reshape((P, F) + t.shape[1:])                 # noqa: E731
        self.record(pick(flags), pick(berr))
        return pick(fr), None if jc is None else pick(jc), self.last_flags, self.last_berr

    # ---- measurement (bench.py)
    def set_timing(self, on, kernels=False):
        for sv in self.solvers:
            sv.set_timing(on, kernels)

    def last_timings(self) -> np.ndarray:
        """Per-phase device ms of the last call, summed over the lanes (lanes overlap in time)."""
        return sum(sv.last_timings() for sv in self.solvers)

    def last_kernel_timings(self):
        ms, n = zip(*(sv.last_kernel_timings() for sv in self.solvers))
        return sum(ms), sum(n)


_JET_TYPES = ('isotropic', 'orthotropic', 'orthotropic_d4', 'sol', 'symm_sol')
_HT = None          # host-turnaround marks (tools/host_turnaround.py sets a callable; None in use)


def _coeffs18(transform, params: torch.Tensor) -> torch.Tensor:
    A, B, D = transform(params)
    return torch.cat([A, B, D]).to(torch.complex128)


def _sensing_axis(axis) -> np.ndarray:
    """The real sensing axis (dU, dV, dW) of the complex response as 3 float64 (default: out of plane)."""
    a = np.asarray((0.0, 0.0, 1.0) if axis is None else axis, dtype=np.float64).reshape(-1)
    if a.size != 3 or not np.isfinite(a).all() or not a.any():
        raise ValueError(f'the sensing axis needs 3 finite components, not all zero: {axis!r}')
    return a


class _SweepResponse(torch.autograd.Function):
    """The response of a frequency vector as a function of c: the magnitude fr (float64; ``axis`` None) or the complex
    H(c) = axis . (ts U, ts V, W).  Backward = one adjoint sweep with the incoming gradient as the loss cotangent:
    dL/dfr (PFR_LOSS_COTANGENT), or g = conj(grad_out) (PFR_LOSS_CCOTANGENT), torch's convention
    dL = Re(conj(grad) dH)."""

    @staticmethod
    def forward(ctx, c, engine, freqs, axis):
        cn = c.detach().cpu().numpy()
        engine.set_coefficients(cn)
        out, flags, berr, _ = engine.outputs(freqs.numel(), torch.float64 if axis is None else torch.complex128)
        engine.sweep(freqs, _native.LOSS_NONE, fr=out, flags=flags, berr=berr, axis=axis)
        engine.record(flags, berr)
        ctx.engine, ctx.freqs, ctx.cn, ctx.axis = engine, freqs, cn, axis
        return out

    @staticmethod
    def backward(ctx, grad):
        engine = ctx.engine
        engine.set_coefficients(ctx.cn)
        if ctx.axis is None:
            ref = torch.zeros(ctx.freqs.numel(), dtype=torch.complex128, device=engine.device)
            ref.real.copy_(grad.to(torch.float64))
        else:
            ref = torch.conj(grad.to(torch.complex128)).resolve_conj().contiguous()
        loss, w = engine.accumulators()
        # the cotangent sweep's solves are checked like the forward ones: flags and backward errors
        # reported, not dropped
        _, flags, berr, _ = engine.outputs(ctx.freqs.numel(), None)
        engine.sweep(ctx.freqs, _native.LOSS_COTANGENT if ctx.axis is None else _native.LOSS_CCOTANGENT,
                     ref=torch.view_as_real(ref), scale=1.0, loss=loss, w=torch.view_as_real(w), flags=flags,
                     berr=berr, axis=ctx.axis)
        engine.record(flags, berr)
        return torch.conj(engine.expand(w)).to(torch.complex128).cpu(), None, None, None


def _loss_id(func_type: str, axis=None, no_complex: str | None = None):
    """``(native loss id, sensing axis)`` of a loss name: the checked axis (default: out of plane) for the complex
    response's losses -- an error for the sweep ``no_complex`` names, which has none -- and None for the magnitude's,
    which take no axis."""
    if func_type in _native.COMPLEX_LOSS_IDS:
        if no_complex is not None:
            raise ValueError(f'the {no_complex} sweep has no complex-response losses ("{func_type}")')
        return _native.COMPLEX_LOSS_IDS[func_type], _sensing_axis(axis)
    if func_type not in _native.LOSS_IDS:
        raise ValueError(f'Function type "{func_type}" is not supported!')
    if axis is not None:
        raise ValueError(f'"{func_type}" is a loss of the magnitude fr: it takes no sensing axis')
    return _native.LOSS_IDS[func_type], None


def _loss_step(engine, freqs, ref, loss_id, n_total, axis):
    """``(loss sum, w (18,) complex)`` of the single-process step (_Engine.loss_step: reused buffers, one
    device->host copy), its flags recorded -- copied only when some are set."""
    lsum, w, flags, nflag = engine.loss_step(freqs, loss_id, torch.view_as_real(ref), 1.0 / n_total, axis)
    engine.record(flags, engine.last_berr, nflag)
    return lsum, w


class _SweepLoss(torch.autograd.Function):
    """Fused loss + gradient: one factorisation per frequency (forward + adjoint).  ``axis`` (None: the magnitude's
    losses): the complex response's losses along it."""

    @staticmethod
    def forward(ctx, c, engine, freqs, ref, loss_id, n_total, reduce_fn, axis=None):
        cn = c.detach().cpu().numpy()
        engine.set_coefficients(cn)
        if reduce_fn is None:
            lsum, w = _loss_step(engine, freqs, ref, loss_id, n_total, axis)
            ctx.save_for_backward(torch.from_numpy(w))
            return torch.tensor(lsum / n_total, dtype=torch.float64)
        loss, w = engine.accumulators()
        _, flags, berr, _ = engine.outputs(freqs.numel(), None)
        engine.sweep(freqs, loss_id, ref=torch.view_as_real(ref), scale=1.0 / n_total,
                     loss=loss, w=torch.view_as_real(w), flags=flags, berr=berr, axis=axis)
        packed = reduce_fn(torch.cat([loss.to(torch.complex128), engine.expand(w)]))
        # one device->host copy per step: loss, gradient partials and the number of flagged frequencies
        # (the flags themselves are copied only when some are set)
        host = torch.cat([packed, torch.count_nonzero(flags).to(torch.complex128).reshape(1)]).cpu()
        engine.record(flags, berr, host[-1].real != 0)
        ctx.save_for_backward(host[1:-1])
        return host[0].real / n_total

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return torch.conj(w) * g, None, None, None, None, None, None, None


class _JetSweepLoss(torch.autograd.Function):
    """params -> loss as ONE autograd node for the material types of the jet transform (_abd_jet.py): c(theta) and
    its Jacobian J from the jet pass, loss and the partials w from the fused sweep (_Engine.loss_step), and
    dL/dtheta = Re(w J) -- the product _Coeffs.backward forms from _SweepLoss.backward's conj(w) -- already in the
    forward, so that the backward is one scale.  The same values, bit for bit, as the chain
    params.to(float64).cpu() * scaling -> _Coeffs -> _SweepLoss, with three autograd nodes fewer on the host's
    step-to-step turnaround (the GPU idles from one step's result to the next step's first launch)."""

    @staticmethod
    def forward(ctx, params, material, h, scaling, engine, freqs, ref, loss_id, n_total, axis=None):
        # scaling: 1.0 or a float64 numpy array (the host arithmetic in numpy: the same IEEE products as the
        # chain's torch ones, a few us less per step)
        ctx.cast = params.dtype != torch.float64 or params.device.type != "cpu"
        p = (params.detach().to(torch.float64).cpu() if ctx.cast else params.detach()).numpy() * scaling
        c, J = _cached_abd(material, h, p)
        engine.set_coefficients(c)
        lsum, w = _loss_step(engine, freqs, ref, loss_id, n_total, axis)
        # dL/dparams for an incoming gradient of 1 (the chain's values for it, bit for bit: Re(w J) * scaling)
        ctx.gt = torch.from_numpy(np.real(w @ J) * scaling)
        ctx.dtype, ctx.device = params.dtype, params.device
        return torch.scalar_tensor(lsum / n_total, dtype=torch.float64)

    @staticmethod
    def backward(ctx, g):
        grad = ctx.gt * g
        return (grad.to(dtype=ctx.dtype, device=ctx.device) if ctx.cast else grad), None, None, None, None, None, \
            None, None, None, None


def field_selection(dofs, n: int, what: str = 'the field loss'):
    """The row selection of a field loss as host int32 (None: every row), checked: integer indices inside ``[0, n)``,
    no row twice (the adjoint seed is a scatter; ``solveForwardField`` allows repeats, a loss does not)."""
    if dofs is None:
        return None
    rows = np.asarray(dofs).reshape(-1)
    if rows.size == 0 or not np.issubdtype(rows.dtype, np.integer):
        raise ValueError(f'{what}: `dofs` is a non-empty list of integer row indices')
    if rows.min() < 0 or rows.max() >= n:
        raise ValueError(f'{what}: `dofs` outside [0, {n})')
    if np.unique(rows).size != rows.size:
        raise ValueError(f'{what}: `dofs` holds a row twice')
    return np.ascontiguousarray(rows, dtype=np.int32)


def field_reference(reference_field, n_freqs: int, n_sel: int, weights=None, what: str = 'the field loss'):
    """``(reference (F, n_sel) complex128, weights (n_sel,) float64 or None)`` of a field loss, checked on the host
    before anything reaches the device: the shape, finite values, weights finite, ``>= 0`` and not all zero, and a
    non-zero weighted norm ``sum_j v_j |r_j|^2`` at every frequency (FIELD_RMSE and FIELD_MAC divide by it)."""
    ref = np.asarray(reference_field)
    if ref.shape != (n_freqs, n_sel):
        raise ValueError(f'{what}: the reference field has shape {ref.shape}, not (frequencies, selected rows) = '
                         f'({n_freqs}, {n_sel})')
    ref = np.ascontiguousarray(ref, dtype=np.complex128)
    if not np.isfinite(ref).all():
        raise ValueError(f'{what}: the reference field holds values that are not finite')
    v = None
    if weights is not None:
        v = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        if v.size != n_sel:
            raise ValueError(f'{what}: {v.size} weights for {n_sel} selected rows')
        if not np.isfinite(v).all() or (v < 0).any():
            raise ValueError(f'{what}: the weights are finite and not negative')
        if not v.any():
            raise ValueError(f'{what}: every weight is zero')
    r2 = (np.abs(ref) ** 2 * (1.0 if v is None else v)).sum(axis=1)
    if not (r2 > 0).all():
        q = int(np.argmin(r2 > 0))
        raise ValueError(f'{what}: the weighted norm of the reference field is zero at frequency {q}')
    return ref, v


class _FieldSweepLoss(torch.autograd.Function):
    """c -> the mean over the frequencies of a field loss term, one fused sweep (``_Engine.field_loss_step``): the
    full forward solve, the loss and its seed on the device, the adjoint over every front and the contraction."""

    @staticmethod
    def forward(ctx, c, engine, freqs, ref, rows, weights, loss_id):
        cn = c.detach().cpu().numpy()
        engine.set_coefficients(cn)
        lsum, w = engine.field_loss_step(freqs, rows, weights, loss_id, ref, 1.0 / freqs.numel())
        ctx.save_for_backward(torch.from_numpy(w))
        return torch.tensor(lsum, dtype=torch.float64)

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return torch.conj(w) * g, None, None, None, None, None, None


class _FieldResponse(torch.autograd.Function):
    """c -> the field (F, n_sel) complex128 on the device (``_Engine.field_sweep``).  Backward = one field-loss sweep
    with the incoming gradient as the cotangent, g = conj(grad_out) (PFR_LOSS_FCOTANGENT), torch's convention
    dL = Re(conj(grad) dx) as in ``_SweepResponse``."""

    @staticmethod
    def forward(ctx, c, engine, freqs, rows):
        cn = c.detach().cpu().numpy()
        engine.set_coefficients(cn)
        ctx.engine, ctx.freqs, ctx.cn, ctx.rows = engine, freqs, cn, rows
        return engine.field_sweep(freqs, rows)

    @staticmethod
    def backward(ctx, grad):
        engine = ctx.engine
        engine.set_coefficients(ctx.cn)
        g = torch.conj(grad.to(torch.complex128)).resolve_conj().contiguous()
        _, w = engine.field_loss_step(ctx.freqs, ctx.rows, None, _native.LOSS_FCOTANGENT, g, 1.0)
        return torch.conj(torch.from_numpy(w)).resolve_conj(), None, None, None


EXTRA_NAMES = ('rho', 'h', 'acc_mass')


def inertia_constants(rho, h, acc, acc_mass=None):
    """``(I (4,), dI (4, 3))`` (host, numpy): the inertia constants ``(I0, I0Corr, I2, I2Corr)`` of a plate of density
    ``rho`` and thickness ``h`` under the accelerometer ``acc`` (its mass ``acc_mass``, default ``acc.mass``) -- the
    lines of ``Problem._build_system``, the same bits at the problem's own values -- and their derivatives with
    respect to ``EXTRA_NAMES`` = (rho, h, acc_mass), closed form."""
    rho, h, m = float(rho), float(h), float(acc.mass if acc_mass is None else acc_mass)
    area_h = 1.0 / (np.pi * acc.radius ** 2) / acc.height        # d rho_corr / d acc_mass
    rho_corr = m / (np.pi * acc.radius ** 2) / acc.height
    top = h / 2 + acc.height
    I = np.array([h * rho, acc.height * rho_corr, rho * h ** 3 / 12, rho_corr / 3 * (top ** 3 - h ** 3 / 8)])
    dI = np.array([[h, rho, 0.0],
                   [0.0, 0.0, acc.height * area_h],
                   [h ** 3 / 12, rho * h ** 2 / 4, 0.0],
                   [0.0, rho_corr / 3 * (1.5 * top ** 2 - 0.375 * h ** 2), area_h / 3 * (top ** 3 - h ** 3 / 8)]])
    return I, dI


def thickness_scaling(h, h0):
    """(18,) ``(h / h0) ** (1, 2, 3)`` on the A, B, D blocks of six: ``c(h) = c(h0) * thickness_scaling(h, h0)``, exact
    for every laminate map here (A ~ h, B ~ h^2, D ~ h^3: the ply coordinates are ``linspace(-h / 2, h / 2)``); so
    ``d c_k / d h = (1, 2, 3) / h * c_k``."""
    return np.repeat((h / h0) ** np.array([1.0, 2.0, 3.0]), 6)


def check_extra(extra):
    """The names of the extended parameters as a tuple, each of ``EXTRA_NAMES`` at most once."""
    extra = (extra,) if isinstance(extra, str) else tuple(extra)
    if not extra or any(e not in EXTRA_NAMES for e in extra) or len(set(extra)) != len(extra):
        raise ValueError(f'`extra` is a tuple of distinct names from {EXTRA_NAMES}, not {extra}')
    return extra


def loss_and_gradient(r, Jr, const, n_freqs: int):
    """``(loss, grad)`` of a least-squares loss from its residual: ``(r @ r + const) / F`` and ``2 Jr^T r / F``
    (``Jr`` None: no gradient)."""
    return (float(r @ r) + const) / n_freqs, None if Jr is None else 2.0 * (Jr.T @ r) / n_freqs


class _ResidualLoss(torch.autograd.Function):
    """A loss whose value and gradient come from one residual evaluation on the host (``res(params) -> (r, Jr,
    const)``): one sweep per evaluation, for the gradient optimisers."""

    @staticmethod
    def forward(ctx, params, res, n_freqs):
        r, Jr, const = res(params.detach().cpu().numpy())
        loss, grad = loss_and_gradient(r, Jr, const, n_freqs)
        ctx.grad = torch.as_tensor(grad, dtype=params.dtype)
        return torch.tensor(loss, dtype=torch.float64)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.grad.to(g.device), None, None


def residual_terms(fr, reference_fr, func_type: str):
    """The four losses as least squares (host, numpy): ``(r, dr/dfr, const)`` with
    ``loss = (r @ r + const) / F`` and ``d loss / d fr = 2 r dr/dfr / F``.

        MSE          r = fr - Re ref              const = sum Im(ref)^2
        RMSE         r = (fr - Re ref) / |ref|    const = sum (Im ref / |ref|)^2
        MSE_AFC      r = fr - |ref|               const = 0
        MSE_LOG_AFC  r = log fr - log |ref|       const = 0"""
    fr = np.asarray(fr, dtype=np.float64)
    ref = np.asarray(reference_fr, dtype=np.complex128)
    rabs = np.abs(ref)
    one = np.ones_like(fr)
    if func_type == 'MSE':
        return fr - ref.real, one, float(np.sum(ref.imag ** 2))
    if func_type == 'RMSE':
        return (fr - ref.real) / rabs, one / rabs, float(np.sum((ref.imag / rabs) ** 2))
    if func_type == 'MSE_AFC':
        return fr - rabs, one, 0.0
    if func_type == 'MSE_LOG_AFC':
        return np.log(fr) - np.log(rabs), one / fr, 0.0
    raise ValueError(f'Function type "{func_type}" is not supported!')


def complex_residual_terms(H, reference_fr, func_type: str):
    """The complex response's losses as least squares (host, numpy): ``(r (2F,), dz/dH (F,), const)`` with
    ``r = [Re z; Im z]``, ``loss = (r @ r + const) / F`` and z holomorphic in H, so that
    ``Jr = [Re(dz/dH dH); Im(dz/dH dH)]`` for the complex rows dH of ``getTFJacobianFunction``.

        MSE_COMPLEX      z = H - ref              const = 0
        RMSE_COMPLEX     z = (H - ref) / |ref|    const = 0
        MSE_LOG_COMPLEX  z = log(H / ref)         const = 0    (principal branch)"""
    H = np.asarray(H, dtype=np.complex128)
    ref = np.asarray(reference_fr, dtype=np.complex128)
    if func_type == 'MSE_COMPLEX':
        z, dz = H - ref, np.ones_like(H)
    elif func_type == 'RMSE_COMPLEX':
        rabs = np.abs(ref)
        z, dz = (H - ref) / rabs, 1.0 / rabs + 0j * H
    elif func_type == 'MSE_LOG_COMPLEX':
        z, dz = np.log(H / ref), 1.0 / H
    else:
        raise ValueError(f'Function type "{func_type}" is not supported!')
    return np.concatenate([z.real, z.imag]), dz, 0.0


def covariance_from_residual(r, Jr, const=0.0, rcond=1e-12):
    """``(cov, std)`` of the least-squares estimate: ``cov = sigma^2 (Jr^T Jr)^+`` with
    ``sigma^2 = (r @ r + const) / (F - p)``, the pseudo-inverse from the eigen-decomposition of the
    column-scaled ``Jr^T Jr`` (unit diagonal: the parameters' units drop out of the singularity test).  Eigenvalues
    below ``rcond`` times the largest are left out, with a warning: those parameter combinations are not determined
    by the data."""
    r, Jr = np.asarray(r, dtype=np.float64), np.asarray(Jr, dtype=np.float64)
    F, p = Jr.shape
    if F <= p:
        raise ValueError(f'the covariance needs more residuals than parameters ({F} <= {p})')
    N = Jr.T @ Jr
    d = np.sqrt(np.diag(N))
    d = np.where(d > 0, d, 1.0)
    lam, V = np.linalg.eigh(N / np.outer(d, d))
    keep = lam > rcond * max(float(lam[-1]), 0.0)
    if not keep.all():
        warnings.warn(f"Jr^T Jr is numerically singular ({int(np.count_nonzero(~keep))} of {p} eigenvalues below "
                      f"{rcond:g} of the largest): the covariance is its pseudo-inverse's", RuntimeWarning)
    Vk = V[:, keep] / d[:, None]
    cov = (float(r @ r) + float(const)) / (F - p) * (Vk / lam[keep]) @ Vk.T
    cov = 0.5 * (cov + cov.T)
    return cov, np.sqrt(np.diag(cov))


def population_layout(n_members: int, n_freqs: int):
    """Lane layout of a population sweep (host, numpy): member ``p`` owns the ``Fpad = 64 ceil(F / 64)`` lanes from
    ``p * Fpad``, its frequencies first and the rest repeating its last one.  Returns ``(index (P Fpad,) of each
    lane's frequency, member (P Fpad / 64,) int32 of each 64-lane group, valid (P Fpad,) bool: not a padded lane)``."""
    P, F = int(n_members), int(n_freqs)
    if P <= 0 or F <= 0:
        raise ValueError('a population sweep needs at least one member and one frequency')
    fpad = (F + 63) // 64 * 64
    lane = np.arange(fpad)
    index = np.tile(np.minimum(lane, F - 1), P)
    member = np.repeat(np.arange(P, dtype=np.int32), fpad // 64)
    valid = np.tile(lane < F, P)
    return index, member, valid


def population_loss_grad(fr, jc, dc, reference_fr, func_type: str):
    """Losses ``(P,)`` and gradients ``(P, n_par)`` (None without ``jc``) of a population from its sweep's results
    (host, numpy): ``fr`` (P, F), the Jacobian sweep's rows ``jc`` (P, F, K) over the K contracted matrices and each
    member's ``dc`` (P, K, n_par) = d c_k / d params.  Per member ``loss = (r @ r + const) / F`` and ``grad = 2 Jr^T r
    / F`` with ``Jr = dr/dfr * Re(jc @ dc)`` (``residual_terms``, ``getFRJacobianFunction``)."""
    fr = np.asarray(fr, dtype=np.float64)
    P, F = fr.shape
    loss = np.empty(P)
    grad = None if jc is None else np.empty((P, np.asarray(dc).shape[2]))
    for p in range(P):
        r, drdfr, const = residual_terms(fr[p], reference_fr, func_type)
        Jr = None if jc is None else drdfr[:, None] * np.real(np.asarray(jc[p]) @ np.asarray(dc[p]))
        loss[p], g = loss_and_gradient(r, Jr, const, F)
        if jc is not None:
            grad[p] = g
    return loss, grad


def _check_flags(flags):
    """Warn about frequencies whose solves were flagged (one device->host copy of F int32)."""
    f = flags.cpu().numpy()
    if not f.any():
        return f
    msgs = []
    for bit, what in ((_native.PFR_FLAG_BAD_PIVOT, "hit a zero/non-finite static pivot"),
                      (_native.PFR_FLAG_BACKWARD_ERROR, "have a forward solution whose backward error exceeds "
                                                        "the check tolerance"),
                      (_native.PFR_FLAG_BACKWARD_ERROR_ADJ, "have an adjoint solution whose backward error exceeds "
                                                            "the check tolerance")):
        n = int(np.count_nonzero(f & bit))
        if n:
            msgs.append(f"{n} frequencies {what}")
    warnings.warn("; ".join(msgs) + " -- their results are not reliable (Problem.solveForwardChecked reports "
                  "the backward errors; PFR_CHECK=15 adds a refinement step)", RuntimeWarning)
    return f


class Problem:
    """Geometry + known parameters; builds the FE system once, exposes differentiable FR/loss."""

    def __init__(self, geometry: Geometry = None, material: Material = None, accel: Accelerometer = None,
                 ref_fr: tuple = None, *, cpu: int | None = 0, spath: str | os.PathLike = None,
                 device=None, max_batch: int | None = None):
        if (geometry, accel, material, spath) == (None,) * 4:                       # Problem.py:86-87
            raise ValueError('Cannot create a Problem object without arguments.')
        self.n_cpu = cpu
        self.geometry, self.material, self.accelerometer = geometry, material, accel
        if spath is None:
            if None in (geometry, accel, material):
                raise ValueError('Cannot create a Problem object without `spath` argument if any of '
                                 '`geometry`, `accel`, `material` arguments is `None`.')
        else:
            self._load_setup(spath, geometry, material, accel)
        if self.material.has_params:
            self.parameters = self.material.get_parameters()
        else:
            warnings.warn('Some elastic moduli of a material were not provided, solving forward problem as '
                          'standalone will not be possible.', RuntimeWarning)
        if ref_fr is not None:
            self.reference_fr = ref_fr
        self.e = self.geometry.height / 2.0
        self.rho = self.material.density
        self._device = device
        self._max_batch = max_batch
        self._engine = None
        self._fr_function = None
        self._build_system()

    # ------------------------------------------------------------------ setup
    def _load_setup(self, spath, geometry, material, accel):
        """``setup.json`` folder semantics of Problem.py:102-214."""
        if not isinstance(spath, (str, os.PathLike)):
            raise TypeError(f'Argument `spath` should have one of the following types: str | os.PathLike, '
                            f'not {type(spath)}.')
        if not os.path.isabs(spath):
            spath = os.path.join(_PKG_DIR, 'setups', spath)
        if not os.path.exists(spath):
            raise ValueError(f'Path of the setup {spath} does not exist.')
        if not os.path.isdir(spath):
            raise ValueError(f'Selected path {spath} is not a directory.')
        fpath = os.path.join(spath, 'setup.json')
        if not os.path.exists(fpath):
            raise FileNotFoundError(f'`setup.json` file was not found in setup directory {spath}.')
        with open(fpath) as f:
            sp = json.load(f)
        if 'accelerometer' in sp:
            v = sp['accelerometer']
            if isinstance(v, str):
                self.accelerometer = Accelerometer(v)
            elif isinstance(v, dict):
                self.accelerometer = Accelerometer(AccelerometerParams(**v))
            else:
                raise TypeError(f'In file {fpath} key `accelerometer` should have a value with type `str` or `dict`.')
        if 'material' in sp:
            v = sp['material']
            if not isinstance(v, (str, dict)):
                raise TypeError(f'In file {fpath} key `material` should have a value with type `str` or `dict`.')
            self.material = get_material(v)
        if material is not None:
            self.material = material
        if accel is not None:
            self.accelerometer = accel
        if geometry is not None:
            self.geometry = geometry
        elif 'geometry' in sp:
            g = dict(sp['geometry'])
            if 'template' not in g:
                raise ValueError(f'Cannot create Geometry object, file {fpath} should contain `template` inside '
                                 '`geometry` (FreeFEM `edp` geometries need FreeFem++, not available).')
            templ = g.pop('template')
            ny = g.pop('ny', 6)
            self.geometry = Geometry(templ, accelerometer=self.accelerometer, params=GeometryParams(**g), ny=ny)
        freq_file = os.path.join(spath, 'freqs.npy')
        if os.path.exists(freq_file):
            freqs = np.load(freq_file)
            amp = np.load(os.path.join(spath, 'amp.npy'))
            ph = os.path.join(spath, 'phase.npy')
            phase = np.load(ph) if os.path.exists(ph) else np.zeros_like(amp)
            self.reference_fr = (freqs, amp * np.exp(1j * phase))
        if None in (self.accelerometer, self.geometry, self.material):
            raise RuntimeError('One of the `geometry`, `accelerometer`, `materials` attributes was not provided '
                               'in setup.json nor as an argument.')

    def _build_system(self):
        """FE matrices + union pattern + inertia constants (Problem.py:310-374)."""
        out = load_matrices_unsymm(self.geometry.build_varfs())
        mats = out[0]
        self.mat_size = mats[0].shape[0]
        up = union_pattern(mats)
        self.sparsity = up.nnz / self.mat_size ** 2
        self.rows, self.cols = up.rows, up.cols
        self.colptr, self.rowind = up.colptr, up.rowind
        self.mats = up.values                                   # (26, nnz), CSC order
        self.present = np.zeros_like(up.values, dtype=bool)
        n = self.mat_size
        keys = up.rows.astype(np.int64) + n * up.cols.astype(np.int64)
        for k, m in enumerate(mats):
            c = m.tocoo()
            self.present[k, np.searchsorted(keys, c.row.astype(np.int64) + n * c.col.astype(np.int64))] = True
        (self.vec, self.interp_mat, self.interp_mat_Lh, self.Lh_size, self.Mh_size, self.mesh,
         self.interp_mat_Wx, self.interp_mat_Wy) = out[1:]
        acc = self.accelerometer
        rho_corr = acc.mass / (np.pi * acc.radius ** 2) / acc.height if acc is not None else 0.0
        h = self.geometry.height
        self.I0 = h * self.rho                                                  # Problem.py:367-374
        self.I0Corr = acc.height * rho_corr
        self.I2 = self.rho * h ** 3 / 12
        self.I2Corr = rho_corr / 3 * ((h / 2 + acc.height) ** 3 - h ** 3 / 8)

    def averaging_vectors(self):
        """aU, aV, aW with U = aU . x etc.: ``mean(I @ x) = (1^T I / P) @ x`` (Problem.py:454-462)."""
        L, n = self.Lh_size, self.mat_size
        k = self.accelerometer.effective_height * self.accelerometer.height
        P = self.interp_mat_Lh.shape[0]
        aU, aV, aW = np.zeros(n), np.zeros(n), np.zeros(n)
        aU[:L] = self.interp_mat_Lh.sum(0) / P
        aU[2 * L:] = -k * self.interp_mat_Wx.sum(0) / P
        aV[L:2 * L] = self.interp_mat_Lh.sum(0) / P
        aV[2 * L:] = -k * self.interp_mat_Wy.sum(0) / P
        aW[2 * L:] = self.interp_mat.sum(0) / P
        return aU, aV, aW

    # ------------------------------------------------------------------ engine
    @property
    def device(self):
        if self._device is None:
            self._device = _default_device()
        return torch.device(self._device)

    def engine(self, n_freqs: int | None = None) -> _Engine:
        """The device engine, sized -- and re-sized when a sweep needs more -- for ``n_freqs``
        (``None``: as it is, or for 1024 frequencies when it is first built)."""
        if self._engine is None:
            dev = self.device
            if dev.type != 'cuda':
                raise _native.NativeError('the plate solver needs a ROCm device (no CPU fallback)')
            self._engine = _Engine(self, dev, 1024 if n_freqs is None else n_freqs, self._max_batch)
        elif n_freqs is not None:
            self._engine.ensure(n_freqs)
        return self._engine

    def _transform(self):
        return self.material.get_ABD_transform(self.geometry.height)

    def _coeffs(self, transform, p: torch.Tensor) -> torch.Tensor:
        """c(theta) (18 complex) differentiable in theta: the jet transform (value and Jacobian in one numpy
        pass, backward one product: _abd_jet.py) for the material types of Material.py, torch autograd
        through ``transform`` otherwise."""
        if self.material.atype in _JET_TYPES:
            return _jet_coeffs18(self.material, self.geometry.height, p)
        return _coeffs18(transform, p)

    def _freqs(self, freqs) -> torch.Tensor:
        return torch.as_tensor(np.asarray(freqs, dtype=np.float64) if not isinstance(freqs, torch.Tensor)
                               else freqs, dtype=torch.float64, device=self.device).contiguous()

    def _response(self, transform, freqs, params, axis) -> torch.Tensor:
        """The response at ``freqs`` on the device, differentiable in ``params``: fr, or H along ``axis``."""
        f = self._freqs(freqs)
        p = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, dtype=np.float64))
        c = self._coeffs(transform, p.to(torch.float64).cpu())
        return _SweepResponse.apply(c, self.engine(f.numel()), f, axis)

    # ------------------------------------------------------------------ API
    def getFRFunction(self) -> Callable:
        """``fr(freqs, params) -> (F,) float64 tensor`` on the device, differentiable in params
        (``Problem.py:377-518``).  Cached per instance while the caller holds it (the reference's ``functools.cache`` on the
        method would keep every Problem -- and its device workspaces -- alive for the process)."""
        fn = self._fr_function() if self._fr_function is not None else None
        if fn is not None:
            return fn
        transform = self._transform()

        def fr_function(freqs, params):
            return self._response(transform, freqs, params, None)

        self._fr_function = weakref.ref(fr_function)    # no Problem <-> closure reference cycle
        return fr_function

    getAFCFunction = getFRFunction

    def getTFFunction(self, axis=(0, 0, 1)) -> Callable:
        """``tf(freqs, params) -> (F,) complex128 tensor`` on the device, differentiable in params: the complex
        response ``H = dU ts U + dV ts V + dW W`` along the real sensing ``axis`` (dU, dV, dW) -- (0, 0, 1) the
        out-of-plane transfer function, (cos phi, sin phi, 1) a z-axis accelerometer with its transverse sensitivity
        along phi; ``|H|`` along e1, e2, e3 squared and summed is ``getFRFunction``'s fr squared.  H is the number the
        solver's x gives, not conjugated: a reference recorded in the other time convention must be conjugated by the
        caller.  The reference computes these phases and drops them (``Problem.py`` ``_solve``)."""
        transform = self._transform()
        ax = _sensing_axis(axis)

        def tf_function(freqs, params):
            return self._response(transform, freqs, params, ax)

        return tf_function

    def solveForwardComplex(self, freqs, params=None, axis=(0, 0, 1)) -> np.ndarray:
        """The complex response along ``axis`` at ``freqs`` [Hz] (numpy complex128; ``getTFFunction``)."""
        if params is None:
            params = self.parameters
        with torch.no_grad():
            return self.getTFFunction(axis)(freqs, params).cpu().numpy()

    def solveForward(self, freqs, params=None, *, distributed: bool = False) -> np.ndarray:
        """Frequency response at ``freqs`` [Hz] (``Problem.py:611-639``).

        With ``distributed=True`` and an initialised ``torch.distributed`` group every rank sweeps
        its contiguous block of ``freqs`` and one all-gather assembles the whole response on every
        rank."""
        if params is None:
            params = self.parameters
        if distributed:
            from .distributed import all_gather_cat, shard_range
            f = np.asarray(freqs, dtype=np.float64)
            lo, hi = shard_range(f.size)
            with torch.no_grad():
                part = self.getFRFunction()(f[lo:hi], params) if hi > lo else \
                    torch.zeros(0, dtype=torch.float64, device=self.device)
                return all_gather_cat(part, f.size).cpu().numpy()
        with torch.no_grad():
            return self.getFRFunction()(freqs, params).cpu().numpy()

    solve_forward = solveForward

    def solveForwardChecked(self, freqs, params=None, *, refine: bool = False, correct: bool | None = None):
        """``(fr, berr, flags)``: the forward sweep with the componentwise backward error of every
        frequency's solve (``max_i |b - A x|_i / (|A||x| + |b|)_i``, the measure UMFPACK's
        refinement monitors) and its status flags (PFR_FLAG_*); ``refine=True`` adds one step of
        iterative refinement on the same factors first (as the reference's UMFPACK solves do by
        default, ``InnerState.h:246-247`` with a NULL Control); ``correct`` turns the functional
        correction on / off (None: the engine's setting, on by default)."""
        if params is None:
            params = self.parameters
        f = self._freqs(freqs)
        p = torch.as_tensor(np.asarray(params, dtype=np.float64))
        c = _coeffs18(self._transform(), p).detach().numpy()
        eng = self.engine(f.numel())
        eng.set_coefficients(c)
        fr, flags, berr, _ = eng.outputs(f.numel())
        mode = eng.check_mode
        m = mode | _native.PFR_CHECK_FORWARD | (_native.PFR_CHECK_REFINE if refine else 0)
        if correct is not None:
            m = (m | _native.PFR_CHECK_CORRECT) if correct else (m & ~_native.PFR_CHECK_CORRECT)
        eng.set_check(m)
        try:
            eng.sweep(f, _native.LOSS_NONE, fr=fr, flags=flags, berr=berr)
        finally:
            eng.set_check(mode)
        return fr.cpu().numpy(), berr[:, 0].cpu().numpy(), flags.cpu().numpy()

    # ------------------------------------------------------------------ the field
    def vertex_rows(self) -> np.ndarray:
        """Rows of the system ``[u (Lh); v (Lh); w (Mh)]`` that hold u, v and w at the mesh vertices, ``(3, V)``
        int64 (host only).  For the geometries meshed by ``fem/``: P1 lives on the vertices and ``fem/varf.py``
        numbers the Morley vertex values before the edge normal derivatives, so vertex ``i`` is rows ``i``,
        ``Lh + i`` and ``2 Lh + i``.  A geometry read from FreeFEM output keeps FreeFEM's numbering of the degrees
        of freedom, which is not recorded in that output."""
        if getattr(self.geometry, "_ff", None) is not None:
            raise NotImplementedError('vertex_rows: a geometry read by Geometry.from_freefem_output carries '
                                      "FreeFEM's numbering of the degrees of freedom, which its output does not give.")
        V, L = int(self.mesh.n_vertices), int(self.Lh_size)
        if L != V or self.Mh_size < V:
            raise RuntimeError(f'vertex_rows: Lh has {L} and Mh {self.Mh_size} degrees of freedom on {V} vertices')
        i = np.arange(V, dtype=np.int64)
        return np.stack([i, L + i, 2 * L + i])

    def _field_fits(self, eng: _Engine, n_freqs: int, n_sel: int, loss_sums: int = 0):
        """ValueError when the (F, n_sel) complex field (with its fr, flags and backward errors) would not fit the
        HBM left free beside the engine's workspaces -- the share of the free memory ``_Engine._shape_for`` lets
        the chunk buffers take (85 %).  ``loss_sums`` (a field loss: 1, 2 or 4 sums per tile and frequency): the
        lanes' partial-sum buffers of pfr_field_loss_sweep, allocated on its first call, are counted too."""
        need = n_freqs * (16 * n_sel + 8 + 4 + 16)
        if loss_sums:
            tiles = -(-n_sel // _native.field_tile_rows())
            need += eng.n_lanes * 8 * (tiles * loss_sums + 3) * int(eng.solver.max_batch)
        free, _ = torch.cuda.mem_get_info(eng.device)
        if need > 0.85 * free:
            raise ValueError(f'solveForwardField: the field of {n_freqs} frequencies x {n_sel} rows takes {need:,} '
                             f'bytes on the device, and {int(free):,} bytes are free beside the solver workspaces; '
                             'sweep the band in parts or select fewer rows (dofs)')

    def solveForwardField(self, freqs, params=None, dofs=None, *, return_fr: bool = False):
        """The solution of ``(K - omega^2 M) x = b`` itself at ``freqs`` [Hz]: a complex ``(F, n_sel)`` numpy array
        in the caller's numbering, ``dofs`` (rows of the system ``[u (Lh); v (Lh); w (Mh)]``, repeats and any order
        allowed; None: every row) selecting its columns -- the operating deflection shapes over a band
        (pfr_field_sweep: one forward sweep, the rows gathered on the device).  ``return_fr``: ``(field, fr)``, fr as
        ``solveForward`` gives it without the functional correction.  Dirichlet rows carry their boundary values.
        The reference solves one frequency per call for its mode picture (``Problem.py:521-608``)."""
        if params is None:
            params = self.parameters
        n = self.mat_size
        rows = None
        if dofs is not None:
            rows = np.asarray(dofs).reshape(-1)
            if rows.size == 0 or not np.issubdtype(rows.dtype, np.integer):
                raise ValueError('solveForwardField: `dofs` is a non-empty list of integer row indices')
            if rows.min() < 0 or rows.max() >= n:
                raise ValueError(f'solveForwardField: `dofs` outside [0, {n})')
        nf = int(freqs.numel()) if isinstance(freqs, torch.Tensor) else int(np.asarray(freqs).size)
        if nf == 0:
            raise ValueError('solveForwardField: no frequencies')
        n_sel = n if rows is None else int(rows.size)
        eng = self.engine(nf)              # sized first: the field has to fit beside the workspaces as they now are
        self._field_fits(eng, nf, n_sel)   # refused before the field is allocated or anything is enqueued
        f = self._freqs(freqs).reshape(-1)
        p = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, dtype=np.float64))
        with torch.no_grad():              # the coefficients as solveForward forms them
            c = self._coeffs(self._transform(), p.to(torch.float64).cpu())
        eng.set_coefficients(c.detach().cpu().numpy())
        fr = torch.empty(f.numel(), dtype=torch.float64, device=eng.device) if return_fr else None
        x = eng.field_sweep(f, rows, fr).cpu().numpy()
        return (x, fr.cpu().numpy()) if return_fr else x

    def solveForwardShapes(self, freqs, params=None) -> dict:
        """The operating deflection shapes over a band: ``{"u", "v", "w"}`` of complex ``(F, V)`` arrays, the
        in-plane and out-of-plane displacements at the mesh vertices (``vertex_rows``) at every frequency."""
        vr = self.vertex_rows()
        x = self.solveForwardField(freqs, params, vr.reshape(-1))
        V = vr.shape[1]
        return {k: np.ascontiguousarray(x[:, i * V:(i + 1) * V]) for i, k in enumerate("uvw")}

    def getModePicture(self, freq, use_freefem: bool = False, params=None, *, plot: bool = True):
        """The deflection shape at ``freq`` [Hz] (``Problem.py:521-608``): returns ``(mesh, values)`` with ``values``
        = ``|w|`` at the mesh vertices, Dirichlet vertices included -- the quantity the reference shows.  ``plot``:
        drawn as the reference draws it (filled contours over the mesh, equal aspect, a horizontal colour bar) when
        matplotlib can be imported; without it the data is returned and nothing is drawn.  ``use_freefem`` (the
        reference's FreeFem++ ``plot``): FreeFem++ is not part of this build."""
        if use_freefem:
            raise NotImplementedError('getModePicture: use_freefem=True needs FreeFem++, which is not part of this build')
        w = self.solveForwardField([float(freq)], params, self.vertex_rows()[2])[0]
        values = np.abs(w)
        if plot:
            try:
                import matplotlib.pyplot as plt
            except ImportError:
                plt = None
            if plt is not None:
                xy, tri = np.asarray(self.mesh.vertices), np.asarray(self.mesh.triangles)
                cf = plt.tricontourf(xy[:, 0], xy[:, 1], tri, values, 200, cmap='coolwarm', norm='symlog',
                                     antialiased=False)
                ax = plt.gca()
                ax.set_aspect('equal')
                plt.colorbar(cf, orientation='horizontal', location='bottom', pad=0.05)
                ax.triplot(xy[:, 0], xy[:, 1], tri, color='k', alpha=.4, lw=.4)
                ax.axis('off')
        return self.mesh, values

    def getFieldLossFunction(self, frequencies, reference_field, func_type: str, dofs=None, weights=None,
                             scaling_params=None, extra=None) -> Callable:
        """``loss(params) -> 0-dim tensor`` with autograd: full-field data -- a scanning vibrometer's deflection shapes
        ``reference_field`` (F, n_sel) complex at the rows ``dofs`` (of the system ``[u (Lh); v (Lh); w (Mh)]``, no
        repeats; None: every row) -- fitted directly (pfr_field_loss_sweep).  With x the solution's selected rows, r
        the reference and the ``weights`` v (n_sel real >= 0; None: all 1), the value is the mean over the frequencies
        of ``func_type``'s term: FIELD_MSE ``sum v |x - r|^2``, FIELD_RMSE that over ``sum v |r|^2``, FIELD_MAC
        ``1 - |sum v conj(r) x|^2 / (sum v |x|^2 sum v |r|^2)`` -- one minus the modal assurance criterion, blind to
        the amplitude and phase of either shape: the form for a scan whose excitation level is not known.  x is the
        number the solver gives, not conjugated (``getTFFunction``).  The reference is validated on the host and has
        to fit the device beside the workspaces (``solveForwardField``)."""
        if extra is not None:
            raise NotImplementedError('the field-loss sweep has no inertia rows: extra is not supported here')
        if func_type not in _native.FIELD_LOSS_IDS:
            raise ValueError(f'Function type "{func_type}" is not a field loss {tuple(_native.FIELD_LOSS_IDS)}')
        loss_id = _native.FIELD_LOSS_IDS[func_type]
        frequencies = np.asarray(frequencies, dtype=np.float64).reshape(-1)
        if frequencies.size == 0:
            raise ValueError('getFieldLossFunction: no frequencies')
        rows = field_selection(dofs, self.mat_size, 'getFieldLossFunction')
        n_sel = self.mat_size if rows is None else int(rows.size)
        ref, v = field_reference(reference_field, frequencies.size, n_sel, weights, 'getFieldLossFunction')
        eng = self.engine(frequencies.size)
        self._field_fits(eng, frequencies.size, n_sel, loss_sums=_native.FIELD_LOSS_SUMS[func_type])
        f = self._freqs(frequencies)
        ref_dev = torch.as_tensor(ref, device=self.device)
        scaling = 1.0 if scaling_params is None else torch.as_tensor(np.array(scaling_params, dtype=np.float64))
        transform = self._transform()

        def loss(params):
            p = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, dtype=np.float64))
            c = self._coeffs(transform, p.to(torch.float64).cpu() * scaling)
            return _FieldSweepLoss.apply(c, self.engine(f.numel()), f, ref_dev, rows, v, loss_id)

        return loss

    def getFieldFunction(self, dofs=None) -> Callable:
        """``field(freqs, params) -> (F, n_sel) complex128 tensor`` on the device, differentiable in params: the
        solution's rows ``dofs`` (no repeats; None: every row) at every frequency.  Forward is the field sweep
        (``solveForwardField``), backward one cotangent sweep of the field loss for the whole band -- any loss on
        field data torch can express, at the cost of the field on the device."""
        rows = field_selection(dofs, self.mat_size, 'getFieldFunction')
        n_sel = self.mat_size if rows is None else int(rows.size)
        transform = self._transform()

        def field_function(freqs, params):
            f = self._freqs(freqs).reshape(-1)
            if f.numel() == 0:
                raise ValueError('getFieldFunction: no frequencies')
            eng = self.engine(f.numel())
            self._field_fits(eng, f.numel(), n_sel)
            p = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, dtype=np.float64))
            c = self._coeffs(transform, p.to(torch.float64).cpu())
            return _FieldResponse.apply(c, eng, f, rows)

        return field_function

    def getLossFunction(self, frequencies, reference_fr, func_type: str, scaling_params=None,
                        *, distributed: bool = False, axis=None, extra=None) -> Callable:
        """``loss(params) -> 0-dim tensor`` (``Problem.py:933-980``).

        ``extra`` (names from ``EXTRA_NAMES``): a function of the extended vector ``[material params, extra values]``
        (``getFRJacobianFunction``), its value and gradient ``2 Jr^T r / F`` from ONE inertia sweep per evaluation.

        ``func_type`` MSE_COMPLEX, RMSE_COMPLEX or MSE_LOG_COMPLEX: the mean over the frequencies of ``|H - ref|^2``,
        ``|H - ref|^2 / |ref|^2`` or ``|log(H / ref)|^2`` of the complex response H along ``axis`` (``getTFFunction``;
        default (0, 0, 1)) -- amplitude and phase of the measurement, where the four losses above use its amplitude.

        With ``distributed=True`` and an initialised ``torch.distributed`` group,
        every rank sweeps its contiguous block of the frequencies and one
        all-reduce combines loss and gradient partials.
        """
        if extra is not None:
            if distributed:
                raise NotImplementedError('the inertia sweep is not distributed: use extra with distributed=False')
            res = self.getResidualFunction(frequencies, reference_fr, func_type, scaling_params, axis, extra=extra)
            n_freqs = np.asarray(frequencies).shape[0]

            def loss_extra(params):
                p = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, dtype=np.float64))
                return _ResidualLoss.apply(p, res, n_freqs)

            return loss_extra
        s = self._loss_setup(frequencies, reference_fr, func_type, scaling_params, distributed, axis)
        scaling = 1.0 if scaling_params is None else torch.as_tensor(s.scaling)
        transform = self._transform()

        def loss(params):
            p = params if isinstance(params, torch.Tensor) else torch.as_tensor(np.asarray(params, dtype=np.float64))
            if s.reduce_fn is None and self.material.atype in _JET_TYPES:
                # one autograd node (host turnaround of the optimiser / bench loop)
                return _JetSweepLoss.apply(p, self.material, self.geometry.height, s.scaling, self.engine(s.n_engine),
                                           s.freqs, s.ref, s.loss_id, s.n_total, s.axis)
            c = self._coeffs(transform, p.to(torch.float64).cpu() * scaling)
            return _SweepLoss.apply(c, self.engine(s.n_engine), s.freqs, s.ref, s.loss_id, s.n_total, s.reduce_fn,
                                    s.axis)

        return loss

    def _loss_setup(self, frequencies, reference_fr, func_type, scaling_params, distributed, axis=None,
                    no_complex=None):
        """What a loss sweep is made from, checked once: the loss id and sensing axis (``_loss_id``), the parameter
        scaling (1.0 or a float64 numpy array), this rank's block of the frequencies and of the reference on the
        device (all of them unless ``distributed``: then ``distributed.shard_range``, and ``reduce_fn`` the
        all-reduce of the packed partials), the frequency count of the mean and the one the engine is sized for."""
        frequencies = np.asarray(frequencies)
        reference_fr = np.asarray(reference_fr)
        assert frequencies.shape[0] == reference_fr.shape[0]
        loss_id, axis = _loss_id(func_type, axis, no_complex)
        n_total = frequencies.shape[0]
        lo, hi, reduce_fn = 0, n_total, None
        if distributed:
            from .distributed import shard_range, all_reduce_sum
            lo, hi = shard_range(n_total)
            reduce_fn = all_reduce_sum
        return SimpleNamespace(loss_id=loss_id, axis=axis, n_total=n_total, n_engine=max(1, hi - lo),
                               reduce_fn=reduce_fn, freqs=self._freqs(frequencies[lo:hi]),
                               ref=torch.as_tensor(reference_fr[lo:hi].astype(np.complex128), device=self.device),
                               scaling=1.0 if scaling_params is None else np.array(scaling_params, dtype=np.float64))

    def getLossHessianFunction(self, frequencies, reference_fr, func_type: str, scaling_params=None,
                               *, distributed: bool = False, extra=None) -> Callable:
        """``model(params) -> (loss, grad, hessian)`` (numpy) of ``getLossFunction``'s loss.

        Replaces the reference's forward-over-reverse Hessian (``jax.jacobian(grad)``,
        ``Optimizers.py:125-136``; its mode-4 solves refactorise per direction,
        ``InnerState.h:289-305``): one GPU sweep factors each frequency once and
        reuses the factors for the tangent solves ``A dx_i = db_i - dA_i x`` and the
        second-order adjoints ``A^T dl_i = dG_i - dA_i^T l`` of every parameter
        direction; the material transform's first and second derivatives come
        from torch autograd on the host.
        """
        if extra is not None:
            raise NotImplementedError('the Hessian sweep has no inertia rows: extra is not supported here')
        s = self._loss_setup(frequencies, reference_fr, func_type, scaling_params, distributed, no_complex='Hessian')
        c_and_dc = self._coeffs_jacobian(scaling_params)       # on the jet materials the same c (to the bit) as
        c_real = c_and_dc.c_real                               # getLossFunction's jet transform

        def model(params):
            p = torch.as_tensor(np.asarray(params, dtype=np.float64)).detach()
            n = p.numel()
            c, dc = c_and_dc(p)                                                            # (18,), (18, n)
            d2 = np.stack([torch.autograd.functional.hessian(lambda x, m=m: c_real(x)[m], p).numpy()
                           for m in range(36)]).reshape(18, 2, n, n)
            d2c = d2[:, 0] + 1j * d2[:, 1]                                                 # (18, n, n)
            eng = self.engine(s.n_engine)
            eng.set_coefficients(c)
            loss, w = eng.accumulators()
            h = torch.zeros(n, eng.n_stiff, dtype=torch.complex128, device=eng.device)
            flags = torch.zeros(s.freqs.numel(), dtype=torch.int32, device=eng.device)
            eng.hessian_sweep(s.freqs, s.loss_id, torch.view_as_real(s.ref), 1.0 / s.n_total, dc[eng.kidx].T,
                              loss=loss, w=torch.view_as_real(w), h=torch.view_as_real(h), flags=flags)
            _check_flags(flags)
            packed = torch.cat([loss.to(torch.complex128), eng.expand(w), eng.expand(h).reshape(-1)])
            if s.reduce_fn is not None:
                packed = s.reduce_fn(packed)
            packed = packed.cpu().numpy()
            val = packed[0].real / s.n_total
            w_, h_ = packed[1:19], packed[19:].reshape(n, 18)
            grad = np.real(w_ @ dc)
            hess = np.real(h_ @ dc) + np.real(np.einsum('k,kij->ij', w_, d2c))
            return float(val), grad, 0.5 * (hess + hess.T)

        return model

    def getFRJacobianFunction(self, scaling_params=None, extra=None) -> Callable:
        """``fn(freqs, params) -> (fr (F,), J (F, n_params))``, float64 tensors on the device:
        ``J[q, i] = d fr_q / d params_i`` from ONE sweep (one factorisation and one adjoint solve per frequency,
        pfr_jacobian_sweep), where reverse mode through ``getFRFunction`` needs one adjoint sweep per frequency.
        ``scaling_params``: the function is of ``params * scaling_params`` and J is with respect to ``params``.

        ``extra``: a tuple of names from ``EXTRA_NAMES`` = ('rho', 'h', 'acc_mass') -- the plate's density, its
        thickness and the accelerometer's mass as parameters too.  ``params`` is then ``[material params, extra
        values]`` in physical units (``scaling_params`` spans all of it) and J gains one column per name, from the
        inertia rows of the same sweep (pfr_inertia_sweep): ``Re(jm @ dI/dname)``, for ``h`` plus ``Re(jc @ dc/dh)``
        (``inertia_constants``, ``thickness_scaling``).  Values other than the problem's own are set for the call --
        the mass matrix recombined and uploaded (``_Engine.set_inertia``), no new analysis -- and the problem's own
        put back after it: a later call without ``extra`` returns the bits it returned before."""
        return self._jacobian_function(scaling_params, None, extra)

    def extendedParameters(self, extra) -> np.ndarray:
        """``[material parameters, the problem's own values of the names in extra]``."""
        own = dict(rho=self.rho, h=self.geometry.height, acc_mass=self.accelerometer.mass)
        return np.concatenate([np.asarray(self.parameters, dtype=np.float64), [own[e] for e in check_extra(extra)]])

    def _extended(self, scaling_params, extra):
        """``fn(params) -> (c (18,), dc (18, n_params), I (4,), dI (4, n_params))`` for the extended vector: the
        coefficients at the thickness in ``params`` (the material's at the problem's thickness times
        ``thickness_scaling``) and the inertia constants, with their derivatives with respect to ``params``."""
        extra = check_extra(extra)
        c_and_dc = self._coeffs_jacobian(None)
        h0 = float(self.geometry.height)
        power = np.repeat([1.0, 2.0, 3.0], 6)

        def fn(params):
            p = np.asarray(params.detach().cpu() if isinstance(params, torch.Tensor) else params, dtype=np.float64)
            sc = np.ones(p.size) if scaling_params is None else \
                np.broadcast_to(np.asarray(scaling_params, dtype=np.float64), (p.size,))
            n_mat = p.size - len(extra)
            if n_mat <= 0:
                raise ValueError(f'the parameter vector holds the material parameters and then {extra}')
            phys = p * sc
            val = dict(rho=self.rho, h=h0, acc_mass=self.accelerometer.mass)
            val.update(zip(extra, phys[n_mat:]))
            c0, dc0 = c_and_dc(phys[:n_mat])
            hs = thickness_scaling(val['h'], h0)
            c = c0 * hs
            I, dI3 = inertia_constants(val['rho'], val['h'], self.accelerometer, val['acc_mass'])
            dc = np.zeros((18, p.size), dtype=np.complex128)
            dI = np.zeros((4, p.size))
            dc[:, :n_mat] = dc0 * hs[:, None]
            for i, name in enumerate(extra):
                dI[:, n_mat + i] = dI3[:, EXTRA_NAMES.index(name)]
                if name == 'h':
                    dc[:, n_mat + i] = power / val['h'] * c
            return c, dc * sc[None, :], I, dI * sc[None, :]

        fn.extra = extra
        return fn

    def _inertia_rows(self, f, c, I, axis, with_jc=True):
        """One inertia sweep at the coefficients ``c`` and inertia constants ``I``: ``(response, jc or None, jm)`` on
        the device; the problem's own constants are put back afterwards."""
        eng = self.engine(f.numel())
        try:
            eng.set_inertia(I)
            eng.set_coefficients(c)
            out, flags, berr, jc = eng.outputs(f.numel(), torch.float64 if axis is None else torch.complex128,
                                               jc=with_jc)
            jm = torch.empty((f.numel(), 4), dtype=torch.complex128, device=eng.device)
            eng.inertia_sweep(f, jm, jc=jc, fr=out, flags=flags, berr=berr, axis=axis)
        finally:
            eng.set_inertia(eng.own_inertia)
        return out, jc, jm

    def _jacobian_function(self, scaling_params, axis, extra=None) -> Callable:
        """``getFRJacobianFunction`` (``axis`` None) or ``getTFJacobianFunction`` along the checked ``axis``."""
        if extra is not None:
            ext = self._extended(scaling_params, extra)

            def fn_extra(freqs, params):
                f = self._freqs(freqs)
                c, dc, I, dI = ext(params)
                out, jc, jm = self._inertia_rows(f, c, I, axis)
                eng = self._engine
                n_mat = dc.shape[1] - len(ext.extra)
                dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.complex128), device=eng.device)  # noqa: E731
                # the material columns by the product the call without extra makes (the same bits at the problem's
                # own values); the extra ones from the inertia rows, for h with the coefficients' share
                J = torch.cat([jc @ dev(dc[eng.kidx][:, :n_mat]),
                               jc @ dev(dc[eng.kidx][:, n_mat:]) + jm @ dev(dI[:, n_mat:])], dim=1)
                return out, torch.real(J) if axis is None else J

            return fn_extra
        c_and_dc = self._coeffs_jacobian(scaling_params)

        def fn(freqs, params):
            f = self._freqs(freqs)
            c, dc = c_and_dc(params)
            eng = self.engine(f.numel())
            eng.set_coefficients(c)
            out, flags, berr, jc = eng.outputs(f.numel(), torch.float64 if axis is None else torch.complex128, jc=True)
            eng.jacobian_sweep(f, jc, fr=out, flags=flags, berr=berr, axis=axis)
            # expand(jc) @ dc from the contracted matrices' rows of dc (the others' partials vanish); fr's is its
            # real part, H is holomorphic in the coefficients
            J = jc @ torch.as_tensor(np.ascontiguousarray(dc[eng.kidx]), device=eng.device)
            return out, torch.real(J) if axis is None else J

        return fn

    def _coeffs_jacobian(self, scaling_params) -> Callable:
        """``fn(params) -> (c (18,), dc (18, n_params))`` complex numpy: c(params * scaling) and its derivative with
        respect to params; ``fn.c_real``: params -> c as 36 reals, for torch's functional derivatives
        (``getLossHessianFunction``'s second ones)."""
        scaling = 1.0 if scaling_params is None else torch.as_tensor(np.array(scaling_params, dtype=np.float64))
        transform = self._transform()

        def c_real(p):
            return torch.view_as_real(_coeffs18(transform, p * scaling)).reshape(-1)      # (36,)

        def fn(params):
            p = torch.as_tensor(np.asarray(params.detach().cpu() if isinstance(params, torch.Tensor) else params,
                                           dtype=np.float64)).detach()
            n = p.numel()
            if self.material.atype in _JET_TYPES:
                from ._abd_jet import abd_and_jacobian
                sc = np.broadcast_to(np.asarray(scaling, dtype=np.float64), (n,))
                c, J = abd_and_jacobian(self.material, self.geometry.height, (p * scaling).numpy())
                return c, J * sc[None, :]
            c = _coeffs18(transform, p * scaling).detach().numpy()
            jac = torch.autograd.functional.jacobian(c_real, p).numpy().reshape(18, 2, n)
            return c, jac[:, 0] + 1j * jac[:, 1]

        fn.c_real = c_real
        return fn

    def getTFJacobianFunction(self, scaling_params=None, axis=(0, 0, 1), extra=None) -> Callable:
        """``fn(freqs, params) -> (H (F,), dH (F, n_params))``, complex128 tensors on the device: the complex response
        along ``axis`` (``getTFFunction``) and ``dH[q, i] = d H_q / d params_i`` from ONE sweep
        (pfr_jacobian_sweep_complex); H is holomorphic in the coefficients, so no real part is taken.
        ``scaling_params`` and ``extra`` as in ``getFRJacobianFunction``."""
        return self._jacobian_function(scaling_params, _sensing_axis(axis), extra)

    def solveForwardJacobian(self, freqs, params=None, extra=None):
        """``(fr (F,), J (F, n_params))`` (numpy): the frequency response and its derivative with respect to the
        material parameters -- with ``extra`` (``getFRJacobianFunction``) also the named ones of density, thickness
        and accelerometer mass -- at every frequency."""
        if params is None:
            params = self.parameters if extra is None else self.extendedParameters(extra)
        fr, J = self.getFRJacobianFunction(extra=extra)(freqs, params)
        return fr.cpu().numpy(), J.cpu().numpy()

    def solveForwardSlope(self, freqs, params=None):
        """``(fr (F,), d fr / d f (F,))`` (numpy), f in Hz: the response and its slope along the frequency axis from
        one inertia sweep -- ``dA/df`` and ``db/df`` are ``(2 / f) sum_j I_j d/dI_j``, so the slope is
        ``(2 / f) Re(jm @ I)``, with no second solve and no finite difference across a resonance."""
        if params is None:
            params = self.parameters
        f = self._freqs(freqs)
        p = torch.as_tensor(np.asarray(params, dtype=np.float64))
        c = self._coeffs_jacobian(None)(p)[0]
        I = np.array(self.engine(f.numel()).own_inertia)
        fr, _, jm = self._inertia_rows(f, c, I, None, with_jc=False)
        slope = 2.0 / f.cpu().numpy() * np.real(jm.cpu().numpy() @ I)
        return fr.cpu().numpy(), slope

    def getResidualFunction(self, frequencies, reference_fr, func_type: str, scaling_params=None,
                            axis=None, extra=None) -> Callable:
        """``res(params) -> (r (F,), Jr (F, p), const)`` (numpy): ``getLossFunction``'s loss as least squares,
        ``loss = (r @ r + const) / F`` and ``grad = 2 / F * Jr.T @ r`` (``residual_terms``), for Gauss-Newton /
        Levenberg-Marquardt (``Optimizers.optimize_lm``) and ``parameterCovariance``.  The complex response's losses
        (``complex_residual_terms``) have 2 F residuals, ``r = [Re z; Im z]`` and ``Jr = [Re(dz/dH dH); Im(dz/dH dH)]``,
        with ``loss = r @ r / F`` (``optimize_lm`` divides by the residual count and so reports half of it)."""
        frequencies = np.asarray(frequencies, dtype=np.float64)
        reference_fr = np.asarray(reference_fr)
        assert frequencies.shape[0] == reference_fr.shape[0]
        _, axis = _loss_id(func_type, axis)
        fn = self._jacobian_function(scaling_params, axis, extra)
        terms = residual_terms if axis is None else complex_residual_terms
        f_dev = self._freqs(frequencies)

        def res(params):
            out, J = fn(f_dev, params)
            r, d, const = terms(out.cpu().numpy(), reference_fr, func_type)
            Jr = d[:, None] * J.cpu().numpy()          # dr/dfr dfr, or dz/dH dH
            return r, Jr if axis is None else np.concatenate([Jr.real, Jr.imag]), const

        return res

    def _population_coeffs(self, params, scaling, with_jac: bool):
        """``(C (P, 18), dC (P, 18, n_par) or None)``: c(params_p * scaling) of every member and, with ``with_jac``,
        its derivative with respect to params_p (as ``getFRJacobianFunction`` forms them)."""
        params = np.atleast_2d(np.asarray(params, dtype=np.float64))
        P, n = params.shape
        sc = np.broadcast_to(np.asarray(scaling, dtype=np.float64), (n,))
        transform = self._transform()
        C = np.empty((P, 18), dtype=np.complex128)
        dC = np.empty((P, 18, n), dtype=np.complex128) if with_jac else None
        for i in range(P):
            p = torch.as_tensor(params[i] * sc)
            if self.material.atype in _JET_TYPES:
                from ._abd_jet import abd_and_jacobian
                C[i], J = abd_and_jacobian(self.material, self.geometry.height, p.numpy())
                if with_jac:
                    dC[i] = J * sc[None, :]
            else:
                C[i] = _coeffs18(transform, p).detach().numpy()
                if with_jac:
                    jac = torch.autograd.functional.jacobian(
                        lambda x: torch.view_as_real(_coeffs18(transform, x)).reshape(-1), p).numpy().reshape(18, 2, n)
                    dC[i] = (jac[:, 0] + 1j * jac[:, 1]) * sc[None, :]
        return C, dC

    def solveForwardPopulation(self, freqs, params) -> np.ndarray:
        """Frequency responses ``(P, F)`` of the P parameter sets ``params`` (P, n_par) at ``freqs`` [Hz] from ONE
        sweep whose lanes are (member, frequency) pairs (``_Engine.population_sweep``): narrow sweeps of many
        parameter sets -- a differential-evolution generation, multi-start trial points -- fill the device that a
        single one leaves mostly idle."""
        f = self._freqs(freqs)
        C, _ = self._population_coeffs(params, 1.0, False)
        eng = self.engine(population_layout(C.shape[0], f.numel())[0].size)
        return eng.population_sweep(f, C, jac=False)[0].cpu().numpy()

    def getPopulationLossFunction(self, frequencies, reference_fr, func_type: str, scaling_params=None,
                                  with_grad: bool = False, *, distributed: bool = False, extra=None) -> Callable:
        """``fn(params (P, n_par)) -> losses (P,)`` -- with ``with_grad`` ``(losses, gradients (P, n_par))`` -- (numpy)
        of ``getLossFunction``'s loss for a whole population in one sweep.  Without ``with_grad`` the sweep is
        forward-only; with it, the per-frequency Jacobian sweep per lane, from which every member's gradient
        ``2 Jr^T r / F`` (and, if wanted, its Levenberg-Marquardt Jacobian) is a small host-side product
        (``population_loss_grad``)."""
        if distributed:
            raise NotImplementedError('the population sweep is not distributed: use distributed=False')
        if extra is not None:
            raise NotImplementedError('the population sweep has no inertia rows: extra is not supported here')
        frequencies = np.asarray(frequencies, dtype=np.float64)
        reference_fr = np.asarray(reference_fr)
        assert frequencies.shape[0] == reference_fr.shape[0]
        _loss_id(func_type, no_complex='population')
        scaling = 1.0 if scaling_params is None else np.array(scaling_params, dtype=np.float64)
        f_dev = self._freqs(frequencies)

        def fn(params):
            C, dC = self._population_coeffs(params, scaling, with_grad)
            P = C.shape[0]
            eng = self.engine(population_layout(P, f_dev.numel())[0].size)
            fr, jc, _, _ = eng.population_sweep(f_dev, C, jac=with_grad)
            loss, grad = population_loss_grad(fr.cpu().numpy(), None if jc is None else jc.cpu().numpy(),
                                              None if dC is None else dC[:, eng.kidx], reference_fr, func_type)
            return (loss, grad) if with_grad else loss

        return fn

    def parameterCovariance(self, frequencies, reference_fr, func_type: str, params=None, scaling_params=None,
                            axis=None, extra=None):
        """``(cov (p, p), std (p,))`` of the parameters identified from ``reference_fr``: the Gauss-Newton
        covariance ``sigma^2 (Jr^T Jr)^+`` with ``sigma^2 = (r @ r + const) / (F - p)`` at ``params`` (default: the
        material's; in the units of ``params``, i.e. scaled ones with ``scaling_params``).  A parameter the
        experiment does not determine shows as a large ``std``; a numerically singular ``Jr^T Jr`` warns."""
        if params is None:
            own = self.parameters if extra is None else self.extendedParameters(extra)
            params = own if scaling_params is None else own / np.asarray(scaling_params, dtype=np.float64)
        r, Jr, const = self.getResidualFunction(frequencies, reference_fr, func_type, scaling_params, axis,
                                                extra=extra)(params)
        return covariance_from_residual(r, Jr, const)

    def solveInverse(self, *args, **kwargs):
        from .inverse import solve_inverse
        return solve_inverse(self, *args, **kwargs)

    def solveInverseLocal(self, *args, **kwargs):
        return self.solveInverse(*args, **kwargs)
