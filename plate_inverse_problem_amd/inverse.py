"""``Problem.solveInverse`` (``source/jax_plate/Problem.py:641-914``).

Same arguments, optimizer names, scaling/relative-start semantics, report text
and ``.npz`` history log as the reference.  The loss is the fused GPU
forward + adjoint sweep; ``distributed=True`` shards the frequencies over the
ranks of an initialised ``torch.distributed`` group (one all-reduce per
evaluation, every rank runs the identical optimiser).  Extra optimizers:
``'lbfgs'`` (BASELINE.json C5) and ``'lm'`` / ``'levenberg_marquardt'`` (least squares over
``Problem.getResidualFunction``'s residual and per-frequency Jacobian; single process).
Full-field data: a ``FIELD_MSE`` / ``FIELD_RMSE`` / ``FIELD_MAC`` loss type with ``ref_field=(freqs, field)``,
``field_dofs`` and ``field_weights`` fits ``Problem.getFieldLossFunction`` with the gradient optimisers and the
non-vectorised ``de`` / ``shgo``.
Nuisance parameters: ``extra=('rho', 'h', 'acc_mass')`` (any of them) extends the vector to ``[material params, extra
values]`` -- ``arg0`` spans all of it -- for ``lm`` and the gradient optimisers (``Problem.getFRJacobianFunction``).
"""
from __future__ import annotations

import os
from time import gmtime, perf_counter, strftime

import numpy as np
import torch
from scipy.optimize import OptimizeResult, differential_evolution, shgo

from . import Optimizers as opt
from . import _native
from .Input import Compressor

_LOCAL = {("trust_region", "tr"): opt.optimize_trust_region, ("coord_descent", "cd"): opt.optimize_cd,
          ("coord_descent_mem", "cd_mem"): opt.optimize_cd_mem2, ("grad_descent", "gd"): opt.optimize_gd,
          ("lbfgs", "l-bfgs"): opt.optimize_lbfgs, ("levenberg_marquardt", "lm"): opt.optimize_lm}


def _a2s(s):
    return s if isinstance(s, str) else np.array2string(np.array(s), separator=', ', precision=5)


def solve_inverse(prob, arg0, loss_type: str, optimizer: str, compression=(False, 0), comp_alg: int = 1,
                  ref_fr=None, use_rel: bool = False, use_scaling: bool = False, use_constraints: bool = False,
                  report: bool = True, log: bool = True, case_name: str = '', uid: str = None,
                  extra_info: str = '', log_dir: str = None, distributed: bool = False, ref_field=None,
                  field_dofs=None, field_weights=None, extra=None, **opt_kwargs):
    field = loss_type in _native.FIELD_LOSS_IDS
    if extra is not None:
        no = {'the field-loss sweep has no inertia rows': field,
              'the trust region needs the Hessian sweep, which has no inertia rows': optimizer in ('trust_region', 'tr'),
              'the population sweep has no inertia rows': bool(opt_kwargs.get('vectorized', False)),
              'the inertia sweep is not distributed': distributed}
        for why, hit in no.items():
            if hit:
                raise NotImplementedError(f'solveInverse with extra={extra}: {why}')
    own = None if getattr(prob, 'parameters', None) is None else \
        np.asarray(prob.parameters) if extra is None else prob.extendedParameters(extra)
    if field:
        # full-field data: (frequencies, field (F, n_sel)) in place of ref_fr; the loss is Problem.getFieldLossFunction
        if ref_field is None:
            raise ValueError(f'the loss "{loss_type}" fits full-field data: pass ref_field=(freqs, field)')
        no = {'the trust region needs the Hessian of the field loss, which is not built': optimizer in ('trust_region', 'tr'),
              'Levenberg-Marquardt needs the field Jacobian, which is not built': optimizer in ('levenberg_marquardt', 'lm'),
              'the field loss has no population form': bool(opt_kwargs.get('vectorized', False)),
              'the field loss has no distributed form': distributed,
              'the compression selects frequencies from a response curve, which field data does not carry':
                  bool(compression[0]) if isinstance(compression, tuple) and len(compression) == 2 else False}
        for why, hit in no.items():
            if hit:
                raise NotImplementedError(f'solveInverse with "{loss_type}": {why}')
        ref_fr = (np.asarray(ref_field[0]), np.asarray(ref_field[1]))
    elif ref_field is not None or field_dofs is not None or field_weights is not None:
        raise ValueError(f'ref_field, field_dofs and field_weights go with a FIELD_* loss, not "{loss_type}"')
    if ref_fr is None:
        ref_fr = getattr(prob, 'reference_fr', None)
        if ref_fr is None:
            raise ValueError('Cannot solve inverse problem as `ref_fr` argument was not provided and the '
                             "Problem object doesn't have a reference_fr attribute.")
    ref_fr = [np.asarray(ref_fr[0]), np.asarray(ref_fr[1])]
    if not isinstance(compression, tuple):
        raise TypeError(f'`compression` argument should have a type `tuple`,not {type(compression)}.')
    if len(compression) != 2:
        raise ValueError(f'`compression` tuple should have 2 elements, not {len(compression)}.')
    if compression[0]:
        comp = Compressor(ref_fr[0], ref_fr[1], compression[1], comp_alg)
        ref_fr[0], ref_fr[1] = comp(compression[1])

    arg0 = np.array(arg0, dtype=np.float64)
    scaling = None
    if arg0.ndim == 1:
        if use_rel:
            if own is None:
                raise ValueError('Cannot use `arg0` as relative coefficients of correction as Problem object has '
                                 'no `parameters` attribute.')
            x0 = own * (arg0 + 1)
            if use_scaling:
                scaling, x0 = x0, arg0 + 1
        else:
            x0 = arg0
            if use_scaling:
                scaling, x0 = x0, np.ones_like(x0)
    elif arg0.ndim == 2:
        if use_scaling:
            scaling = np.max(np.abs(arg0), axis=1)
            x0 = arg0 / scaling[:, None]
        else:
            x0 = arg0
    else:
        raise ValueError('Invalid shape of `arg0` argument.')

    if distributed and optimizer in ('levenberg_marquardt', 'lm'):
        raise NotImplementedError('the Jacobian sweep is not distributed: use `lm` with distributed=False')
    if field:
        loss = prob.getFieldLossFunction(ref_fr[0], ref_fr[1], loss_type, field_dofs, field_weights, scaling)
    elif extra is not None:
        loss = prob.getLossFunction(ref_fr[0], ref_fr[1], loss_type, scaling, extra=extra)
    else:
        loss = prob.getLossFunction(ref_fr[0], ref_fr[1], loss_type, scaling, distributed=distributed)
    scale_arr = np.ones_like(x0) if scaling is None else (np.tile(scaling, (2, 1)).T if x0.ndim == 2 else scaling)

    local = next((fn for names, fn in _LOCAL.items() if optimizer in names), None)
    if local is not None:
        fn, call_x0 = local, x0
        if local is opt.optimize_trust_region and 'model' not in opt_kwargs and opt_kwargs.get('exact_hessian', True):
            # exact Hessian from one GPU sweep per model (factors reused per direction)
            opt_kwargs['model'] = prob.getLossHessianFunction(ref_fr[0], ref_fr[1], loss_type, scaling,
                                                              distributed=distributed)
        opt_kwargs.pop('exact_hessian', None)
        if local is opt.optimize_lm:
            # least squares: the residual and its per-frequency Jacobian (one sweep) in place of the loss
            loss = prob.getResidualFunction(ref_fr[0], ref_fr[1], loss_type, scaling, **({} if extra is None else {'extra': extra}))
    elif optimizer in ('de', 'shgo'):
        def np_loss(x):
            return float(loss(torch.as_tensor(np.asarray(x, dtype=np.float64))))
        vg = opt.value_and_grad(loss)
        if optimizer == 'de' and opt_kwargs.pop('vectorized', False):
            # a whole generation per call: scipy hands x (n_par, S), the population loss one sweep over S members
            if distributed:
                raise NotImplementedError('the population sweep is not distributed: use vectorized with '
                                          'distributed=False')
            pop_loss = prob.getPopulationLossFunction(ref_fr[0], ref_fr[1], loss_type, scaling)
            opt_kwargs.setdefault('updating', 'deferred')
            fn = lambda f, bounds, **kw: differential_evolution(                          # noqa: E731
                lambda x: pop_loss(np.asarray(x, dtype=np.float64).T), bounds, vectorized=True, **kw)
        elif optimizer == 'de':
            fn = lambda f, bounds, **kw: differential_evolution(np_loss, bounds, **kw)   # noqa: E731
        else:
            if use_constraints:
                raise NotImplementedError('material constraints for shgo are not provided by this build')
            o = dict(opt_kwargs.pop('options', {}))
            o['jac'] = lambda x: vg(x)[1]
            fn = lambda f, bounds, **kw: shgo(np_loss, bounds, options=o, **kw)          # noqa: E731
        call_x0 = [tuple(b) for b in x0]
    else:
        raise ValueError(f'Optimizer type `{optimizer}` is not supported!')

    t0 = perf_counter()
    result = fn(loss, call_x0, **opt_kwargs)
    elapsed = (perf_counter() - t0) / 60

    if optimizer in ('de', 'shgo'):
        result = OptimizeResult(dict(result))
        result.f = result.fun
        result.x_history = [list(result.population)] if optimizer == 'de' else [list(getattr(result, 'xl', []))]
        result.f_history = [-1.0]
        result.status = result.message
        result.niter = result.nit
        result.grad_history = []
    if use_scaling:
        d = result._asdict() if hasattr(result, '_asdict') else dict(result)
        d['x'] = np.asarray(d['x']) * (scale_arr if scale_arr.ndim == 1 else scale_arr[:, 1])
        result = opt.optResult(**{k: d[k] for k in opt.optResult._fields}) if hasattr(result, '_asdict') \
            else OptimizeResult(d)

    full = case_name + (strftime("%d_%m_%Y_%H_%M_%S", gmtime()) if uid is None else uid)
    log_dir = log_dir or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'optimization')
    rank0 = not (torch.distributed.is_available() and torch.distributed.is_initialized()) \
        or torch.distributed.get_rank() == 0
    if report and rank0:
        rel1 = rel2 = 'Unknown'
        if own is not None:
            p0 = own
            if arg0.ndim != 2:
                rel1 = (np.asarray(x0) * scale_arr - p0) / p0
            rel2 = (np.asarray(result.x) - p0) / p0
        comp_str = f'Using compression algorithm {comp_alg} with {compression[1]} points.\n' if compression[0] else ''
        kind = 'parameters' if arg0.ndim == 1 else 'bounds'
        rep = (f'{prob.accelerometer}\n{prob.material}\n{prob.geometry}\n' + extra_info + comp_str +
               f'Starting {kind}: {_a2s(np.asarray(x0) * scale_arr)}.\n'
               f'With relative error: {_a2s(rel1)}.\n'
               f'Initial loss: {result.f_history[0]}.\n'
               f'Elapsed time: {elapsed} min.\n'
               f'After optimization: {_a2s(result.x)}.\n'
               f'With relative error: {_a2s(rel2)}.\n'
               f'Resulting loss: {result.f}.\n'
               f'Optimization status: {result.status}.\n'
               f'Optimizer parameters: {opt_kwargs}.\n'
               f'Optimizer type: {optimizer}.\n'
               f'Scaling parameters used: {scale_arr}.\n')
        print(rep, end='')
        os.makedirs(log_dir, exist_ok=True)
        with open(os.path.join(log_dir, full + '.txt'), 'w+') as fh:
            fh.write(rep)
    if log and rank0:
        os.makedirs(log_dir, exist_ok=True)
        np.savez_compressed(os.path.join(log_dir, full), x=np.array(list(result.x_history) + [result.x]),
                            f=np.array(list(result.f_history) + [result.f]), k=np.array([result.niter]))
    return result
