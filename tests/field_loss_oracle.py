"""The field loss on the plate by the CPU oracle (test infrastructure, not a test): loss and gradient by the adjoint
method from the oracle's own matrices and refined solves (oracle/plate_oracle.py), in the conventions of
include/pfr.h's pfr_field_loss_sweep -- what tests/test_gpu_field_loss.py compares the device with, itself checked
against 4th-order central differences of the oracle field loss in tests/test_field_loss_cpu.py."""
import numpy as np

from oracle.plate_oracle import (RHS_WEIGHTS_D, OracleProblem, coeffs18_jacobian, refined_solve, sparse_lu, _mr)
from synthetic_fieldloss import scatter, terms_g


def field_loss(orc: OracleProblem, freqs, data, loss_type, theta, rows=None, v=None) -> float:
    """The mean over the frequencies of the term of ``loss_type`` on the rows ``rows`` of the oracle's solutions."""
    tot = 0.0
    for i, f in enumerate(np.asarray(freqs, dtype=np.float64)):
        x = orc.solve(f, theta)[0]
        tot += float(terms_g(x if rows is None else x[rows], data[i], v, loss_type)[0])
    return tot / len(freqs)


def field_loss_and_grad(orc: OracleProblem, freqs, data, loss_type, theta, rows=None, v=None, scaling=None):
    """(loss, d loss / d theta): per frequency A^T lam = g / F scattered to the rows, w_k += -lam^T S_k x + e_k lam^T b0,
    gradient Re(w J) with the oracle's coefficient Jacobian (``plate_oracle.loss_and_grad``'s construction)."""
    theta = np.asarray(theta, dtype=np.float64)
    s = np.ones_like(theta) if scaling is None else np.asarray(scaling, dtype=np.float64)
    phys = theta * s
    freqs = np.asarray(freqs, dtype=np.float64)
    c = orc.coefficients(phys)
    e = np.concatenate([np.zeros(12), RHS_WEIGHTS_D])
    w = np.zeros(18, dtype=complex)
    tot = 0.0
    for i, f in enumerate(freqs):
        A = orc.matrix(f, c)
        lu = sparse_lu(A)
        x = refined_solve(lu, A, orc.rhs_vec * orc.rhs_scale(f, c))
        term, g = terms_g(x if rows is None else x[rows], data[i], v, loss_type)
        tot += float(term)
        lam = refined_solve(lu, A, scatter(g, rows, orc.n) / freqs.size, trans=True)
        w += -_mr(orc.mats[:18], lam[orc.rows] * x[orc.cols]) + e * (lam @ orc.rhs_vec)
    J = coeffs18_jacobian(orc.atype, orc.h, phys, orc.angles)
    return tot / freqs.size, np.real(w @ J) * s


def fd_grad(orc: OracleProblem, freqs, data, loss_type, theta, rows=None, v=None, rel=2e-4):
    """4th-order central differences of ``field_loss`` (``plate_oracle.fd_grad``'s stencil and step)."""
    theta = np.asarray(theta, dtype=np.float64)
    g = np.zeros_like(theta)
    for p in range(theta.size):
        h = rel * abs(theta[p])
        vals = []
        for m in (-2, -1, 1, 2):
            t = theta.copy()
            t[p] += m * h
            vals.append(field_loss(orc, freqs, data, loss_type, t, rows, v))
        g[p] = (vals[0] - 8 * vals[1] + 8 * vals[2] - vals[3]) / (12 * h)
    return g
