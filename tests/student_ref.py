"""The Student-t family's log density and gradient in np.longdouble, straight from the formulas of
include/stark_hip.h (STK_STUDENT): the reference of tests/test_gpu_student.py and tests/test_host_student.py.

With eta_i = alpha + x_i . beta, sigma = exp(s), z_i = (y_i - eta_i) / sigma and w_i = z_i^2 / nu,
  lp             = -(nu + 1)/2 sum_i log1p(w_i) - n s + s  - (pa alpha^2 + pb |beta|^2) / 2
  d lp / d eta_i = (nu + 1) z_i / (sigma (nu + z_i^2))
  d lp / d s     = (nu + 1) sum_i z_i^2 / (nu + z_i^2) - n + 1
(Stan's `y ~ student_t(nu, eta, sigma)` with nu as data drops the lgamma, log nu and log pi terms).  Written with
np.log1p and plain divisions on longdouble: no reciprocal, no table, none of the device code's algebra.
"""
import numpy as np

L = np.longdouble
DBL_MAX = np.finfo(np.float64).max


def ref_lpgrad(X, y, q, nu, prior=(0.0, 0.0)):
    """lp (C,) and gradient (C, d + 2) at the rows of q = (alpha, beta[1..d], s = log sigma), in np.longdouble."""
    Xl, yl, ql, nul = np.asarray(X).astype(L), np.asarray(y).astype(L)[:, None], np.asarray(q).astype(L), L(nu)
    n = L(Xl.shape[0])
    pa, pb = (L(0) if s in (0.0, None) else 1 / (L(s) * L(s)) for s in prior)
    with np.errstate(over="ignore", invalid="ignore"):
        s = ql[:, -1]
        sigma = np.exp(s)
        eta = ql[:, 0][None, :] + Xl @ ql[:, 1:-1].T                  # (n, C)
        z = (yl - eta) / sigma[None, :]
        z2 = z * z
        lp = (-(nul + 1) / 2 * np.log1p(z2 / nul).sum(0) - n * s + s
              - (pa * ql[:, 0] ** 2 + pb * (ql[:, 1:-1] ** 2).sum(1)) / 2)
        de = (nul + 1) * z / (sigma[None, :] * (nul + z2))
        g = np.concatenate([de.sum(0)[:, None] - pa * ql[:, :1], de.T @ Xl - pb * ql[:, 1:-1],
                            ((nul + 1) * (z2 / (nul + z2)).sum(0) - n + 1)[:, None]], axis=1)
    return lp, g


def max_w(X, y, q, nu):
    """Per point: the largest w_i = z_i^2 / nu over the rows (longdouble), and whether some z_i^2 is past the
    largest double (where an fp64 evaluation overflows)."""
    Xl, yl, ql = np.asarray(X).astype(L), np.asarray(y).astype(L)[:, None], np.asarray(q).astype(L)
    with np.errstate(over="ignore"):
        z = (yl - (ql[:, 0][None, :] + Xl @ ql[:, 1:-1].T)) / np.exp(ql[:, -1])[None, :]
        z2 = (z * z).max(0)
    return z2 / L(nu), z2 > DBL_MAX


def ref_linear_lp(X, y, q):
    """The linear family's density at the same points: -sum z^2 / 2 - n s + s (Stan's normal, constants dropped)."""
    Xl, yl, ql = np.asarray(X).astype(L), np.asarray(y).astype(L)[:, None], np.asarray(q).astype(L)
    s = ql[:, -1]
    z = (yl - (ql[:, 0][None, :] + Xl @ ql[:, 1:-1].T)) / np.exp(s)[None, :]
    return -(z * z).sum(0) / 2 - L(Xl.shape[0]) * s + s
