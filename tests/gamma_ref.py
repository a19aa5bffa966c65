"""The gamma family's log density and gradient in np.longdouble, straight from the formulas of include/stark_hip.h
(STK_GAMMA): the reference of tests/test_gpu_gamma.py and tests/test_host_gamma.py.

With a = exp(u), n rows, eta_i = alpha + x_i . beta, ly_i = log y_i, L = sum_i ly_i and t_i = ly_i - eta_i,
  lp             = n kappa(a) - L - a H + u  - (pa alpha^2 + pb |beta|^2) / 2 + (s - 1) u - r a
  kappa(a)       = a log a - a - lgamma(a),   H = sum_i (e^t_i - 1 - t_i)
  d lp / d eta_i = a (e^t_i - 1)
  d lp / d u     = a [n (log a - psi(a)) - H] + 1 + (s - 1) - r a
(Stan's `y ~ gamma(a, a exp(-eta))`, nothing dropped, plus the Jacobian u; shape ~ gamma(s, r)).  lgamma and psi come
from Stirling's series after a recurrence shift to an argument >= 20 and kappa, kappa' are formed from them by plain
subtraction in longdouble: none of the device code's remainders or recurrences.  np.expm1, np.log and plain sums on
longdouble: no table, no clamp.  One thing is taken from fp64: the shape e^u is a double, so a point whose e^u is 0
or inf as a double has no density (NaN), though longdouble's wider exponent could carry it.
"""
import numpy as np

L = np.longdouble
HALF_LOG_2PI = np.log(2 * L("3.14159265358979323846264338327950288")) / 2
# B_2k, k = 1 .. 9
_B = [(1, 6), (-1, 30), (1, 42), (-1, 30), (5, 66), (-691, 2730), (7, 6), (-3617, 510), (43867, 798)]


def _shift(a):
    """(x, sum log(a + k), sum 1 / (a + k)) over k < m with x = a + m the first argument >= 20; a > 0, any shape."""
    x = np.array(a, L, ndmin=1)
    sl, sr = np.zeros_like(x), np.zeros_like(x)
    while True:
        m = x < 20
        if not m.any():
            return x, sl, sr
        sl[m] += np.log(x[m])
        sr[m] += 1 / x[m]
        x[m] += 1


def lgamma(a):
    x, sl, _ = _shift(a)
    s = sum(L(p) / L(q) / (2 * k * (2 * k - 1)) / x ** (2 * k - 1) for k, (p, q) in enumerate(_B, 1))
    return (x - L(1) / 2) * np.log(x) - x + HALF_LOG_2PI + s - sl


def digamma(a):
    x, _, sr = _shift(a)
    s = sum(L(p) / L(q) / (2 * k) / x ** (2 * k) for k, (p, q) in enumerate(_B, 1))
    return np.log(x) - 1 / (2 * x) - s - sr


def shape_terms(a):
    """(kappa(a), kappa'(a)) in longdouble, by subtraction; a > 0 and finite, a scalar or an array (arrays back)."""
    a = np.array(a, L, ndmin=1)
    return a * np.log(a) - a - lgamma(a), np.log(a) - digamma(a)


def ref_lpgrad(X, y, q, shape_prior=None, prior=(0.0, 0.0)):
    """lp (C,) and gradient (C, d + 2) at the rows of q = (alpha, beta[1..d], u = log shape), in np.longdouble."""
    Xl, ql = np.asarray(X).astype(L), np.asarray(q).astype(L)
    ly = np.log(np.asarray(y).astype(L))[:, None]
    n = L(Xl.shape[0])
    pa, pb = (L(0) if s in (0.0, None) else 1 / (L(s) * L(s)) for s in prior)
    ps, pr = (L(1), L(0)) if shape_prior is None else (L(shape_prior[0]), L(shape_prior[1]))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        u = ql[:, -1]
        a = np.exp(u)
        a64 = a.astype(np.float64)                                    # the shape is a double: where e^u is 0 or inf
        ok = np.isfinite(a64) & (a64 > 0)                             # there (|u| past 745 / 709) there is no density
        k0, k1 = (np.where(ok, k, L(np.nan)) for k in shape_terms(np.where(ok, a, L(1))))
        t = ly - (ql[:, 0][None, :] + Xl @ ql[:, 1:-1].T)             # (n, C)
        em1 = np.expm1(t)
        H = (em1 - t).sum(0)
        lp = (n * k0 - ly.sum() - a * H + u - (pa * ql[:, 0] ** 2 + pb * (ql[:, 1:-1] ** 2).sum(1)) / 2
              + (ps - 1) * u - pr * a)
        de = a[None, :] * em1
        g = np.concatenate([de.sum(0)[:, None] - pa * ql[:, :1], de.T @ Xl - pb * ql[:, 1:-1],
                            (a * (n * k1 - H) + 1 + (ps - 1) - pr * a)[:, None]], axis=1)
    return lp, g
