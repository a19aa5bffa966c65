"""The negative-binomial family's reference: the density of include/stark_hip.h (STK_NEGBIN) restated
in np.longdouble, numpy alone.

With eta = alpha + x . beta, v = log phi, t = eta - v, sp(t) = log(1 + e^t), sigma(t) = 1 / (1 + e^-t):
    ll_i       = sum_{j < y_i} log1p(j / phi) + y_i eta_i - (y_i + phi) sp(t_i)
    d ll/d eta = y_i - (y_i + phi) sigma(t_i)
    d lp / d v = phi sum_i [psi(y_i + phi) - psi(phi)] - d alpha_lik - phi sum_i sp(t_i) + (a - 1) - b phi + 1
    lp         = sum_i ll_i - (pa alpha^2 + pb |beta|^2) / 2 + (a - 1) v - b phi + v
(pa, pb = 1 / s^2 of the normal(0, s) priors; phi ~ gamma(a, b); the last v is the Jacobian of phi = e^v).

The phi-only sums, per distinct count y:
    A1(y) = sum_{j < y} log1p(j / phi),    S2(y) = psi(y + phi) - psi(phi) = sum_{j < y} 1 / (phi + j)
are the finite sums themselves up to FINITE_MAX terms; the part of a larger count past FINITE_MAX comes from
the Stirling / asymptotic series of lgamma and digamma at x >= FINITE_MAX + phi (`series_tail`), whose
truncation error there is below 1e-30.  tests/test_host_negbin.py checks the two against each other where
both apply.
"""
import numpy as np

L = np.longdouble
FINITE_MAX = 4096          # counts up to here: the finite sums alone
DBL_MAX = np.finfo(np.float64).max


def finite_sums(y, phi):
    """(A1, S2) of one count y by the finite sums, any y that fits memory."""
    j = np.arange(int(y), dtype=L)
    phi = L(phi)
    return np.log1p(j / phi).sum(), (1 / (phi + j)).sum()


def _B(x):    # lgamma(x) - [(x - 1/2) ln x - x + ln(2 pi) / 2]
    s = 1 / (x * x)
    return (L(1) / 12 - (L(1) / 360 - (L(1) / 1260 - (L(1) / 1680 - L(1) / 1188 * s) * s) * s) * s) / x


def _A(x):    # psi(x) - ln x
    s = 1 / (x * x)
    return -(L(1) / 2 + (L(1) / 12 - (L(1) / 120 - (L(1) / 252 - (L(1) / 240 - L(1) / 132 * s) * s) * s) * s) / x) / x


def series_tail(k0, y, phi):
    """(sum_{j = k0}^{y - 1} log1p(j / phi), sum_{j = k0}^{y - 1} 1 / (phi + j)) from the series; k0 + phi >~ 1000.
    lgamma(x1) - lgamma(x0) - M v with the v terms cancelled analytically: x1 - x0 = M."""
    phi, k0, y = L(phi), L(int(k0)), L(int(y))
    x0, x1, M = k0 + phi, y + phi, y - k0
    a1 = (x1 - L(1) / 2) * np.log1p(y / phi) - (x0 - L(1) / 2) * np.log1p(k0 / phi) - M + (_B(x1) - _B(x0))
    s2 = np.log1p(M / x0) + (_A(x1) - _A(x0))
    return a1, s2


def count_terms(y, phi):
    """(A1, S2) of one count."""
    y = int(y)
    if y <= FINITE_MAX:
        return finite_sums(y, phi)
    a, s = finite_sums(FINITE_MAX, phi)
    ta, ts = series_tail(FINITE_MAX, y, phi)
    return a + ta, s + ts


def phi_terms(y, phi):
    """(sum_i A1(y_i), sum_i S2(y_i)) over the counts y, in longdouble: cumulative finite sums for the counts
    up to FINITE_MAX, the series for the rest of a larger one."""
    y = np.asarray(y, np.int64).reshape(-1)
    phi = L(phi)
    vals, mult = np.unique(y, return_counts=True)
    top = int(min(vals.max(), FINITE_MAX))
    j = np.arange(top, dtype=L)
    with np.errstate(over="ignore", divide="ignore"):
        c1 = np.concatenate([[L(0)], np.cumsum(np.log1p(j / phi))])      # c1[k] = sum_{j < k} log1p(j / phi)
        c2 = np.concatenate([[L(0)], np.cumsum(1 / (phi + j))])
        a1 = s2 = L(0)
        for v, m in zip(vals, mult):
            if v <= FINITE_MAX:
                a1, s2 = a1 + L(m) * c1[v], s2 + L(m) * c2[v]
            else:
                ta, ts = series_tail(FINITE_MAX, v, phi)
                a1, s2 = a1 + L(m) * (c1[FINITE_MAX] + ta), s2 + L(m) * (c2[FINITE_MAX] + ts)
    return a1, s2


def ref_lpgrad(X, y, q, prior=(0.0, 0.0), phi_prior=(1.0, 0.0)):
    """lp (C,) and gradient (C, d + 2) at the rows of q = (alpha, beta[1..d], v), in np.longdouble.  An exp
    past the largest double is +inf, as the fp64 kernels overflow there; phi = e^v outside the doubles'
    normal range (0 or inf in fp64) makes lp NaN."""
    Xl, yl, ql = X.astype(L), y.astype(L)[:, None], np.asarray(q).astype(L)
    C = ql.shape[0]
    pa, pb = (0.0 if s in (0.0, None) else 1.0 / (L(s) * L(s)) for s in prior)
    a, b = L(phi_prior[0]), L(phi_prior[1])
    lp = np.empty(C, L)
    g = np.empty((C, ql.shape[1]), L)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        v = ql[:, -1]
        phi = np.exp(v)
        eta = ql[:, 0][None, :] + Xl @ ql[:, 1:-1].T                 # (n, C)
        t = eta - v[None, :]
        e = np.exp(-np.abs(t))
        sp = np.maximum(t, 0) + np.log1p(e)
        sp = np.where(np.isnan(t), np.nan, sp)
        w = yl + phi[None, :]
        r = np.where(t >= 0, yl * e - phi[None, :], yl - phi[None, :] * e) / (1 + e)     # y - (y + phi) sigma(t)
        r = np.where(np.isnan(t), np.nan, r)
        slik = (yl * eta - w * sp).sum(0)
        ssp = sp.sum(0)
        ga = r.sum(0)
        for c in range(C):
            f = float(phi[c])
            if not (f > 0 and np.isfinite(f)):
                lp[c] = np.nan
                g[c] = np.nan
                continue
            a1, s2 = phi_terms(y, phi[c])
            lp[c] = (slik[c] + a1 - (pa * ql[c, 0] ** 2 + pb * (ql[c, 1:-1] ** 2).sum()) / 2
                     + (a - 1) * v[c] - b * phi[c] + v[c])
            g[c, 0] = ga[c] - pa * ql[c, 0]
            g[c, 1:-1] = r[:, c] @ Xl - pb * ql[c, 1:-1]
            g[c, -1] = phi[c] * s2 - ga[c] - phi[c] * ssp[c] + (a - 1) - b * phi[c] + 1
        lp[np.abs(lp) > DBL_MAX] = np.sign(lp[np.abs(lp) > DBL_MAX]) * np.inf
    return lp, g


def ref_poisson_lp(X, y, q):
    """sum(y eta - e^eta) at the rows of q = (alpha, beta[1..d]): Stan's poisson_log, propto, for the phi -> inf limit."""
    Xl, yl, ql = X.astype(L), y.astype(L)[:, None], np.asarray(q).astype(L)
    eta = ql[:, 0][None, :] + Xl @ ql[:, 1:].T
    return (yl * eta - np.exp(eta)).sum(0)
