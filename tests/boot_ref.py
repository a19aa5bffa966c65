"""Restatements shared by tests/test_host_boot.py and tests/test_gpu_boot.py (no test in here).

weights_np     the bootstrap weights from engine.philox_words and the slicing of csrc/boot_math.h, with the
               Poisson thresholds recomputed here from the definition (decimal arithmetic);
weighted       lp, gradient and wsum of a shard at R points under given weights [n, R], in any float type,
               with the scales the bars are taken from;
newton         the maximiser of the weighted log density summed over shards, by a damped full Newton solve;
NumpyModel     a host stand-in for engine.Model with the methods engine.bootstrap calls.
"""
import math
from decimal import Decimal, getcontext

import numpy as np

L = np.longdouble
FAMILIES = ("logistic", "poisson", "linear")


def thresholds_ref():
    """floor(2^32 cdf_k) of Poisson(1), k = 0 .. 12, and cdf_k itself at 60 digits."""
    getcontext().prec = 60
    e1 = 1 / Decimal(1).exp()
    cdf, acc = [], Decimal(0)
    for k in range(13):
        acc += e1 / Decimal(math.factorial(k))
        cdf.append(acc)
    return [int((c * Decimal(2 ** 32)).to_integral_value(rounding="ROUND_FLOOR")) for c in cdf], cdf


def words_np(seed, stream, rows, reps):
    """The 32-bit word of every (row, replicate): [nrows, nreps] uint64."""
    from stark_amd import engine
    i = np.asarray(rows, np.int64).astype(np.uint64)[:, None]
    b = np.asarray(reps, np.uint64)[None, :]
    u = np.uint64
    c0 = (i >> u(4)) & u(0xFFFFFFFF)
    c1 = ((((i >> u(36)) & u(0xFFFFFFFF)) << u(2)) | (i & u(3))) & u(0xFFFFFFFF)
    c2 = (u(int(stream)) << u(12)) | b
    ra, rb = engine.philox_words(seed, c0 + 0 * b, c1 + 0 * b, c2 + 0 * i, u(0x22))
    four = np.stack([ra & u(0xFFFFFFFF), ra >> u(32), rb & u(0xFFFFFFFF), rb >> u(32)])
    sel = ((i >> u(2)) & u(3)).astype(np.int64) + 0 * b.astype(np.int64)
    return np.take_along_axis(four, sel[None], axis=0)[0]


def weights_np(seed, stream, rows, reps, kind):
    w = words_np(seed, stream, rows, reps)
    if kind == "poisson":
        T = np.array(thresholds_ref()[0], np.uint64)
        return (w[:, :, None] >= T[None, None, :]).sum(axis=2).astype(np.float64)
    return -np.log((w.astype(np.float64) + 0.5) * 2.0 ** -32)


def make_data(family, n, d, seed):
    """n rows of X ~ U(-1.7, 1.7) (row n // 2 all zero), y from the family, and the generating point."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.7, 1.7, (n, d))
    X[n // 2] = 0.0
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    eta = 0.3 + X @ beta
    if family == "logistic":
        y = (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.int32)
        truth = np.concatenate([[0.3], beta])
    elif family == "poisson":
        y = rng.poisson(np.exp(eta)).astype(np.int32)
        truth = np.concatenate([[0.3], beta])
    else:
        y = eta + 0.7 * rng.normal(size=n)
        truth = np.concatenate([[0.3], beta, [np.log(0.7)]])
    return X, y, truth


def weighted(family, X, y, Q, W, prior=None, ft=L):
    """lp [R], grad [R, D], wsum [R] of the rows (X, y) at the points Q [R, D] under the weights W [n, R], in
    the float type ft, and the scales of the bars: lp_scale [R] = sum w |ll| + the absolute prior and Jacobian
    terms, g_scale [R, D] = sum_i w_i |x_ij| |resid_i| per coordinate (x = 1 for alpha; for u the absolute
    terms sum w z^2 + wsum + 1) + the absolute prior term."""
    n, d = X.shape
    Xf, Qf, Wf = X.astype(ft), np.asarray(Q).astype(ft), np.asarray(W).astype(ft)
    yf = np.asarray(y).astype(ft)[:, None]
    R, D = Qf.shape
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        eta = Qf[:, 0][None, :] + Xf @ Qf[:, 1:d + 1].T            # [n, R]
        if family == "logistic":
            z = (2 * yf - 1) * eta
            ll = np.minimum(z, 0) - np.log1p(np.exp(-np.abs(z)))
            res = yf - 1 / (1 + np.exp(-eta))
        elif family == "poisson":
            ll = yf * eta - np.exp(eta)
            res = yf - np.exp(eta)
        else:
            u = Qf[:, -1][None, :]
            r = yf - eta
            zz = r * r * np.exp(-2 * u)
            ll = -u - ft(0.5) * zz
            res = r * np.exp(-2 * u)
        wsum = Wf.sum(axis=0)
        lp, lp_scale = (Wf * ll).sum(axis=0), (Wf * np.abs(ll)).sum(axis=0)
        wr = Wf * res
        g, gs = np.zeros((R, D), ft), np.zeros((R, D), ft)
        g[:, 0], gs[:, 0] = wr.sum(axis=0), np.abs(wr).sum(axis=0)
        g[:, 1:d + 1], gs[:, 1:d + 1] = wr.T @ Xf, np.abs(wr).T @ np.abs(Xf)
        if family == "linear":
            swz = (Wf * zz).sum(axis=0)
            g[:, -1], gs[:, -1] = swz - wsum + 1, swz + wsum + 1
            lp, lp_scale = lp + Qf[:, -1], lp_scale + np.abs(Qf[:, -1])
        if prior is not None:
            pa, pb = 1 / ft(prior[0]) ** 2, 1 / ft(prior[1]) ** 2
            ta, tb = pa * Qf[:, 0] ** 2 / 2, pb * (Qf[:, 1:d + 1] ** 2).sum(axis=1) / 2
            lp, lp_scale = lp - ta - tb, lp_scale + ta + tb
            g[:, 0], gs[:, 0] = g[:, 0] - pa * Qf[:, 0], gs[:, 0] + np.abs(pa * Qf[:, 0])
            g[:, 1:d + 1] -= pb * Qf[:, 1:d + 1]
            gs[:, 1:d + 1] += np.abs(pb * Qf[:, 1:d + 1])
    return lp, g, wsum, lp_scale, gs


def _hessian(family, X, y, q, w, prior):
    n, d = X.shape
    Xt = np.hstack([np.ones((n, 1)), X])
    eta = Xt @ q[:d + 1]
    D = q.size
    H = np.zeros((D, D))
    if family == "logistic":
        p = 1 / (1 + np.exp(-eta))
        H[:d + 1, :d + 1] = -(Xt * (w * p * (1 - p))[:, None]).T @ Xt
    elif family == "poisson":
        H[:d + 1, :d + 1] = -(Xt * (w * np.exp(eta))[:, None]).T @ Xt
    else:
        s2 = np.exp(-2 * q[-1])
        r = y - eta
        H[:d + 1, :d + 1] = -s2 * (Xt * w[:, None]).T @ Xt
        H[:d + 1, -1] = H[-1, :d + 1] = -2 * s2 * (Xt * w[:, None]).T @ r
        H[-1, -1] = -2 * s2 * (w * r * r).sum()
    if prior is not None:
        H[0, 0] -= 1 / prior[0] ** 2
        H[np.arange(1, d + 1), np.arange(1, d + 1)] -= 1 / prior[1] ** 2
    return H


def newton(family, shards, weights, q0, prior=None, iters=100):
    """argmax over q of the shards' weighted log densities summed -- sum_s [sum_i w_si ll_si(q) + prior +
    Jacobian], what engine.laplace and engine.bootstrap maximise (a shard's density carries its own prior and
    Jacobian) -- on the union of the rows; weights[s] the [n_s] weights of shard s (None: ones).  A damped
    Newton iteration in float64 from q0, run until the step is below 1e-13 of the scale of q.
    Returns (q, cov = (-H)^-1)."""
    X = np.vstack([np.asarray(s["x"], np.float64) for s in shards])
    y = np.concatenate([np.asarray(s["y"], np.float64) for s in shards])
    w = np.ones(X.shape[0]) if weights is None else np.concatenate([np.asarray(v, np.float64) for v in weights])
    q = np.array(q0, np.float64)
    ns = len(shards)
    hprior = None if prior is None else (prior[0] / np.sqrt(ns), prior[1] / np.sqrt(ns))   # ns copies of the prior

    def f(p):
        lp, g, *_ = weighted(family, X, y, p[None], w[:, None], hprior, np.float64)
        lp, g = float(lp[0]), g[0].copy()
        if family == "linear":                   # ns Jacobians
            lp, g[-1] = lp + (ns - 1) * p[-1], g[-1] + (ns - 1)
        return lp, g

    lp, g = f(q)
    for _ in range(iters):
        H = _hessian(family, X, y, q, w, hprior)
        step = np.linalg.solve(-H, g)
        a = 1.0
        while True:
            lpn, gn = f(q + a * step)
            if np.isfinite(lpn) and lpn >= lp - 1e-12 * abs(lp):
                break
            a *= 0.5
            if a < 1e-6:
                raise RuntimeError("newton: no ascent step")
        q, lp, g = q + a * step, lpn, gn
        if np.abs(a * step).max() < 1e-13 * max(1.0, np.abs(q).max()):
            break
    cov = np.linalg.inv(-_hessian(family, X, y, q, w, hprior))
    return q, 0.5 * (cov + cov.T)


def newton_replicates(family, shards, streams, B, kind, seed, q0, prior=None):
    """The Newton solve of every replicate b < B on the twin's weights: [B, D]."""
    from stark_amd import engine
    out = []
    Ws = [engine.boot_weights(seed, st, 0, np.asarray(s["x"]).shape[0], 0, B, kind) for s, st in zip(shards, streams)]
    for b in range(B):
        out.append(newton(family, shards, [W[:, b] for W in Ws], q0, prior)[0])
    return np.array(out)


class NumpyModel:
    """engine.Model's bootstrap-facing methods on the host: float64 numpy on the twin's weights."""

    def __init__(self, family, shards, prior=None, poison=()):
        self.family, self.shards, self.prior, self.poison = family, shards, prior, set(poison)
        self.nshards = len(shards)
        d = np.asarray(shards[0]["x"]).shape[1]
        self.D = [d + (2 if family == "linear" else 1)] * self.nshards
        self.calls = 0

    def log_density_grad_boot(self, q, shard=None, rep0=0, seed=0, streams=None, kind="exponential"):
        from stark_amd import engine
        q = np.atleast_2d(np.asarray(q, np.float64))
        ids = range(self.nshards) if shard is None else [shard]
        self.calls += 1
        lps, gs, wss = [], [], []
        for k, s in enumerate(ids):
            X, y = np.asarray(self.shards[s]["x"], np.float64), self.shards[s]["y"]
            st = s if streams is None else int(np.atleast_1d(streams)[k])
            W = engine.boot_weights(seed, st, 0, X.shape[0], rep0, q.shape[0], kind)
            lp, g, ws, *_ = weighted(self.family, X, y, q, W, self.prior, np.float64)   # a shard's own density
            for b in self.poison:
                if rep0 <= b < rep0 + q.shape[0]:
                    lp[b - rep0] = np.nan
            lps.append(lp), gs.append(g), wss.append(ws)
        if shard is None:
            return np.array(lps), np.array(gs), np.array(wss)
        return lps[0], gs[0], wss[0]
