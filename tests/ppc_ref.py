"""Restatements shared by tests/test_host_ppc.py and tests/test_gpu_ppc.py (no test in here).

counters       the Philox counter of call j of element (row, draw), as csrc/yrep_math.h lays it out;
uv             (U, V) of that call from engine.philox_words;
yrep_np        the generator of include/stark_hip.h in numpy -- Philox, Bernoulli, Box-Muller, inversion, PTRS and the
               normal tail -- with the number of PTRS attempts of every element;
eta_ld         eta in long double;
restate        stats / obs / rows of a shard in long double from GIVEN replicates, with the scales of the bars;
pool           engine.ppc's pooling, written out.
"""
import math

import numpy as np

L = np.longdouble
FAMILIES = ("logistic", "poisson", "linear")
TAG_YREP = 0x26
FRAGILE = 1e-10
PTRS_MIN, NORMAL_MIN = 10.0, 2.0 ** 30
_lgamma = np.frompyfunc(math.lgamma, 1, 1)


def counters(stream, rows, draws, j):
    """[nrows, ndraws] arrays c0, c1, c2, c3 (uint64 holding 32-bit words)."""
    u = np.uint64
    i = np.asarray(rows, np.int64).astype(u)[:, None]
    s = np.asarray(draws, np.int64).astype(u)[None, :]
    m32 = u(0xFFFFFFFF)
    c0 = (i & m32) + u(0) * s
    c1 = ((i >> u(32)) | (s << u(8))) & m32
    c2 = ((u(int(stream)) << u(12)) | u(int(j))) + u(0) * (i + s)
    return c0, c1, c2, u(TAG_YREP) + u(0) * (i + s)


def uv(seed, stream, rows, draws, j):
    from stark_amd import engine
    ra, rb = engine.philox_words(seed, *counters(stream, rows, draws, j))
    f = lambda x: ((x >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    return f(ra), f(rb)


def normal(U, V):
    return np.sqrt(-2.0 * np.log(U)) * np.cos(6.283185307179586 * V)


def yrep_np(family, seed, stream, row0, draw0, eta, u=None):
    """(y_rep [n, S], attempts [n, S]): attempts is the number of PTRS attempts made (0 off the PTRS range, 65 where
    the fallback after 64 rejections was taken)."""
    eta = np.asarray(eta, np.float64)
    n, S = eta.shape
    rows, draws = row0 + np.arange(n), draw0 + np.arange(S)
    U, V = uv(seed, stream, rows, draws, 0)
    att = np.zeros(eta.shape, np.int64)
    with np.errstate(all="ignore"):
        if family == "logistic":
            e = np.exp(-np.abs(eta))
            g = np.where(eta >= 0, 1 / (1 + e), e / (1 + e))
            return np.where(np.isnan(eta), np.nan, (U < g).astype(np.float64)), att
        if family == "linear":
            sigma = np.exp(np.asarray(u, np.float64))[None, :]
            y = eta + sigma * normal(U, V)
            return np.where(np.isfinite(eta) & np.isfinite(sigma) & np.isfinite(y), y, np.nan), att
        mu = np.exp(eta)
        y = np.full(eta.shape, np.nan)
        # ---- mu < 10: inversion by upward search
        lo = mu < PTRS_MIN
        k, p = np.zeros(eta.shape), np.exp(-mu)
        c = p.copy()
        for _ in range(128):
            go = lo & (U > c)
            if not go.any():
                break
            k = np.where(go, k + 1, k)
            p = np.where(go, p * (mu / np.maximum(k, 1)), p)
            c = np.where(go, c + p, c)
        y[lo] = k[lo]
        # ---- 10 <= mu < 2^30: PTRS
        mid = (mu >= PTRS_MIN) & (mu < NORMAL_MIN)
        if mid.any():
            slam, loglam = np.sqrt(mu), np.log(mu)
            b = 0.931 + 2.53 * slam
            a = -0.059 + 0.02483 * b
            invalpha = 1.1239 + 1.1328 / (b - 3.4)
            vr = 0.9277 - 3.6224 / (b - 2.0)
            pend = mid.copy()
            for j in range(64):
                if not pend.any():
                    break
                if j > 0:
                    U, V = uv(seed, stream, rows, draws, j)
                att[pend] += 1
                Us = U - 0.5
                us = 0.5 - np.abs(Us)
                kk = np.floor((2.0 * a / us + b) * Us + mu + 0.43)
                acc = (us >= 0.07) & (V <= vr)
                rej = ~acc & ((kk < 0) | ((us < 0.013) & (V > us)))
                test = pend & ~acc & ~rej
                lg = np.zeros(eta.shape)
                lg[test] = _lgamma(kk[test] + 1.0).astype(np.float64)
                lhs = np.log(V) + np.log(invalpha) - np.log(a / (us * us) + b)
                rhs = -mu + kk * loglam - lg
                ok = pend & (acc | (test & (lhs <= rhs)))
                y[ok] = kk[ok]
                pend &= ~ok
            y[pend] = np.floor(mu[pend] + 0.5)
            att[pend] = 65
        # ---- 2^30 <= mu < inf: the normal approximation, on call 0
        hi = (mu >= NORMAL_MIN) & np.isfinite(mu)
        if hi.any():
            U0, V0 = uv(seed, stream, rows, draws, 0)
            y[hi] = np.maximum(0.0, np.floor(mu + np.sqrt(mu) * normal(U0, V0) + 0.5))[hi]
        return y, att


def make_data(family, n, d, seed):
    """X ~ U(-1.5, 1.5) (row n // 2 all zero), y from the family at a generating point of moderate eta."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.5, 1.5, (n, d))
    X[n // 2] = 0.0
    beta = rng.normal(0, 0.8 / np.sqrt(d), d)
    a0 = 1.0 if family == "poisson" else 0.3
    eta = a0 + X @ beta
    if family == "logistic":
        y = (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.int32)
        truth = np.concatenate([[a0], beta])
    elif family == "poisson":
        y = rng.poisson(np.exp(eta)).astype(np.int32)
        truth = np.concatenate([[a0], beta])
    else:
        y = eta + 0.7 * rng.normal(size=n)
        truth = np.concatenate([[a0], beta, [np.log(0.7)]])
    return rng, X, y, truth


def eta_ld(X, Q):
    d = X.shape[1]
    Qf = np.asarray(Q).astype(L)
    return Qf[:, 0][None, :] + X.astype(L) @ Qf[:, 1:d + 1].T            # [n, S]


def pearson(family, eta, u, z):
    """The terms (z - m)^2 / V [n, S] in eta's float type; V = 0: 0 where z = m, else +inf."""
    ft = eta.dtype.type
    z = np.asarray(z).astype(ft)
    with np.errstate(all="ignore"):
        if family == "linear":
            r = z - eta
            return r * r * np.exp(-2 * np.asarray(u).astype(ft))[None, :]
        if family == "logistic":
            e = np.exp(-np.abs(eta))
            g = np.where(eta >= 0, 1 / (1 + e), e / (1 + e))
            omg = np.where(eta >= 0, e / (1 + e), 1 / (1 + e))
            V = e / ((1 + e) * (1 + e))
            r = np.where(z != 0, omg, -g)                          # z in {0, 1}
            r = np.where(np.isnan(z), np.nan, r)
        else:
            V = np.exp(eta)
            r = z - V
        t = r * r / V
        return np.where(V == 0, np.where(r == 0, ft(0), ft(np.inf)), t)


def restate(family, X, y, Q, yrep):
    """stats [S, 8], obs [8], rows [n, 4] in long double from the replicates yrep [S, n], and the scales of the
    sums that carry rounding: sscale [S, 8] and rscale [n, 4] (sum of absolute terms; 0 for counts and extrema)."""
    n, d = X.shape
    eta = eta_ld(X, Q)
    u = np.asarray(Q)[:, -1] if family == "linear" else None
    yr = np.asarray(yrep).T.astype(L)                              # [n, S]
    yo = np.asarray(y).astype(L)[:, None]
    S = yr.shape[1]
    stats, sscale = np.zeros((S, 8), L), np.zeros((S, 8), L)
    with np.errstate(all="ignore"):
        trep, tobs = pearson(family, eta, u, yr), pearson(family, eta, u, yo + 0 * yr)
        bad = np.isnan(yr)
        trep = np.where(bad, np.nan, trep)
        stats[:, 0], sscale[:, 0] = yr.sum(axis=0), np.abs(yr).sum(axis=0)
        stats[:, 1], sscale[:, 1] = (yr * yr).sum(axis=0), (yr * yr).sum(axis=0)
        stats[:, 2], stats[:, 3] = yr.max(axis=0), yr.min(axis=0)
        stats[:, 4] = (yr == 0).sum(axis=0)
        stats[:, 5], sscale[:, 5] = trep.sum(axis=0), np.abs(trep).sum(axis=0)
        stats[:, 6], sscale[:, 6] = tobs.sum(axis=0), np.abs(tobs).sum(axis=0)
        stats[:, 7] = bad.sum(axis=0)
        yv = yo[:, 0]
        obs = np.array([yv.sum(), (yv * yv).sum(), yv.max(), yv.min(), (yv == 0).sum(), n, 0, 0], L)
        rows, rscale = np.zeros((n, 4), L), np.zeros((n, 4), L)
        rows[:, 0], rows[:, 1] = (yr < yo).sum(axis=1), (yr == yo).sum(axis=1)
        rows[:, 2], rscale[:, 2] = yr.sum(axis=1), np.abs(yr).sum(axis=1)
        rows[:, 3], rscale[:, 3] = (yr * yr).sum(axis=1), (yr * yr).sum(axis=1)
    return stats, obs, rows, sscale, rscale


def pool(stats, obs):
    """engine.ppc written out on [P, S, 8] and [P, 8] (no NaN replicates): the dict of (T(y), T(y_rep_s), p)."""
    st, ob = np.asarray(stats, np.float64), np.asarray(obs, np.float64)
    S = st.shape[1]
    tot, to = st.sum(axis=0), ob.sum(axis=0)
    tot[:, 2], tot[:, 3], to[2], to[3] = st[:, :, 2].max(axis=0), st[:, :, 3].min(axis=0), ob[:, 2].max(), ob[:, 3].min()
    n = to[5]

    def T(t):
        var = (t[..., 1] - t[..., 0] ** 2 / n) / (n - 1)
        return {"mean": t[..., 0] / n, "sd": np.sqrt(np.maximum(var, 0)), "max": t[..., 2], "min": t[..., 3],
                "frac_zero": t[..., 4] / n}
    To, Tr = T(to), T(tot)
    out = {k: {"obs": float(To[k]), "rep": Tr[k], "p": float((Tr[k] >= To[k]).sum()) / S} for k in To}
    out["chi2"] = {"obs": tot[:, 6], "rep": tot[:, 5], "p": float((tot[:, 5] >= tot[:, 6]).sum()) / S}
    return out
