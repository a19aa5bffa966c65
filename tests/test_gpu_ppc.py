"""The posterior predictive sweep (stk_posterior_predict, csrc/ppc.hip) on the GPU.

Replicates are checked against the host twin (stk_yrep_host) fed with eta computed in long double: they must be
equal wherever the twin's margin is at least 1e-10 (tests/test_host_ppc.py has the definition), and at most 1e-4
of a case's elements may be below it (linear: within 1e-10 of |eta| + sigma |z|).  stats, rows and obs are checked
against a long-double restatement computed from the DEVICE's own replicates: counts, extrema and integer sums
exactly, the Pearson discrepancies and the linear sums within BAR = 1e-10 of the sum of their absolute terms --
the bar of tests/test_gpu_predictive.py."""
import ctypes
import math

import numpy as np
import pytest

import ppc_ref as R

pytestmark = pytest.mark.gpu

BAR = 1e-10
FAMILIES = R.FAMILIES
DS = (1, 3, 4, 5, 100, 128)
NS = (1, 15, 17, 64, 65, 257, 513)
SS = (1, 15, 16, 17, 33, 100)
SEED = 77


def draws_near(rng, truth, S, sd=0.1):
    return truth[None, :] + sd * rng.normal(size=(S, truth.size))


def multi_chunk_n(d, S):
    """The smallest n of at least 3 chunks whose last 16-row tile is ragged, from the launch info."""
    from stark_amd import engine
    n = 17
    while engine.ppc_launch(n, d, S)["G"] < 3 or n % 16 == 0:
        n += 101
    return n


def shapes():
    out = [(37 + d % 7, d, 33) for d in DS]
    out += [(n, 100, 33) for n in NS] + [(None, 100, 33)]
    out += [(65, 17, S) for S in SS]
    return out


def twin(family, X, Q, seed, stream, draw0=0):
    """The twin's replicates [S, n] and margins on eta formed in long double."""
    from stark_amd import engine
    eta = R.eta_ld(X, Q).astype(np.float64)
    u = Q[:, -1] if family == "linear" else None
    y, mg = engine.yrep_host(family, seed, stream, 0, draw0, eta, u=u, margin=True)
    return y.T, mg.T, eta.T


def check_shard(family, X, y, Q, seed, stream, stats, obs, rows, yrep, draw0=0):
    """Every output of one shard; returns the largest errors in units of the bar."""
    n, S = X.shape[0], Q.shape[0]
    assert stats.shape == (S, 8) and obs.shape == (8,) and yrep.shape == (S, n)
    ty, mg, eta = twin(family, X, Q, seed, stream, draw0)
    err = {}
    if family == "linear":
        sigma = np.exp(Q[:, -1])[:, None]
        scale = np.maximum(1.0, np.abs(eta) + np.abs(ty - eta)) + 0 * sigma
        err["yrep"] = float((np.abs(yrep - ty) / (BAR * scale)).max())
    else:
        fragile = mg < R.FRAGILE
        assert fragile.sum() <= 1e-4 * fragile.size, (int(fragile.sum()), fragile.size)
        diff = (yrep != ty) & ~fragile
        assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4], yrep[diff][:4], ty[diff][:4], mg[diff][:4])
        err["yrep"] = 0.0
    rs, ro, rr, sscale, rscale = R.restate(family, X, y, Q, yrep)
    exact_s = (2, 3, 4, 7) if family == "linear" else (0, 1, 2, 3, 4, 7)
    for k in exact_s:
        assert np.array_equal(stats[:, k], rs[:, k].astype(np.float64)), (k, stats[:4, k], rs[:4, k])
    for k in (0, 1, 5, 6):
        if k in exact_s:
            continue
        e = np.abs(stats[:, k] - rs[:, k]) / (BAR * np.maximum(sscale[:, k], np.finfo(float).tiny))
        err[f"stats{k}"] = float(e.max())
    ex_o = (2, 3, 4, 5, 6, 7) if family == "linear" else range(8)
    for k in ex_o:
        assert obs[k] == float(ro[k]), (k, obs, ro)
    if family == "linear":
        for k in (0, 1):
            sc = float(np.abs(np.asarray(y, R.L) ** (k + 1)).sum())
            err[f"obs{k}"] = float(abs(obs[k] - ro[k]) / (BAR * max(sc, 1e-300)))
    if rows is not None:
        cols = [rows[k] for k in ("n_less", "n_equal", "sum", "sum_sq")]
        exact_r = (0, 1) if family == "linear" else (0, 1, 2, 3)
        for k in range(4):
            if k in exact_r:
                assert np.array_equal(cols[k], rr[:, k].astype(np.float64)), (k, cols[k][:4], rr[:4, k])
            else:
                e = np.abs(cols[k] - rr[:, k]) / (BAR * np.maximum(rscale[:, k], np.finfo(float).tiny))
                err[f"rows{k}"] = float(e.max())
    return err


@pytest.mark.parametrize("n,d,S", shapes())
@pytest.mark.parametrize("family", FAMILIES)
def test_values_match_the_twin_and_the_restatement(ctx, family, n, d, S):
    """Two shards in one grouped launch (the first a third of the rows), streams 7 and 2, draws = truth + N(0, 0.1)."""
    from stark_amd import engine
    if n is None:
        n = multi_chunk_n(d, S)
    rng, X, y, truth = R.make_data(family, n + n // 3 + 1, d, 1000 + 7 * d + n)
    Q = np.ascontiguousarray(draws_near(rng, truth, S))
    cut = n // 3 + 1
    parts = [(X[:cut], y[:cut]), (X[cut:], y[cut:])]
    m = engine.Model(ctx, family, [{"x": a, "y": b} for a, b in parts])
    try:
        stats, obs, rows, yrep = m.posterior_predict(Q, seed=SEED, streams=[7, 2], rows=True, yrep=True)
        s2, o2 = m.posterior_predict(Q, seed=SEED, streams=[7, 2])          # the stats-only kernel: the same bits
        assert np.array_equal(stats, s2, equal_nan=True) and np.array_equal(obs, o2)
    finally:
        m.close()
    off = 0
    for k, (a, b) in enumerate(parts):
        sl = slice(off, off + a.shape[0])
        err = check_shard(family, a, b, Q, SEED, (7, 2)[k], stats[k], obs[k], {c: v[sl] for c, v in rows.items()},
                          yrep[:, sl])
        off += a.shape[0]
        print(f"{family} n={a.shape[0]} d={d} S={S}: largest errors / bar {err}")
        assert all(v <= 1.0 for v in err.values()), err


@pytest.mark.parametrize("family", FAMILIES)
def test_outputs_carry_the_same_bits_anywhere(ctx, family):
    """A shard alone and inside a 3-shard grouped launch; q[a:b] with draw0 = a against all of q; a row's outputs
    at two shard lengths; seeds and streams change the replicates."""
    from stark_amd import engine
    d, S = 17, 45
    n = multi_chunk_n(d, S)
    rng, X, y, truth = R.make_data(family, n + 100, d, 5)
    Q = np.ascontiguousarray(draws_near(rng, truth, S))
    sh = lambda lo, hi: {"x": X[lo:hi], "y": y[lo:hi]}
    m1 = engine.Model(ctx, family, [sh(0, n)])
    m3 = engine.Model(ctx, family, [sh(n, n + 37), sh(n + 37, n + 100), sh(0, n)])
    ms = engine.Model(ctx, family, [sh(0, 83)])
    try:
        a = m1.posterior_predict(Q, 0, seed=SEED, streams=[9], rows=True, yrep=True)
        b = m3.posterior_predict(Q, seed=SEED, streams=[1, 2, 9], rows=True, yrep=True)
        assert np.array_equal(a[0], b[0][2], equal_nan=True) and np.array_equal(a[1], b[1][2])
        assert all(np.array_equal(a[2][k], b[2][k][100:]) for k in a[2]) and np.array_equal(a[3], b[3][:, 100:])
        c = m3.posterior_predict(Q, 2, seed=SEED, streams=[9])
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
        # a window of the draws
        lo, hi = 5, 39
        w = m1.posterior_predict(Q[lo:hi], 0, seed=SEED, draw0=lo, streams=[9], yrep=True)
        assert np.array_equal(w[0], a[0][lo:hi]) and np.array_equal(w[2], a[3][lo:hi]) and np.array_equal(w[1], a[1])
        w0 = m1.posterior_predict(Q[lo:hi], 0, seed=SEED, draw0=0, streams=[9], yrep=True)
        assert not np.array_equal(w0[2], w[2])
        # the first 83 rows as a shard of their own: per-row outputs and replicates are the same
        s = ms.posterior_predict(Q, 0, seed=SEED, streams=[9], rows=True, yrep=True)
        assert all(np.array_equal(s[2][k], a[2][k][:83]) for k in a[2]) and np.array_equal(s[3], a[3][:, :83])
        # seeds and streams
        for kw in (dict(seed=SEED + 1, streams=[9]), dict(seed=SEED, streams=[10])):
            o = m1.posterior_predict(Q, 0, yrep=True, **kw)
            assert not np.array_equal(o[2], a[3]) and np.array_equal(o[1], a[1])
        assert np.array_equal(m1.posterior_predict(Q, 0, seed=SEED, yrep=True)[2],
                              m1.posterior_predict(Q, 0, seed=SEED, streams=[0], yrep=True)[2])
    finally:
        m1.close()
        m3.close()
        ms.close()


def test_nan_draw_touches_no_other(ctx):
    from stark_amd import engine
    n, d, S = 131, 5, 20
    rng, X, y, truth = R.make_data("logistic", n, d, 3)
    Q = np.ascontiguousarray(draws_near(rng, truth, S))
    Qn = Q.copy()
    Qn[6, 2] = np.nan
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        a = m.posterior_predict(Q, 0, seed=SEED, rows=True, yrep=True)
        b = m.posterior_predict(Qn, 0, seed=SEED, rows=True, yrep=True)
    finally:
        m.close()
    keep = np.arange(S) != 6
    assert np.array_equal(a[0][keep], b[0][keep]) and np.array_equal(a[3][keep], b[3][keep])
    assert np.all(np.isnan(b[0][6, [0, 1, 2, 3, 5]])) and b[0][6, 7] == n and b[0][6, 4] == 0
    assert np.all(np.isnan(b[3][6]))
    zero = X[n // 2]                                   # the all-zero row has a finite eta = alpha even so
    assert not zero.any()
    assert np.all(np.isnan(b[2]["sum"])) and np.all(np.isnan(b[2]["sum_sq"]))
    yr = np.delete(b[3], 6, axis=0)
    assert np.array_equal(b[2]["n_less"], (yr < y[None, :]).sum(axis=0))
    assert np.array_equal(b[2]["n_equal"], (yr == y[None, :]).sum(axis=0))
    assert engine.ppc(b[0], b[1])["n_non_finite"] == n


def test_poisson_extremes(ctx):
    """eta = 800 (mu = inf): NaN replicates; eta = -800: y_rep = 0 and a discrepancy term of 0 where y = 0."""
    from stark_amd import engine
    n, d = 70, 3
    X = np.zeros((n, d))
    y = np.zeros(n, np.int32)
    Q = np.zeros((3, d + 1))
    Q[:, 0] = [800.0, -800.0, 0.5]
    m = engine.Model(ctx, "poisson", [{"x": X, "y": y}])
    try:
        stats, obs, yrep = m.posterior_predict(Q, 0, seed=SEED, yrep=True)
    finally:
        m.close()
    assert np.all(np.isnan(yrep[0])) and stats[0, 7] == n and np.all(np.isnan(stats[0, [0, 1, 2, 3, 5]]))
    assert np.all(yrep[1] == 0) and np.array_equal(stats[1], [0, 0, 0, 0, n, 0, 0, 0])
    assert stats[2, 7] == 0 and np.isfinite(stats[2]).all() and abs(stats[2, 6] - n * math.exp(0.5)) <= 1e-9 * n
    assert np.array_equal(obs, [0, 0, 0, 0, n, n, 0, 0])


def test_logistic_extremes(ctx):
    """|eta| = 800: g is 0 or 1 and V = 0; the replicate is the point mass, D(y_rep) = 0, and D(y) is 0 where every y
    sits on it and +inf otherwise."""
    from stark_amd import engine
    n, d = 40, 2
    X = np.zeros((n, d))
    Q = np.zeros((2, d + 1))
    Q[:, 0] = [800.0, -800.0]
    for yval in (0, 1):
        m = engine.Model(ctx, "logistic", [{"x": X, "y": np.full(n, yval, np.int32)}])
        try:
            stats, obs, yrep = m.posterior_predict(Q, 0, seed=SEED, yrep=True)
        finally:
            m.close()
        assert np.all(yrep[0] == 1) and np.all(yrep[1] == 0)
        assert np.array_equal(stats[:, 5], [0, 0]) and np.array_equal(stats[:, 7], [0, 0])
        assert np.array_equal(stats[:, 6], [np.inf, 0] if yval == 0 else [0, np.inf])
        assert np.isfinite(stats[:, :5]).all() and np.array_equal(stats[:, 0], [n, 0])


@pytest.mark.parametrize("n", [17, 65])
def test_no_write_outside_the_outputs(ctx, n):
    """Through ctypes, every output inside a larger buffer of a sentinel: nothing outside it changes."""
    from stark_amd import _lib, engine
    d, S, pad, sentinel = 5, 17, 64, -7.25
    rng, X, y, truth = R.make_data("logistic", n, d, 2)
    Q = np.ascontiguousarray(draws_near(rng, truth, S))
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        sizes = (8 * S, 8, 4 * n, n * S)
        bufs = [np.full(pad + k + pad, sentinel) for k in sizes]
        at = [ctypes.c_void_p(b.ctypes.data + 8 * pad) for b in bufs]
        _lib.check(_lib.load().stk_posterior_predict(m._h, 0, Q.ctypes.data, S, 0, SEED, None, *at))
        for buf, k in zip(bufs, sizes):
            assert np.all(buf[:pad] == sentinel) and np.all(buf[pad + k:] == sentinel)
            assert np.all(buf[pad:pad + k] != sentinel)
        stats, obs, rows, yrep = m.posterior_predict(Q, 0, seed=SEED, rows=True, yrep=True)
        assert np.array_equal(bufs[0][pad:pad + 8 * S].reshape(S, 8), stats) and np.array_equal(bufs[1][pad:pad + 8], obs)
        assert np.array_equal(bufs[2][pad:pad + 4 * n].reshape(n, 4)[:, 2], rows["sum"])
        assert np.array_equal(bufs[3][pad:pad + n * S].reshape(n, S).T, yrep)
        # stats alone
        sb = np.full(pad + 8 * S + pad, sentinel)
        _lib.check(_lib.load().stk_posterior_predict(m._h, 0, Q.ctypes.data, S, 0, SEED, None,
                                                     ctypes.c_void_p(sb.ctypes.data + 8 * pad), None, None, None))
        assert np.array_equal(sb, bufs[0])
    finally:
        m.close()


def test_device_outputs_are_written_in_place(ctx):
    import torch
    from stark_amd import _lib, engine
    n, d, S = 65, 5, 17
    rng, X, y, truth = R.make_data("poisson", n, d, 4)
    Q = np.ascontiguousarray(draws_near(rng, truth, S))
    m = engine.Model(ctx, "poisson", [{"x": X, "y": y}])
    try:
        dev = f"cuda:{ctx.device}"
        tr = torch.full((n + 2, 4), -7.25, dtype=torch.float64, device=dev)
        ty = torch.full((n + 2, S), -7.25, dtype=torch.float64, device=dev)
        ts = torch.full((S + 2, 8), -7.25, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        _lib.check(_lib.load().stk_posterior_predict(m._h, 0, Q.ctypes.data, S, 0, SEED, None,
                                                     ctypes.c_void_p(ts.data_ptr() + 64), None,
                                                     ctypes.c_void_p(tr.data_ptr() + 32), ctypes.c_void_p(ty.data_ptr() + 8 * S)))
        hr, hy, hs = tr.cpu().numpy(), ty.cpu().numpy(), ts.cpu().numpy()
        stats, obs, rows, yrep = m.posterior_predict(Q, 0, seed=SEED, rows=True, yrep=True)
        for h in (hr, hy, hs):
            assert np.all(h[0] == -7.25) and np.all(h[-1] == -7.25)
        assert np.array_equal(hr[1:-1, 0], rows["n_less"]) and np.array_equal(hr[1:-1, 3], rows["sum_sq"])
        assert np.array_equal(hy[1:-1].T, yrep) and np.array_equal(hs[1:-1], stats)
    finally:
        m.close()


def test_refusals_name_the_family_or_the_limit(ctx):
    from stark_amd import _lib, engine
    from stark_amd._lib import StarkHipError
    m = engine.Model(ctx, "schools", [{"y": [28.0, 8.0, -3.0], "sigma": [15.0, 10.0, 16.0]}])
    try:
        with pytest.raises(StarkHipError, match="schools") as e:
            m.posterior_predict(np.zeros((4, m.D[0])), 0)
        assert e.value.code == -1
    finally:
        m.close()
    rng = np.random.default_rng(3)
    m = engine.Model(ctx, "logistic", [{"x": rng.normal(size=(20, 129)), "y": rng.integers(0, 2, 20)}])
    try:
        with pytest.raises(StarkHipError, match="d = 129") as e:
            m.posterior_predict(np.zeros((4, 130)), 0)
        assert e.value.code == -1
    finally:
        m.close()
    m = engine.Model(ctx, "logistic", [{"x": rng.normal(size=(20, 5)), "y": rng.integers(0, 2, 20)}])
    try:
        q, st = np.zeros((4, 6)), np.zeros((4, 8))
        with pytest.raises(StarkHipError, match="2\\^24"):
            m.posterior_predict(q, 0, draw0=2 ** 24 - 3)
        with pytest.raises(StarkHipError, match="draw0 = -1"):
            m.posterior_predict(q, 0, draw0=-1)
        with pytest.raises(StarkHipError, match="stream = 1048576"):
            m.posterior_predict(q, 0, streams=[2 ** 20])
        assert m.posterior_predict(q, 0, draw0=2 ** 24 - 4, streams=[2 ** 20 - 1])[0].shape == (4, 8)
        fn = _lib.load().stk_posterior_predict
        for args, word in (((m._h, 0, q.ctypes.data, 0, 0, 1, None, st.ctypes.data, None, None, None), "S = 0"),
                           ((m._h, 0, q.ctypes.data, 4, 0, 1, None, None, None, None, None), "stats"),
                           ((m._h, 0, None, 4, 0, 1, None, st.ctypes.data, None, None, None), "q is NULL")):
            assert fn(*args) == -1
            msg = _lib.load().stk_last_error().decode()
            assert word in msg and ("logistic" in msg or "d = 5" in msg), msg
    finally:
        m.close()


# ---------------------------------------------------------------- the driver
PARTS = (200, 333, 64)
DRIVER_S, DRIVER_SEED = 256, 12


def driver_case(kind):
    """Rows, the P x S sample matrix and the family of a driver case: "logistic" and "poisson" are well specified
    (data from the model, draws = truth + the Laplace sd), "overdispersed" is a Poisson fit to counts of the same
    mean and four times the variance (negative binomial, made here)."""
    family = "logistic" if kind == "logistic" else "poisson"
    n, d = sum(PARTS), 5
    rng, X, y, truth = R.make_data(family, n, d, 21)
    mu = np.exp(truth[0] + X @ truth[1:])
    if kind == "overdispersed":
        y = rng.negative_binomial(mu / 3.0, 0.25).astype(np.int32)      # mean mu, variance 4 mu
    Xt = np.hstack([np.ones((n, 1)), X])
    w = mu if family == "poisson" else (1 / (1 + 1 / mu)) * (1 / (1 + mu))
    cov = np.linalg.inv((Xt * w[:, None]).T @ Xt)
    Q = truth[None, :] + rng.multivariate_normal(np.zeros(d + 1), cov, DRIVER_S)
    return family, X, y, Q


def host_ppc(family, X, y, Q, seed):
    """The driver's result from the twin and the restatement: partition p has stream p; pooled in partition order."""
    cuts = np.concatenate([[0], np.cumsum(PARTS)])
    stats, obs, fragile = [], [], 0
    for p in range(len(PARTS)):
        a, b = X[cuts[p]:cuts[p + 1]], y[cuts[p]:cuts[p + 1]]
        ty, mg, _ = twin(family, a, Q, seed, p)
        fragile += int((mg < R.FRAGILE).sum())
        rs, ro, *_ = R.restate(family, a, b, Q, ty)
        stats.append(rs.astype(np.float64))
        obs.append(ro.astype(np.float64))
    return np.array(stats), np.array(obs), fragile


def _driver(family, rows):
    import os
    from conftest import ROOT
    from stark_amd import stark
    from stark_amd.rdd import LocalContext, LocalRDD

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": 5, "x": a[:, :5], "y": a[:, 5].astype(np.int64)}

    cuts = np.concatenate([[0], np.cumsum(PARTS)])
    rdd = LocalRDD([rows[cuts[i]:cuts[i + 1]] for i in range(len(PARTS))])
    st = stark.Stark(LocalContext(), rdd, prep)
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", f"{family}.stan"))
    return st


@pytest.mark.parametrize("kind", ["logistic", "poisson", "overdispersed"])
def test_driver_ppc(ctx, kind):
    """Stark.ppc over 3 partitions (n = 200, 333, 64; d = 5; S = 256) equals engine.ppc of the restatement's pooled
    arrays.  A well-specified fit has every p-value in (0.01, 0.99); the Poisson fit to overdispersed counts has
    chi2 and sd p-values below 0.01."""
    from stark_amd import engine
    family, X, y, Q = driver_case(kind)
    n, S = X.shape[0], Q.shape[0]
    hs, ho, fragile = host_ppc(family, X, y, Q, DRIVER_SEED)
    assert fragile == 0                                      # so the device's replicates ARE the twin's
    ref = engine.ppc(hs, ho)
    hand = R.pool(hs, ho)
    rows = [tuple(X[i]) + (int(y[i]),) for i in range(n)]
    samples = np.vstack([Q.T, np.zeros((1, S))])              # P x S with an lp__ row
    out = _driver(family, rows).ppc(samples, seed=DRIVER_SEED)
    assert out["n"] == n and out["n_non_finite"] == 0
    assert out["partition_stats"].shape == (3, S, 8) and out["partition_obs"].shape == (3, 8)
    assert [int(v) for v in out["partition_obs"][:, 5]] == list(PARTS)
    for k in engine.PPC_STATS:
        assert out[k]["obs"] == ref[k]["obs"] and np.array_equal(out[k]["rep"], ref[k]["rep"]), k
        assert out[k]["p"] == ref[k]["p"] == hand[k]["p"], (k, out[k]["p"], ref[k]["p"])
    scale = np.abs(ref["chi2"]["rep"]) + np.abs(ref["chi2"]["obs"])
    for k in ("rep", "obs"):
        assert np.all(np.abs(out["chi2"][k] - ref["chi2"][k]) <= BAR * scale), k
    assert out["chi2"]["p"] == ref["chi2"]["p"]
    ps = {k: out[k]["p"] for k in engine.PPC_STATS + ("chi2",)}
    print(kind, ps)
    if kind == "overdispersed":
        assert ps["chi2"] < 0.01 and ps["sd"] < 0.01, ps
    else:
        # With counts, a statistic that sits at the lower end of its range in the data has p = 1 by the ">=" of the
        # definition, whatever the fit: max and min of binary data (1 and 0 in the data and in every replicate)
        # and the minimum 0 of these Poisson counts.  Those are asserted to BE 1; every other p-value is inside.
        pinned = ("max", "min") if family == "logistic" else ("min",)
        assert out["min"]["obs"] == 0 and all(ps[k] == 1.0 for k in pinned), ps
        assert all(0.01 < v < 0.99 for k, v in ps.items() if k not in pinned), ps
