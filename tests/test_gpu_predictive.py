"""The pointwise log-predictive sweep (stk_log_predictive, predictive.hip) against a numpy restatement of
the definitions in np.longdouble, for the three regression families.

With eta_is = alpha_s + x_i . beta_s (draw s, row i):
    logistic  z = (2 y - 1) eta, ll = min(z, 0) - log1p(exp(-|z|)),        g = 1 / (1 + exp(-eta))
    poisson   ll = y eta - exp(eta) - lgamma(y + 1),                        g = exp(eta)
    linear    r = y - eta, ll = -log(2 pi)/2 - u_s - r^2 e^{-2 u_s} / 2,    g = eta
    per row   lppd = logsumexp_s ll - log S, mean = sum ll / S, var = the sample variance (0 at S = 1),
              mu = sum g / S, elpd = lppd - var
    totals    n, sum lppd, sum var, sum elpd, sum elpd^2, #(var > 0.4), #(a non-finite statistic), 0
lgamma(y + 1) is a longdouble sum of logs.  The bars are the project's density bar, 1e-10: with
scale_i = max(1, max_s |ll_is|), lppd and mean within 1e-10 scale_i, var within 1e-10 scale_i^2, mu within
1e-10 max(1, |mu_i|), every total within 1e-10 max(1, sum_i |term_i|).  Every case prints its largest
error, in units of its bar, as a MAXERR line.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 1e-10
DBL_MAX = np.finfo(np.float64).max
FAMILIES = ("logistic", "poisson", "linear")
DS = (1, 3, 4, 5, 15, 16, 17, 100, 127, 128)
NS = (1, 15, 16, 17, 63, 64, 65, 333)
SS = (1, 2, 15, 16, 17, 33, 64)
L = np.longdouble


def make_data(family, n, d, seed=None):
    """X ~ U(-1.7, 1.7) with one all-zero row (n >= 3); y from the family at a true (alpha, beta[, sigma])."""
    rng = np.random.default_rng(1000 * n + d if seed is None else seed)
    X = rng.uniform(-1.7, 1.7, (n, d))
    if n >= 3:
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
    return rng, X, y, truth


def draws_near(rng, truth, S, sd=0.1):
    return truth[None, :] + rng.normal(0, sd, (S, truth.size))


def ref_ll(family, X, y, Q):
    """ll [n, S] and g [n, S] in longdouble; an exp past the largest double is +inf, as in fp64."""
    d = X.shape[1]
    Xl, Ql, yl = X.astype(L), np.asarray(Q).astype(L), np.asarray(y).astype(L)[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        eta = Ql[:, 0][None, :] + Xl @ Ql[:, 1:d + 1].T
        if family == "logistic":
            z = (2 * yl - 1) * eta
            ll = np.minimum(z, 0) - np.log1p(np.exp(-np.abs(z)))
            ex = np.exp(-eta)
            ex[ex > DBL_MAX] = np.inf
            g = 1 / (1 + ex)
        elif family == "poisson":
            lg = np.array([np.log(np.arange(1, int(v) + 1).astype(L)).sum() if v > 0 else L(0) for v in np.asarray(y)], L)
            g = np.exp(eta)
            g[g > DBL_MAX] = np.inf
            ll = yl * eta - g - lg[:, None]
        else:
            u = Ql[:, -1][None, :]
            r = yl - eta
            ll = -L(0.5) * np.log(2 * L(np.pi)) - u - L(0.5) * r * r * np.exp(-2 * u)
            g = eta
    return ll, g


def ref_stats(family, X, y, Q):
    """{lppd, mean, var, mu, scale} per row (float64; the statistics from longdouble) and the [8] totals."""
    ll, g = ref_ll(family, X, y, Q)
    n, S = ll.shape
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        M = ll.max(axis=1)                                  # NaN if any NaN
        Ms = np.where(np.isfinite(M), M, 0)
        lse = Ms + np.log(np.exp(ll - Ms[:, None]).sum(axis=1))
        lppd = np.where(M == -np.inf, -np.inf, lse) - np.log(L(S))
        mean = ll.sum(axis=1) / S
        if S > 1:
            var = ((ll - mean[:, None]) ** 2).sum(axis=1) / (S - 1)
        else:
            var = np.where(np.isnan(ll[:, 0]), np.nan, 0).astype(L)
        mu = g.sum(axis=1) / S
        fin = np.where(np.isfinite(ll), np.abs(ll), 0)
        scale = np.maximum(1, fin.max(axis=1)).astype(np.float64)
        elpd = lppd - var
        bad = ~(np.isfinite(lppd) & np.isfinite(mean) & np.isfinite(var) & np.isfinite(mu))
        tot = np.array([n, lppd.sum(), var.sum(), elpd.sum(), (elpd * elpd).sum(), (var > 0.4).sum(), bad.sum(), 0], L)
        tscale = np.array([1, np.abs(lppd).sum(), np.abs(var).sum(), np.abs(elpd).sum(), (elpd * elpd).sum(), 0, 0, 0], L)
    rows = {k: v.astype(np.float64) for k, v in (("lppd", lppd), ("mean", mean), ("var", var), ("mu", mu))}
    rows["scale"] = scale
    return rows, tot.astype(np.float64), np.maximum(1, np.where(np.isfinite(tscale), tscale, 0)).astype(np.float64)


def same_class(a, b):
    """Non-finite entries agree exactly (NaN with NaN, each infinity with itself)."""
    a, b = np.asarray(a), np.asarray(b)
    nf = ~np.isfinite(b)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[nf & ~np.isnan(b)], b[nf & ~np.isnan(b)])
                and np.isfinite(a[~nf]).all())


def row_errors(rows, ref):
    """The largest error of each statistic in units of its bar (<= 1 passes); non-finite entries must agree."""
    sc = ref["scale"]
    bars = {"lppd": BAR * sc, "mean": BAR * sc, "var": BAR * sc * sc, "mu": BAR * np.maximum(1, np.abs(ref["mu"]))}
    worst = 0.0
    for k, bar in bars.items():
        assert same_class(rows[k], ref[k]), k
        f = np.isfinite(ref[k])
        if f.any():
            worst = max(worst, float((np.abs(rows[k][f] - ref[k][f]) / np.where(np.isfinite(bar[f]), bar[f], 1)).max()))
    return worst


def total_errors(tot, rtot, tscale):
    assert same_class(tot, rtot)
    f = np.isfinite(rtot)
    assert tot[0] == rtot[0] and tot[5] == rtot[5] and tot[6] == rtot[6] and tot[7] == 0
    return float((np.abs(tot[f] - rtot[f]) / (BAR * tscale[f])).max())


def multi_chunk_n(d, S):
    """The smallest n of at least 3 chunks whose last 16-row tile is ragged, from the launch info."""
    from stark_amd import engine
    n = 17
    while engine.predictive_launch(n, d, S)["G"] < 3 or n % 16 == 0:
        n += 101
    return n


def shapes():
    out = [(37 + d % 7, d, 33) for d in DS]
    out += [(n, 100, 33) for n in NS] + [(None, 100, 33)]
    out += [(65, 17, S) for S in SS]
    return out


@pytest.mark.parametrize("n,d,S", shapes())
@pytest.mark.parametrize("family", FAMILIES)
def test_rows_and_totals_match_the_restatement(ctx, family, n, d, S):
    """Two shards (the first a third of the rows; the second is checked), draws = truth + N(0, 0.1)."""
    from stark_amd import engine
    if n is None:
        n = multi_chunk_n(d, S)
        info = engine.predictive_launch(n, d, S)
        assert info["G"] >= 3 and n % info["T"] != 0
    rng, X, y, truth = make_data(family, n, d)
    Q = draws_near(rng, truth, S)
    k = max(1, n // 3)
    m = engine.Model(ctx, family, [{"x": X[:k], "y": y[:k]}, {"x": X, "y": y}])
    try:
        tot, rows = m.log_predictive(Q, 1, rows=True)
        ref, rtot, tscale = ref_stats(family, X, y, Q)
        assert all(np.isfinite(v).all() for v in rows.values()) and np.isfinite(tot).all()
        e_rows, e_tot = row_errors(rows, ref), total_errors(tot, rtot, tscale)
        print(f"MAXERR predictive[{family}-{n}-{d}-{S}] rows {e_rows:.3e} totals {e_tot:.3e} (units of the 1e-10 bars)")
        assert e_rows <= 1 and e_tot <= 1, (family, n, d, S, e_rows, e_tot)
        assert np.array_equal(m.log_predictive(Q, 1), tot)             # rows = NULL changes no total
    finally:
        m.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_one_draw_is_the_oracle_log_density(ctx, orc, family):
    """S = 1: sum_i lppd_i is oracle.Model.lpgrad's lp with flat priors, after the constants the
    definitions add back (linear: lp - u - (n/2) log 2 pi; poisson: lp - sum lgamma(y + 1), with lp from
    the restatement of the Poisson tests: sum y eta - exp(eta)); within 1e-10 relative."""
    from stark_amd import engine
    n, d = 333, 17
    rng, X, y, truth = make_data(family, n, d)
    q = draws_near(rng, truth, 1)
    m = engine.Model(ctx, family, [{"x": X, "y": y}])
    try:
        tot, rows = m.log_predictive(q, 0, rows=True)
    finally:
        m.close()
    if family == "logistic":
        want = orc.Model(orc.FAM_LOGREG, X=X, y=y).lpgrad(q[0])[0]
    elif family == "linear":
        want = orc.Model(orc.FAM_LINREG, X=X, y=y).lpgrad(q[0])[0] - q[0, -1] - 0.5 * n * np.log(2 * np.pi)
    else:
        eta = q[0, 0].astype(L) + X.astype(L) @ q[0, 1:].astype(L)
        lg = sum(np.log(np.arange(1, int(v) + 1).astype(L)).sum() for v in y)
        want = float((y.astype(L) * eta - np.exp(eta)).sum() - lg)
    err = abs(tot[1] - want) / abs(want)
    print(f"MAXERR predictive_oracle[{family}] {err:.3e}")
    assert err < BAR
    assert tot[2] == 0 and np.all(rows["var"] == 0) and np.array_equal(rows["lppd"], rows["mean"])
    assert tot[3] == tot[1]


def test_logistic_extreme_eta_is_finite_and_right(ctx):
    """Rows with eta = +-40, +-750 and 745 (every draw the same point, plus one ordinary draw)."""
    from stark_amd import engine
    n, d, S = 70, 100, 17
    rng, X, y, truth = make_data("logistic", n, d)
    q = rng.normal(0, 0.3, d + 1)
    b = q[1:]
    for row, eta in ((1, 40.0), (2, -40.0), (3, 750.0), (4, -750.0), (20, 745.0)):
        X[row] = (eta - q[0]) * b / (b @ b)
    Q = np.tile(q, (S, 1))
    Q[-1] = truth
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        tot, rows = m.log_predictive(Q, 0, rows=True)
    finally:
        m.close()
    ref, rtot, tscale = ref_stats("logistic", X, y, Q)
    assert all(np.isfinite(v).all() for v in rows.values()) and np.isfinite(tot).all() and tot[6] == 0
    e_rows, e_tot = row_errors(rows, ref), total_errors(tot, rtot, tscale)
    print(f"MAXERR predictive[logistic-extreme-eta] rows {e_rows:.3e} totals {e_tot:.3e}")
    assert e_rows <= 1 and e_tot <= 1


def test_poisson_overflow_and_nan_propagate(ctx):
    """One draw whose alpha is 800: that draw is -inf in every row, the lppd stays finite and right, the
    mean is -inf and the var NaN.  Every draw overflowing: lppd -inf, never NaN, never finite.  One NaN
    coordinate in one draw: every row NaN and totals[6] == n -- for the three families."""
    from stark_amd import engine
    n, d, S = 40, 5, 20
    for family in FAMILIES:
        rng, X, y, truth = make_data(family, n, d)
        Q = draws_near(rng, truth, S)
        m = engine.Model(ctx, family, [{"x": X, "y": y}])
        try:
            if family == "poisson":
                one = Q.copy()
                one[7, 0] = 800.0
                tot, rows = m.log_predictive(one, 0, rows=True)
                ref, rtot, tscale = ref_stats(family, X, y, one)
                assert np.isfinite(rows["lppd"]).all() and np.all(rows["mean"] == -np.inf) and np.isnan(rows["var"]).all()
                assert np.all(rows["mu"] == np.inf) and tot[6] == n
                e = row_errors(rows, ref)
                print(f"MAXERR predictive[poisson-one-overflowing-draw] rows {e:.3e}")
                assert e <= 1 and same_class(tot, rtot)
                assert abs(tot[1] - rtot[1]) <= BAR * tscale[1]
                every = Q.copy()
                every[:, 0] = 800.0
                tot, rows = m.log_predictive(every, 0, rows=True)
                assert np.all(rows["lppd"] == -np.inf) and np.all(rows["mean"] == -np.inf) and tot[1] == -np.inf
                assert tot[6] == n
            bad = Q.copy()
            bad[3, 1] = np.nan
            tot, rows = m.log_predictive(bad, 0, rows=True)
            assert all(np.isnan(rows[k]).all() for k in ("lppd", "mean", "var", "mu")), family
            assert tot[6] == n and tot[0] == n and np.isnan(tot[1:5]).all()
            ref, rtot, _ = ref_stats(family, X, y, bad)
            assert same_class(tot, rtot) and all(same_class(rows[k], ref[k]) for k in ("lppd", "mean", "var", "mu"))
        finally:
            m.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_rows_carry_the_same_bits_anywhere(ctx, family):
    """Rows 0 .. k - 1 of a shard equal the rows of a k-row shard with the same data; shard = -1 over 3
    shards of different n equals the three single calls, rows and totals, in either shard order."""
    from stark_amd import engine
    d, S = 17, 33
    parts, Xs = [], []
    for n in (37, multi_chunk_n(d, S), 600):
        rng, X, y, truth = make_data(family, n, d, seed=77 + n)
        parts.append({"x": X, "y": y})
    Q = draws_near(np.random.default_rng(5), truth, S, sd=0.3)
    keys = ("lppd", "mean", "var", "mu")
    m = engine.Model(ctx, family, parts)
    m2 = engine.Model(ctx, family, parts[::-1])
    k = 41
    mk = engine.Model(ctx, family, [{"x": parts[2]["x"][:k], "y": parts[2]["y"][:k]}])
    try:
        tot, rows = m.log_predictive(Q, None, rows=True)
        tot2, rows2 = m2.log_predictive(Q, None, rows=True)
        assert tot.shape == (3, 8) and rows["lppd"].shape == (sum(m.n_rows),)
        assert np.array_equal(tot2, tot[::-1])
        off = np.concatenate([[0], np.cumsum(m.n_rows)])
        off2 = np.concatenate([[0], np.cumsum(m2.n_rows)])
        for s in range(3):
            t1, r1 = m.log_predictive(Q, s, rows=True)
            assert np.array_equal(t1, tot[s], equal_nan=True)
            for key in keys:
                assert np.array_equal(r1[key], rows[key][off[s]:off[s + 1]])
                assert np.array_equal(r1[key], rows2[key][off2[2 - s]:off2[3 - s]])
            ref, rtot, tscale = ref_stats(family, parts[s]["x"], parts[s]["y"], Q)
            assert row_errors(r1, ref) <= 1 and total_errors(t1, rtot, tscale) <= 1
        _, rk = mk.log_predictive(Q, 0, rows=True)
        for key in keys:
            assert np.array_equal(rk[key], rows[key][off[2]:off[2] + k])
    finally:
        m.close()
        m2.close()
        mk.close()


@pytest.mark.parametrize("n", [17, 65])
def test_no_write_outside_the_outputs(ctx, n):
    """Through ctypes, rows and totals inside larger buffers of a sentinel: nothing outside [n][4] and
    [8] changes."""
    from stark_amd import _lib, engine
    d, S, pad, sentinel = 5, 17, 64, -7.25
    rng, X, y, truth = make_data("logistic", n, d)
    Q = np.ascontiguousarray(draws_near(rng, truth, S))
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        rbuf = np.full(pad + 4 * n + pad, sentinel)
        tbuf = np.full(pad + 8 + pad, sentinel)
        fn = _lib.load().stk_log_predictive
        _lib.check(fn(m._h, 0, Q.ctypes.data, S, ctypes.c_void_p(rbuf.ctypes.data + 8 * pad),
                      ctypes.c_void_p(tbuf.ctypes.data + 8 * pad)))
        for buf, k in ((rbuf, 4 * n), (tbuf, 8)):
            assert np.all(buf[:pad] == sentinel) and np.all(buf[pad + k:] == sentinel)
            assert np.all(buf[pad:pad + k] != sentinel)
        tot, rows = m.log_predictive(Q, 0, rows=True)
        assert np.array_equal(tbuf[pad:pad + 8], tot)
        assert np.array_equal(rbuf[pad:pad + 4 * n].reshape(n, 4)[:, 3], rows["mu"])
        # totals alone, rows alone
        tbuf[:] = sentinel
        _lib.check(fn(m._h, 0, Q.ctypes.data, S, None, ctypes.c_void_p(tbuf.ctypes.data + 8 * pad)))
        assert np.array_equal(tbuf[pad:pad + 8], tot) and np.all(tbuf[:pad] == sentinel) and np.all(tbuf[pad + 8:] == sentinel)
        r2 = np.full(4 * n, sentinel)
        _lib.check(fn(m._h, 0, Q.ctypes.data, S, r2.ctypes.data, None))
        assert np.array_equal(r2, rbuf[pad:pad + 4 * n])
    finally:
        m.close()


def test_device_rows_are_written_in_place(ctx):
    """rows as a device tensor: written where it lies, the same bits as the host copy."""
    import torch
    from stark_amd import _lib, engine
    n, d, S = 65, 5, 17
    rng, X, y, truth = make_data("poisson", n, d)
    Q = np.ascontiguousarray(draws_near(rng, truth, S))
    m = engine.Model(ctx, "poisson", [{"x": X, "y": y}])
    try:
        t = torch.full((n + 2, 4), -7.25, dtype=torch.float64, device=f"cuda:{ctx.device}")
        torch.cuda.synchronize()
        tot = np.empty(8)
        _lib.check(_lib.load().stk_log_predictive(m._h, 0, Q.ctypes.data, S, ctypes.c_void_p(t.data_ptr() + 32),
                                                  tot.ctypes.data))
        host = t.cpu().numpy()
        tot2, rows = m.log_predictive(Q, 0, rows=True)
        assert np.all(host[0] == -7.25) and np.all(host[-1] == -7.25)
        assert np.array_equal(host[1:-1, 0], rows["lppd"]) and np.array_equal(host[1:-1, 3], rows["mu"])
        assert np.array_equal(tot, tot2)
    finally:
        m.close()


def test_refusals_name_the_family_or_the_limit(ctx):
    from stark_amd import _lib, engine
    from stark_amd._lib import StarkHipError
    m = engine.Model(ctx, "schools", [{"y": [28.0, 8.0, -3.0], "sigma": [15.0, 10.0, 16.0]}])
    try:
        with pytest.raises(StarkHipError, match="schools") as e:
            m.log_predictive(np.zeros((4, m.D[0])), 0)
        assert e.value.code == -1
    finally:
        m.close()
    with pytest.raises(StarkHipError, match="d = 1025") as e:       # no model holds 1025 columns: the geometry refuses
        engine.predictive_launch(100, 1025, 16)
    assert e.value.code == -1
    rng = np.random.default_rng(3)
    m = engine.Model(ctx, "logistic", [{"x": rng.normal(size=(20, 129)), "y": rng.integers(0, 2, 20)}])
    try:
        with pytest.raises(StarkHipError, match="d = 129") as e:
            m.log_predictive(np.zeros((4, 130)), 0)
        assert e.value.code == -1
    finally:
        m.close()
    m = engine.Model(ctx, "logistic", [{"x": rng.normal(size=(20, 5)), "y": rng.integers(0, 2, 20)}])
    try:
        q, tot = np.zeros((4, 6)), np.zeros(8)
        fn = _lib.load().stk_log_predictive
        for args in ((m._h, 0, q.ctypes.data, 0, None, tot.ctypes.data),          # S = 0
                     (m._h, 0, q.ctypes.data, 4, None, None),                     # both outputs NULL
                     (m._h, 0, None, 4, None, tot.ctypes.data)):                  # q NULL
            assert fn(*args) == -1
            msg = _lib.load().stk_last_error().decode()
            assert "logistic" in msg or "d = 5" in msg, msg
    finally:
        m.close()


# ---------------------------------------------------------------- the driver
PARTS = (200, 333, 64)


def _driver(rows):
    import os
    from conftest import ROOT
    from stark_amd import stark
    from stark_amd.rdd import LocalContext, LocalRDD

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": 5, "x": a[:, :5], "y": a[:, 5].astype(np.int64)}

    cuts = np.concatenate([[0], np.cumsum(PARTS)])
    rdd = LocalRDD([rows[cuts[i]:cuts[i + 1]] for i in range(len(PARTS))])     # three partitions of these sizes
    st = stark.Stark(LocalContext(), rdd, prep)
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "logistic.stan"))
    return st


def test_driver_waic_and_fitted_mean(ctx):
    """Stark.waic over 3 logistic partitions (n = 200, 333, 64; d = 5) equals the restatement over the
    union of rows; draws shifted by three posterior sd score a lower elpd_waic (the restatement says so
    first); fitted_mean is the restatement's mu."""
    from stark_amd import engine, stark
    from stark_amd import rdd as _rdd
    n, d, S = sum(PARTS), 5, 48
    rng, X, y, truth = make_data("logistic", n, d)
    rows = [tuple(X[i]) + (int(y[i]),) for i in range(n)]
    st = _driver(rows)
    assert [len(p) for p in _rdd.partitions_of(st.rdd)] == list(PARTS)
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        _, _, H = m.hessian(0, truth)
    finally:
        m.close()
    sd = np.sqrt(np.diag(np.linalg.inv(-H)))
    Q = truth[None, :] + rng.normal(size=(S, d + 1)) * sd[None, :]
    results = []
    for shift in (0.0, 3.0):
        Qs = Q + shift * sd[None, :]
        samples = np.vstack([Qs.T, np.zeros((1, S))])              # P x S with an lp__ row
        ref, rtot, tscale = ref_stats("logistic", X, y, Qs)
        out = st.waic(samples)
        assert out["partition_totals"].shape == (3, 8) and out["n"] == n
        assert [int(v) for v in out["partition_totals"][:, 0]] == list(PARTS)
        for key, j in (("lppd", 1), ("p_waic", 2), ("elpd_waic", 3)):
            assert abs(out[key] - rtot[j]) <= BAR * tscale[j], (key, out[key], rtot[j])
        assert out["waic"] == -2 * out["elpd_waic"] and out["n_non_finite"] == 0 and out["n_high_var"] == rtot[5]
        e = (ref["lppd"] - ref["var"]).astype(L)
        se = float(np.sqrt(n / L(n - 1) * ((e * e).sum() - e.sum() ** 2 / n)))
        assert abs(out["se"] - se) <= 1e-8 * se
        results.append((out["elpd_waic"], rtot[3]))
    assert results[1][1] < results[0][1]          # the restatement: the shifted draws score lower
    assert results[1][0] < results[0][0]
    Xn = rng.uniform(-1.7, 1.7, (23, d))
    mu = engine.fitted_mean(ctx, "logistic", Xn, Q)
    rmu = ref_stats("logistic", Xn, np.zeros(23, np.int32), Q)[0]["mu"]
    assert np.abs(mu - rmu).max() <= BAR
