"""The dense_e and unit_e metrics of the regression NUTS sampler (k_nuts_step<NCH, DENSE>).

The CPU oracle has only a diagonal metric, so the dense kernels are pinned through it indirectly:

  1. a block metric blockdiag(a, L L^T[, s]) is the oracle's diag NUTS on the reparametrised data X L;
  2. a general dense metric at max_depth 1 has two one-leapfrog candidates, computed in numpy;
  3. the adapted metric is Stan's covar_adaptation formula on the run's own warmup draws;
  4. moments against the closed-form posterior, leapfrogs against the diag_e run;
  5. save / load; 6. unit_e replayed by the oracle; 7. refusals; 8. the Stark driver.

Bars: q rtol 1e-8 / atol 1e-10, lp 1e-9 relative, discrete stats equal, accept_stat and energy
rtol 1e-9 / atol 1e-12 (those of test_gpu_sweep_shards.py's twin)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _over(a, b, rtol, atol):
    a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
    with np.errstate(invalid="ignore"):
        r = np.where(a == b, 0.0, np.abs(a - b) / (atol + rtol * np.abs(b)))
    return float(np.where(np.isnan(r), np.inf, r).max())


def _check_rows(tag, rows):
    """rows: (where, q, lp, stats, want q, want lp, want stats).  Prints the largest errors in units
    of the bars, then asserts every bar on every row."""
    eq = max(_over(r[1], r[4], 1e-8, 1e-10) for r in rows)
    elp = max(_over(r[2], r[5], 0.0, 1e-9 * max(1.0, abs(r[5]))) for r in rows)
    est = max(_over(r[3][[0, 5]], r[6][[0, 5]], 1e-9, 1e-12) for r in rows)
    flips = sum(int(not np.array_equal(r[3][2:5], r[6][2:5])) for r in rows)
    print(f"MAXERR {tag} transitions={len(rows)} flipped={flips} q_over_bar={eq:.3e} lp_over_bar={elp:.3e} "
          f"stat_over_bar={est:.3e}")
    for where, q, lp, st, oq, olp, ost in rows:
        assert st[2] == ost[2] and st[3] == ost[3] and st[4] == ost[4], (where, st, ost)
        np.testing.assert_allclose(q, oq, rtol=1e-8, atol=1e-10, err_msg=str(where))
        assert abs(lp - olp) <= 1e-9 * max(1.0, abs(olp)), (where, lp, olp)
        np.testing.assert_allclose(st[[0, 5]], ost[[0, 5]], rtol=1e-9, atol=1e-12, err_msg=str(where))


def _regression(family, n, d, seed, xscale=1.0):
    rng = np.random.default_rng(seed)
    X = xscale * rng.uniform(-1.7, 1.7, (n, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d) / xscale
    if family == "logistic":
        y = (rng.uniform(size=n) < 1 / (1 + np.exp(-(0.2 + X @ beta)))).astype(np.int32)
    else:
        y = 0.3 + X @ beta + rng.normal(size=n)
    return X, y


def _fam(orc, family):
    return orc.FAM_LOGREG if family == "logistic" else orc.FAM_LINREG


# ================================================================ 1. fixed-metric twin by reparametrisation
TWIN_D = [9, 70, 200, 300]          # NCH = 1, 2, 4, 16 of k_nuts_step
TWIN_EPS = (0.02, 0.05, 0.1, 0.3)


@pytest.mark.parametrize("d", TWIN_D)
@pytest.mark.parametrize("family", ["logistic", "linear"])
def test_block_dense_metric_is_the_oracle_on_reparametrised_data(ctx, orc, family, d):
    """M^-1 = blockdiag(a, L L^T[, s]): dense NUTS on (X, q) is the oracle's diag NUTS on (X L, q')
    with beta' = L^-1 beta and inv_metric (a, 1, ..., 1[, s]), on the same momentum normals."""
    from stark_amd import engine
    n, chains = 300, 16 if d <= 70 else 4
    lin = family == "linear"
    D = d + 1 + int(lin)
    X, y = _regression(family, n, d, 100 * d + int(lin), xscale=0.07 if lin else 1.0)
    rng = np.random.default_rng(7 * d + int(lin))
    Lb = np.tril(rng.normal(0, 0.3 / np.sqrt(d), (d, d)), -1) + np.diag(rng.uniform(0.5, 1.5, d))
    a, s = rng.uniform(0.5, 2.0, 2)
    if lin:
        # the linear density curves by n / sigma^2 along alpha and by 2 n along log sigma, and its
        # columns are scaled so that beta's curvature n var(x) is of order 1: with a and s of the
        # inverse size the largest step, 0.3, stays inside the leapfrog's stability bound
        a, s = a / n, s / (2 * n)
    Minv = np.zeros((D, D))
    Minv[0, 0] = a
    Minv[1:d + 1, 1:d + 1] = Lb @ Lb.T
    Minv[1:d + 1, 1:d + 1] = np.tril(Minv[1:d + 1, 1:d + 1]) + np.tril(Minv[1:d + 1, 1:d + 1], -1).T
    im_orc = np.ones(D)
    im_orc[0] = a
    if lin:
        Minv[-1, -1] = s
        im_orc[-1] = s
    q0p = rng.normal(0, 0.1, (chains, D))          # start points in the oracle's coordinates
    to_q = lambda qp: np.concatenate([qp[:1], Lb @ qp[1:d + 1], qp[d + 1:]])   # noqa: E731
    q0 = np.array([to_q(v) for v in q0p])
    om = orc.Model(_fam(orc, family), X=np.ascontiguousarray(X @ Lb), y=y)
    want = {(eps, c): om.transition(q0p[c], seed=31, gid=c, iteration=4, eps=eps, inv_metric=im_orc, max_depth=6)
            for eps in TWIN_EPS for c in range(chains)}
    # the case is what it is meant to be, by the oracle alone
    depths = sorted({int(w[2][2]) for w in want.values()})
    assert max(depths) >= 4, depths
    moved = sum(bool(np.any(want[eps, c][0] != q0p[c])) for eps in TWIN_EPS for c in range(chains))
    assert 4 * moved >= 3 * len(want), (moved, len(want))
    m = engine.Model(ctx, family, [{"x": X, "y": y}])
    rows = []
    try:
        for eps in TWIN_EPS:
            q, lp, st = m.transition(0, q0, seed=31, iteration=4, eps=eps, inv_metric=Minv, max_depth=6)
            for c in range(chains):
                oq, olp, ost, _ = want[eps, c]
                rows.append(((eps, c), q[c], lp[c], st[c], to_q(oq), olp, ost))
    finally:
        m.close()
    _check_rows(f"dense_twin[{family}-{d}] depths={depths}", rows)


# ================================================================ 2. general dense metric, one leaf
@pytest.mark.parametrize("D", [11, 202])
def test_general_dense_metric_one_leaf(ctx, orc, D):
    """A random SPD M^-1 with alpha-beta and log sigma cross terms, max_depth 1: the draw is q0 or one
    of the two one-leapfrog candidates of p = L^-T u, u the diag path's normals (numpy + the oracle's
    lpgrad).  16 chains; at D = 202 the sweeps take at most 8 chains per launch, so they run as two
    calls of 8 with their own RNG iteration."""
    from stark_amd import engine
    d, n, seed = D - 2, 300, 19
    X, y = _regression("linear", n, d, 5 * D)
    rng = np.random.default_rng(D)
    G = rng.normal(size=(D, D))
    Minv = (G @ G.T / D + 0.5 * np.eye(D)) / n
    Minv = np.tril(Minv) + np.tril(Minv, -1).T
    assert abs(Minv[0, 1]) > 0 and abs(Minv[-1, 1]) > 0 and abs(Minv[-1, 0]) > 0    # cross terms
    L = np.linalg.cholesky(Minv)
    om = orc.Model(orc.FAM_LINREG, X=X, y=y)
    # starts within 0.02 of the posterior mode and a step at which, by the numpy reference alone, the
    # acceptance probabilities of the 32 candidates spread below 1 (0.76..1 at D = 11, 0.84..1 at 202)
    eps = 0.35 if D == 11 else 0.1
    batches = [(0, 16)] if D <= 130 else [(0, 8), (1, 8)]
    ols, _ = orc.linreg_exact_moments(X, y)
    rss = float(((y - np.hstack([np.ones((n, 1)), X]) @ ols) ** 2).sum())
    q0 = np.concatenate([ols, [0.5 * np.log(rss / n)]]) + np.random.default_rng(3).normal(0, 0.02, (16, D))
    m = engine.Model(ctx, "linear", [{"x": X, "y": y}])
    moved, worst_q, worst_a, below1 = 0, 0.0, 0.0, 0
    try:
        for b, (it, C) in enumerate(batches):
            qs = q0[b * C:(b + 1) * C]
            q, lp, st = m.transition(0, qs, seed=seed, iteration=it, eps=eps, inv_metric=Minv, max_depth=1)
            for c in range(C):
                u = np.array([orc.lib().orc_normal(seed, c, it, 0, e, orc.TAG_MOM) for e in range(D)])
                p = np.linalg.solve(L.T, u)
                lp0, g0 = om.lpgrad(qs[c])
                H0 = -lp0 + 0.5 * p @ Minv @ p
                cands = []
                for sgn in (1.0, -1.0):
                    ph = p + 0.5 * sgn * eps * g0
                    q1 = qs[c] + sgn * eps * (Minv @ ph)
                    lp1, g1 = om.lpgrad(q1)
                    p1 = ph + 0.5 * sgn * eps * g1
                    H1 = -lp1 + 0.5 * p1 @ Minv @ p1
                    acc = 1.0 if H0 - H1 > 0 else float(np.exp(H0 - H1))
                    cands.append((q1, acc, lp1))
                assert st[c, 2] == 1 and st[c, 3] == 1, st[c]
                below1 += int(st[c, 0] < 1.0)
                if np.array_equal(q[c], qs[c]):
                    err = min(abs(st[c, 0] - a) for _, a, _ in cands)
                else:
                    moved += 1
                    k = int(np.argmin([np.abs(q[c] - q1).max() for q1, _, _ in cands]))
                    q1, acc, lp1 = cands[k]
                    worst_q = max(worst_q, _over(q[c], q1, 1e-8, 1e-10))
                    np.testing.assert_allclose(q[c], q1, rtol=1e-8, atol=1e-10, err_msg=str((b, c)))
                    assert abs(lp[c] - lp1) <= 1e-9 * max(1.0, abs(lp1)), (lp[c], lp1)
                    err = abs(st[c, 0] - acc)
                worst_a = max(worst_a, err)
                assert err <= 1e-9, ((b, c), st[c, 0], [a for _, a, _ in cands])
    finally:
        m.close()
    print(f"MAXERR dense_leaf[D={D}] moved={moved}/16 accept_below_1={below1}/16 q_over_bar={worst_q:.3e} "
          f"accept_abs={worst_a:.3e}")
    assert moved > 8, moved


# ================================================================ correlated linear data (tests 3, 4, 5, 8)
def _correlated_linear(n=400, d=12, rho=0.9, seed=5):
    rng = np.random.default_rng(seed)
    X = np.sqrt(rho) * rng.normal(size=(n, 1)) + np.sqrt(1 - rho) * rng.normal(size=(n, d))
    beta = rng.normal(0, 1, d)
    y = 0.3 + X @ beta + rng.normal(size=n)
    return X, y


def _covar_formula(draws):
    """Stan 2.19.1 covar_adaptation at a window's end, on the window's draws (n x D)."""
    n = draws.shape[0]
    cov = np.cov(draws.T, ddof=1)
    return (n / (n + 5.0)) * cov + 1e-3 * (5.0 / (n + 5.0)) * np.eye(draws.shape[1]), cov


def _assert_metric(got, draws, where):
    want, cov = _covar_formula(draws)
    sc = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    over = float((np.abs(got - want) / (1e-8 * sc)).max())
    print(f"MAXERR dense_adapt{where} n={draws.shape[0]} metric_over_bar={over:.3e}")
    np.testing.assert_array_equal(got, got.T, err_msg=str(where))
    assert np.all(np.abs(got - want) <= 1e-8 * sc), (where, over)


# ================================================================ 3. adaptation follows the formula
@pytest.mark.parametrize("nshards", [1, 2])
def test_dense_adaptation_follows_the_formula(ctx, nshards):
    """Default buffers at num_warmup 200: windows end after draws 99 (n = 25, draws 75..99) and 149
    (n = 50, draws 100..149)."""
    from stark_amd import engine
    X, y = _correlated_linear()
    rows = 400 // nshards
    shards = [{"x": X[k * rows:(k + 1) * rows], "y": y[k * rows:(k + 1) * rows]} for k in range(nshards)]
    chains, D = 4, 14
    m = engine.Model(ctx, "linear", shards)
    s = m.sampler(num_warmup=200, num_samples=10, chains=chains, seed=5, save_warmup=True, metric="dense_e")
    try:
        s.run(100)
        _, im1 = s.adaptation()
        s.run()
        eps, im2 = s.adaptation()
        uq = [s.unconstrained(k) for k in range(nshards)]
        info = s.info()
    finally:
        s.close()
        m.close()
    assert info["errors"] == 0 and info["done"] == nshards * chains
    assert im1.shape == im2.shape == (nshards * chains, D, D)
    for k in range(nshards):
        for c in range(chains):
            _assert_metric(im1[k * chains + c], uq[k][c, 75:100], (nshards, k, c, "w1"))
            _assert_metric(im2[k * chains + c], uq[k][c, 100:150], (nshards, k, c, "w2"))
    assert np.all(eps > 0) and np.all(eps != 1.0)


# ================================================================ 4. moments and efficiency
def test_dense_moments_and_leapfrogs(ctx, orc):
    from stark_amd import engine
    from stark_amd.diagnostics import ess
    X, y = _correlated_linear()
    mean, _ = orc.linreg_exact_moments(X, y)
    chains, ns = 8, 300
    m = engine.Model(ctx, "linear", [{"x": X, "y": y}])
    try:
        dense = m.sample(num_warmup=300, num_samples=ns, chains=chains, seed=5, metric="dense_e")
        diag = m.sample(num_warmup=300, num_samples=ns, chains=chains, seed=5, metric="diag_e")
    finally:
        m.close()
    assert dense.info["errors"] == 0 and dense.info["divergent"] == 0
    d = dense.draws[0]
    z = []
    for r in range(13):                                         # alpha, beta_1..12
        x = d[r].reshape(chains, ns)
        mcse = x.std(ddof=1) / np.sqrt(ess(x))
        z.append((x.mean() - mean[r]) / mcse)
    lf_dense, lf_diag = dense.stats[0][:, 3].mean(), diag.stats[0][:, 3].mean()
    print(f"MAXERR dense_moments max|z|={np.abs(z).max():.2f} leapfrogs dense={lf_dense:.2f} diag={lf_diag:.2f} "
          f"ratio={lf_dense / lf_diag:.3f}")
    assert np.all(np.abs(z) < 5), z
    assert lf_dense <= lf_diag / 3.0, (lf_dense, lf_diag)


# ================================================================ 5. split run
def test_dense_split_run_is_bit_identical(ctx):
    from stark_amd import engine
    X, y = _correlated_linear()
    m = engine.Model(ctx, "linear", [{"x": X, "y": y}])
    cfg = dict(num_warmup=200, num_samples=20, chains=4, seed=5, save_warmup=True)

    def arrays(s):
        eps, im = s.adaptation()
        dr, st = s.draws(0)
        return {"eps": eps, "metric": im, "draws": dr, "stats": st, "uq": s.unconstrained(0)}

    ref, a, b = (m.sampler(metric="dense_e", **cfg) for _ in range(3))
    dg, dg2 = m.sampler(**cfg), m.sampler(**cfg)
    try:
        ref.run()
        want = arrays(ref)
        a.run(120)                          # inside the second window: its Welford sums travel too
        blob = a.save_state()
        b.load_state(blob)
        assert int(b.iterations().min()) == 120
        np.testing.assert_array_equal(arrays(a)["metric"], arrays(b)["metric"])
        b.run()
        got = arrays(b)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert want["metric"].shape == (4, 14, 14) and ref.info()["errors"] == 0
        dg.run(120)
        before = arrays(a)
        with pytest.raises(engine.StarkHipError, match="STK_E_ARG") as ei:
            a.load_state(dg.save_state())                      # a diag blob into a dense sampler
        assert ei.value.code == -1
        for k, v in arrays(a).items():                         # nothing was written
            np.testing.assert_array_equal(v, before[k], err_msg=k)
        with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
            dg2.load_state(blob)                               # and the reverse
    finally:
        for x in (ref, a, b, dg, dg2):
            x.close()
        m.close()


# ================================================================ 6. unit_e
def _unit_e_case(ctx, orc, family, shard, om, chains):
    from stark_amd import engine
    nw, ns, seed = 150, 20, 23
    m = engine.Model(ctx, family, [shard])
    s = m.sampler(num_warmup=nw, num_samples=ns, chains=chains, seed=seed, save_warmup=True, metric="unit_e")
    try:
        s.run()
        eps, im = s.adaptation()
        d, st = s.draws(0)
        uq = s.unconstrained(0)
        info = s.info()
    finally:
        s.close()
        m.close()
    assert info["errors"] == 0 and info["done"] == chains
    np.testing.assert_array_equal(im, np.ones((chains, om.D)))
    assert np.all(eps != 1.0) and np.all(eps > 0) and len(set(eps)) == chains       # adapted, per chain
    rows = []
    for c in range(chains):
        assert np.all(st[c * ns:(c + 1) * ns, 1] == eps[c])
        for t in range(nw, nw + ns):
            i = c * ns + t - nw
            oq, olp, ost, _ = om.transition(uq[c, t - 1], seed=seed, gid=c, iteration=t, eps=st[i, 1])
            rows.append(((c, t), uq[c, t], d[-1, i], st[i], oq, olp, ost))
    _check_rows(f"unit_e[{family}]", rows)


def test_unit_e_logistic(ctx, orc):
    X, y = _regression("logistic", 400, 9, 77)
    _unit_e_case(ctx, orc, "logistic", {"x": X, "y": y}, orc.Model(orc.FAM_LOGREG, X=X, y=y), 4)


def test_unit_e_schools(ctx, orc):
    sh = {"y": orc.SCHOOLS_Y, "sigma": orc.SCHOOLS_SIGMA}
    _unit_e_case(ctx, orc, "schools", sh, orc.Model(orc.FAM_SCHOOLS, y=sh["y"], sigma=sh["sigma"]), 5)


# ================================================================ 7. refusals
def test_dense_refusals(ctx, orc):
    from stark_amd import engine
    ms = engine.Model(ctx, "schools", [{"y": orc.SCHOOLS_Y, "sigma": orc.SCHOOLS_SIGMA}])
    X, y = _regression("linear", 50, 3, 1)
    ml = engine.Model(ctx, "linear", [{"x": X, "y": y}])
    kw = dict(num_warmup=20, num_samples=5, chains=2)
    try:
        with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG.*dense_e is for the regression families"):
            ms.sampler(metric="dense_e", **kw)
        bad = np.eye(5)
        bad[1, 2] = bad[2, 1] = 2.0                                    # symmetric, indefinite
        with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG.*not positive definite"):
            ml.sampler(metric="dense_e", inv_metric=bad, **kw)
        with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG.*not positive definite"):
            ml.transition(0, np.zeros((2, 5)), seed=1, iteration=0, eps=0.1, inv_metric=bad)
        ns = np.eye(5)
        ns[1, 2] = 0.25                                                # not symmetric
        with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG.*not symmetric"):
            ml.sampler(metric="dense_e", inv_metric=ns, **kw)
        with pytest.raises(ValueError, match="shape"):
            ml.sampler(metric="dense_e", inv_metric=np.eye(4), **kw)   # D = 5
        with pytest.raises(ValueError, match="shape"):
            ml.sampler(metric="dense_e", inv_metric=np.ones((5, 4)), **kw)
        with pytest.raises(ValueError, match="shape"):
            ml.transition(0, np.zeros((2, 5)), seed=1, iteration=0, eps=0.1, inv_metric=np.eye(6))
        ml.sampler(metric="dense_e", inv_metric=np.eye(5) * 0.5, **kw).close()
    finally:
        ms.close()
        ml.close()


# ================================================================ 8. the Stark driver
def test_driver_dense_metric_end_to_end(ctx, orc):
    """Two partitions of the correlated linear data through concensusWeight with dense_e: the consensus
    means of (alpha, beta) against the closed form (the precision-weighted mean of the partitions'
    exact posterior means) in units of the draws' MCSE; distribute() on the logistic family."""
    from stark_amd import stark
    from stark_amd.diagnostics import ess
    from stark_amd.rdd import LocalContext
    X, y = _correlated_linear()
    sc = LocalContext()
    rowsl = [(tuple(X[i]), float(y[i])) for i in range(400)]

    def prep(data):
        return {"N": len(data), "K": 12, "x": [r[0] for r in data], "y": [r[1] for r in data]}

    st = stark.Stark(sc, sc.parallelize(rowsl, 2), prep)
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "linear.stan"))
    out = st.concensusWeight(iter=400, chains=4, seed=8, control={"metric": "dense_e"}, separate_lp=True,
                             permuted=False)
    assert st.last_run.info["metric"] == "dense_e" and st.last_run.info["errors"] == 0
    assert out.shape == (15, 800) and np.isfinite(out).all()
    parts = sc.parallelize(rowsl, 2).partitions()
    exact = [orc.linreg_exact_moments(np.array([r[0] for r in p]), np.array([r[1] for r in p]))[0] for p in parts]

    def zscores(draws, want):
        z = []
        for r in range(13):                                      # alpha, beta_1..12
            x = draws[r].reshape(4, 200)
            z.append((x.mean() - want[r]) / (x.std(ddof=1) / np.sqrt(ess(x))))
        return np.array(z)

    # every partition's own draws against that partition's closed-form posterior mean
    zp = [zscores(st.last_run.draws[k], exact[k]) for k in range(2)]
    # The combine is linear in the draws: its mean is sum_s W_s mean_s under sum_s W_s = I, with W_s the
    # weights it formed from the run's sample covariances.  The closed form is that combination of the
    # partitions' closed-form means.  (With the exact posterior precisions as weights instead, the
    # weights' own sampling noise, sqrt(P / S) relative, times the distance between the two partitions'
    # means enters the difference, and the draws' MCSE does not cover it: max |z| = 6.2 on this run.)
    Ws = [np.linalg.inv(np.cov(st.last_run.draws[k][:14])) for k in range(2)]
    want = np.linalg.solve(Ws[0] + Ws[1], Ws[0] @ np.append(exact[0], st.last_run.draws[0][13].mean())
                           + Ws[1] @ np.append(exact[1], st.last_run.draws[1][13].mean()))
    z = zscores(out, want)
    print(f"MAXERR dense_driver max|z| partitions={np.abs(zp[0]).max():.2f}, {np.abs(zp[1]).max():.2f} "
          f"consensus={np.abs(z).max():.2f}")
    assert np.all(np.abs(zp[0]) < 5) and np.all(np.abs(zp[1]) < 5), zp
    assert np.all(np.abs(z) < 5), z
    Xl, yl = _regression("logistic", 300, 6, 9)
    rl = [(tuple(Xl[i]), int(yl[i])) for i in range(300)]
    sl = stark.Stark(sc, sc.parallelize(rl, 2), lambda data: {"N": len(data), "K": 6, "x": [r[0] for r in data],
                                                               "y": [r[1] for r in data]})
    sl.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "logistic.stan"))
    nv = sl.distribute(n=2, iter=200, chains=2, seed=4, control={"metric": "dense_e"})
    assert nv.shape == (2 * 8, 200) and np.isfinite(nv).all() and sl.last_run.info["metric"] == "dense_e"
