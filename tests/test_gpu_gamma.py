"""The gamma family (gamma, log link) on the GPU: every sweep's lp / gradient against the longdouble reference
tests/gamma_ref.py (the density of include/stark_hip.h, STK_GAMMA) on outlier data and on precise data (shape 1e4,
the case that tells the deviance form from the textbook form), extreme coefficients and shapes, priors, chain batches
and grouped launches, the data round trip, sampling against an exact grid posterior, determinism and checkpoints, the
metrics and U-turn criteria, the Stark driver, and the family's refusals.

Bars: check_bars of tests/test_gpu_student.py (the project's 1e-10 density bars), restated here.

Inputs.  X, alpha and beta are dyadic (X multiples of 2^-6 in [-1.7, 1.7], the coefficients multiples of 2^-10), as
tests/test_gpu_student.py builds them and for the reason its docstring gives: every product x_ij beta_j and every
partial sum of eta is exact in fp64 whatever the order of the sum, so eta reaches the residual without rounding error,
on the device as in the reference.  Here d (d lp / d eta) / d eta is a e^t, 1e8 at the largest shapes, so an ulp of an
eta of size 1 would move a row's gradient term by 1e-8.  y is arbitrary.
"""
import numpy as np
import pytest

import gamma_ref as R

pytestmark = pytest.mark.gpu

FAM = "gamma"
RTOL = 1e-10


def check_bars(lp, g, olp, og, where=""):
    """lp within 1e-10 of max(|lp|, 1); every gradient component within 1e-10 of max(|g_j|, 1e-3 (max |g| + 1)).
    Returns the largest of each as a fraction of its bar."""
    wl = wg = 0.0
    for c in range(len(olp)):
        o = np.float64(olp[c])
        elp = abs(lp[c] - o) / max(abs(o), 1.0)
        ogc = og[c].astype(np.float64)
        bar = RTOL * np.maximum(np.abs(ogc), (np.abs(ogc).max() + 1.0) * 1e-3)
        eg = np.abs(g[c] - ogc)
        assert elp < RTOL, (where, c, lp[c], o, elp)
        assert np.all(eg <= bar), (where, c, float((eg / bar).max()))
        wl, wg = max(wl, elp / RTOL), max(wg, float((eg / bar).max()))
    return wl, wg


def either_or(lp, g, olp, og, where):
    """either_or of tests/test_gpu_negbin.py: a point whose reference is finite in fp64 meets the bars or is
    non-finite, never +inf; one whose reference is not finite is non-finite."""
    with np.errstate(over="ignore", invalid="ignore"):
        fin = np.isfinite(olp.astype(np.float64)) & np.all(np.isfinite(og.astype(np.float64)), axis=1)
    assert not np.any(lp == np.inf), (where, lp)
    assert not np.any(np.isfinite(lp[~fin])), (where, lp[~fin])
    idx = np.flatnonzero(fin & np.isfinite(lp))
    wl, wg = check_bars(lp[idx], g[idx], olp[idx], og[idx], where)
    return fin, idx, wl, wg


A0 = 0.2998046875        # 307 / 1024


def dyadic(v, bits):
    return np.round(np.asarray(v) * 2.0 ** bits) / 2.0 ** bits


def make_data(n, d, seed=None, shape=2.0, outliers=True):
    """X ~ U(-1.7, 1.7) and beta ~ N(0, 1/sqrt(d)), dyadic; y = exp(A0 + X beta) Gamma(shape, 1 / shape); with
    outliers: rows 1 .. max(1, n/50) times 1e6 and 1e-6 alternately, and row 0 with x = 0 and y = 1."""
    rng = np.random.default_rng(n * 1000 + d if seed is None else seed)
    X = dyadic(rng.uniform(-1.7, 1.7, (n, d)), 6)
    if outliers:
        X[0] = 0.0
    beta = dyadic(rng.normal(0, 1 / np.sqrt(d), d), 10)
    y = np.exp(A0 + X @ beta) * rng.gamma(shape, 1.0 / shape, n)
    if outliers:
        k = min(max(1, n // 50), n - 1)
        y[1:1 + k] *= np.where(np.arange(k) % 2 == 0, 1e6, 1e-6)
        y[0] = 1.0
    return rng, X, y, beta


def points(rng, beta, C, d, lo=1e-2, hi=1e4, one=2.0):
    """C points (alpha, beta, u) as tests/test_gpu_student.py's: point 0 the data's own coefficients, the others
    within N(0, 0.2) of them, dyadic; the shape spread log-uniformly over [lo, hi] across the chains (C = 1: `one`)."""
    q = rng.normal(0, 0.2, (C, d + 2))
    q[:, 0] += A0
    q[:, 1:d + 1] += beta
    q[0, :d + 1] = np.concatenate([[A0], beta])
    q[:, :d + 1] = dyadic(q[:, :d + 1], 10)
    q[:, -1] = np.log(one) if C == 1 else np.log(lo) + np.log(hi / lo) * np.arange(C) / (C - 1)
    return q


VALU = [(1, 1, 1), (7, 3, 5), (65, 104, 3), (3000, 120, 5), (333, 129, 5), (257, 300, 8)]
S16 = [(1, 1, 16), (7, 3, 16), (300, 113, 16), (333, 128, 16), (4097, 50, 16), (65, 104, 20)]
S16W = [(333, 129, 16), (257, 512, 16), (130, 1023, 16), (200, 1024, 16)]
G64 = [(1, 1, 64), (300, 17, 64), (333, 129, 64), (200, 1024, 64), (130, 1001, 70)]


# ---------------------------------------------------------------- 1. every sweep, outlier data
@pytest.mark.parametrize("n,d,C", VALU + S16 + S16W + G64)
def test_gamma_lpgrad(ctx, n, d, C):
    """VALU sweeps (k_sweep3, k_sweep2, k_sweep at odd and wide d), k_sweep16 (masked last sub-tile, the VALU last
    tile, the slot released early or late, several chunks, 16 + 4), k_sweep16w and the 64-chain passes (64 + 4 + 2),
    each with the family's reduce.  Two shards, the first a third of the rows; the second is evaluated.  Outliers at
    1e6 and 1e-6 of the mean (t = +-13.8: e^t from 1e-6 to 1e6), shapes from 1e-2 to 1e4 across the chains."""
    from stark_amd import engine
    rng, X, y, beta = make_data(n, d)
    k = max(1, n // 3)
    m = engine.Model(ctx, FAM, [{"x": X[:k], "y": y[:k]}, {"x": X, "y": y}])
    try:
        assert m.D == [d + 2, d + 2] and m.P == [d + 3, d + 3] and m.n_rows == [k, n]
        q = points(rng, beta, C, d)
        lp, g = m.log_density_grad(1, q)
    finally:
        m.close()
    olp, og = R.ref_lpgrad(X, y, q)
    assert np.all(np.isfinite(olp.astype(np.float64))) and np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    wl, wg = check_bars(lp, g, olp, og, (n, d, C))
    print(f"MAXERR gamma[outlier-{n}-{d}-{C}] lp={wl:.3e} grad={wg:.3e}")


# ---------------------------------------------------------------- 2. every sweep family, precise data
@pytest.mark.parametrize("n,d,C", [(300, 113, 16), (4097, 50, 16), (300, 17, 64), (200, 1024, 16), (257, 300, 8)])
def test_gamma_lpgrad_precise(ctx, n, d, C):
    """y = exp(A0 + X beta) Gamma(1e4, 1e-4), no outliers; every chain at the data's own coefficients, the shape
    log-uniform over [1e2, 1e8].  The textbook form of the density fails the lp bar here in fp64 (a n and a L cancel);
    the deviance form does not."""
    from stark_amd import engine
    rng, X, y, beta = make_data(n, d, shape=1e4, outliers=False)
    q = points(rng, beta, C, d, lo=1e2, hi=1e8)
    q[:, :d + 1] = np.concatenate([[A0], beta])
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    try:
        lp, g = m.log_density_grad(0, q)
    finally:
        m.close()
    olp, og = R.ref_lpgrad(X, y, q)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    wl, wg = check_bars(lp, g, olp, og, ("precise", n, d, C))
    print(f"MAXERR gamma[precise-{n}-{d}-{C}] lp={wl:.3e} grad={wg:.3e}")


# ---------------------------------------------------------------- 3. extreme coefficients and shapes
SHAPES_X = [(300, 113, 16), (500, 100, 64), (400, 60, 4), (300, 200, 16), (257, 131, 3)]


@pytest.mark.parametrize("scale", [30.0, 1e3, 1e150])
@pytest.mark.parametrize("n,d,C", SHAPES_X)
def test_gamma_lpgrad_extreme_eta(ctx, scale, n, d, C):
    """The first half of the points' (alpha, beta) scaled by 30, 1e3, 1e150.  At 30 every reference point is finite
    in fp64 (e^t up to about 1e60), so the GPU must be finite and within the bars at every point; at 1e3 and 1e150
    some row's e^t overflows at every scaled point, so exactly the unscaled half is finite, and those points must be
    finite and within the bars; a scaled point is -inf or NaN, never +inf."""
    from stark_amd import engine
    rng, X, y, beta = make_data(n, d, seed=int(scale) % 1000 + n)
    q = points(rng, beta, C, d)
    q[: C // 2, : d + 1] *= scale
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    try:
        lp, g = m.log_density_grad(0, q)
    finally:
        m.close()
    olp, og = R.ref_lpgrad(X, y, q)
    fin, idx, wl, wg = either_or(lp, g, olp, og, (scale, n, d, C))
    assert fin[C // 2:].all() and set(range(C // 2, C)) <= set(idx.tolist())
    if scale == 30.0:
        assert fin.all() and len(idx) == C
    else:
        assert not fin[: C // 2].any()
    print(f"MAXERR gamma[scale{scale:g}-{n}-{d}-{C}] lp={wl:.3e} grad={wg:.3e}")


@pytest.mark.parametrize("n,d,C", SHAPES_X)
def test_gamma_lpgrad_extreme_u(ctx, n, d, C):
    """u = +-40 and +-700 (shape from 1e-304 to 1e304: inside the doubles), and +-800, where e^u is 0 or inf in fp64:
    lp must be NaN or -inf there, and so must d lp / d u.  The reference is finite in fp64 at +-40 and at -700; at
    +700 it is not on this data (a H and a (e^t - 1) pass the largest double: H > 1e6 with the outlier rows), and
    either_or then asks the GPU for a non-finite lp there too."""
    from stark_amd import engine
    rng, X, y, beta = make_data(n, d, seed=n + d)
    q = points(rng, beta, C, d)
    q[:, -1] = np.resize([40.0, -40.0, 700.0, -700.0, 800.0, -800.0], C)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    try:
        lp, g = m.log_density_grad(0, q)
    finally:
        m.close()
    olp, og = R.ref_lpgrad(X, y, q)
    fin, idx, _wl, _wg = either_or(lp, g, olp, og, ("u", n, d, C))
    u = q[:, -1]
    assert not fin[np.abs(u) > 750].any() and fin[(np.abs(u) == 40) | (u == -700)].all() and len(idx) == int(fin.sum())
    assert not np.any(np.isfinite(g[~fin, -1]))


def test_gamma_nan_stays_nan(ctx):
    """A NaN alpha, beta or u gives a NaN lp at that point and leaves the other points alone."""
    from stark_amd import engine
    for n, d, C in [(300, 113, 16), (257, 100, 2), (300, 17, 64)]:
        rng, X, y, beta = make_data(n, d)
        q = points(rng, beta, C, d)
        m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
        try:
            lp0, _g0 = m.log_density_grad(0, q)
            qn = q.copy()
            qn[0, 0] = qn[1, 1] = np.nan
            if C > 2:
                qn[2, -1] = np.nan
            lp, _g = m.log_density_grad(0, qn)
        finally:
            m.close()
        bad = np.isnan(qn).any(1)
        assert np.all(np.isnan(lp[bad])) and np.array_equal(lp[~bad], lp0[~bad]), (n, d, C, lp[bad])


# ---------------------------------------------------------------- 4. priors, batches, grouped launches, data
@pytest.mark.parametrize("n,d,C", [(300, 113, 16), (257, 100, 2), (300, 17, 64)])
def test_gamma_priors(ctx, n, d, C):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    rng, X, y, beta = make_data(n, d)
    q = points(rng, beta, C, d)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    try:
        lp0, g0 = m.log_density_grad(0, q)
        m.set_prior(alpha=2.0, beta=0.5, shape=(2.0, 0.5))
        lp1, g1 = m.log_density_grad(0, q)
        m.set_prior(shape=(1.0, 0.25))                             # exponential(0.25); alpha, beta flat again
        lp2, g2 = m.log_density_grad(0, q)
        for bad in ((0.0, 1.0), (-1.0, 1.0), (2.0, -0.5), (np.inf, 1.0)):
            with pytest.raises(StarkHipError) as e:
                m.set_prior(shape=bad)
            assert e.value.code == -1
        with pytest.raises(StarkHipError) as e:                    # phi's prior is the negative binomial's
            m.set_prior(phi=(2.0, 0.5))
        assert e.value.code == -1 and FAM in str(e.value)
        m.set_prior(shape=(1.0, 0.0))                              # flat again
        lp3, g3 = m.log_density_grad(0, q)
    finally:
        m.close()
    check_bars(lp0, g0, *R.ref_lpgrad(X, y, q), where="flat")
    check_bars(lp1, g1, *R.ref_lpgrad(X, y, q, shape_prior=(2.0, 0.5), prior=(2.0, 0.5)), where="all three")
    check_bars(lp2, g2, *R.ref_lpgrad(X, y, q, shape_prior=(1.0, 0.25)), where="exponential")
    assert np.all(lp2 < lp0) and np.array_equal(lp0, lp3) and np.array_equal(g0, g3)


def test_gamma_chain_batches_and_shards_bitwise(ctx):
    """chains = 3, 17, 20 and 70 are the single launches of their batches, bit for bit; every shard at once, on
    shards of unequal n, is the per-shard calls, bit for bit."""
    from stark_amd import engine
    shards = []
    for s, n in enumerate((600, 333, 1025)):
        _rng, X, y, _beta = make_data(n, 100, seed=50 + s)
        shards.append({"x": X, "y": y})
    rng = np.random.default_rng(5)
    m = engine.Model(ctx, FAM, shards)
    try:
        for C in (3, 17, 20, 70):
            bt = engine.chain_batches(C, 100)
            assert bt == {3: [2, 1], 17: [16, 1], 20: [16, 4], 70: [64, 4, 2]}[C]
            q = rng.normal(0, 0.2, (3, C, 102))
            q[:, :, -1] = rng.uniform(-3, 6, (3, C))
            lp, g = m.log_density_grad_chains(q)
            c0 = 0
            for b in bt:
                blp, bg = m.log_density_grad_shards(np.ascontiguousarray(q[:, c0:c0 + b]))
                assert np.array_equal(lp[:, c0:c0 + b], blp) and np.array_equal(g[:, c0:c0 + b], bg), (C, c0, b)
                c0 += b
            assert c0 == C
        q = rng.normal(0, 0.2, (3, 16, 102))
        lp, g = m.log_density_grad_shards(q)
        for s in range(3):
            slp, sg = m.log_density_grad(s, q[s])
            assert np.array_equal(lp[s], slp) and np.array_equal(g[s], sg), s
            olp = R.ref_lpgrad(shards[s]["x"], shards[s]["y"], q[s])[0].astype(np.float64)
            assert np.all(np.abs(slp - olp) <= RTOL * np.maximum(np.abs(olp), 1.0))
    finally:
        m.close()


def test_gamma_refused_chain_count_then_a_valid_sweep(ctx):
    """tests/test_gpu_sweep_family_switch.py's case for this family: three chains are no single batch and are
    refused with STK_E_ARG before anything is launched; the same model then runs n = 77, d = 5, C = 2."""
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    N, D, C = 77, 5, 2
    rng, X, y, beta = make_data(N, D)
    q = points(rng, beta, C, D)[None]
    olp, og = R.ref_lpgrad(X, y, q[0])
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    try:
        assert engine.chain_batches(3, D) == [2, 1]
        with pytest.raises(StarkHipError) as e:
            m.log_density_grad_shards(np.concatenate([q, q[:, :1]], axis=1))
        assert e.value.code == -1
        lp, g = m.log_density_grad_shards(q)
        assert lp.shape == (1, C) and np.isfinite(lp).all() and np.isfinite(g).all()
        check_bars(lp[0], g[0], olp, og, "switch[gamma]")
    finally:
        m.close()


def test_gamma_model_data_round_trip(ctx):
    """copy_data returns y as given, bit for bit (the shard keeps it next to log y); the device fingerprint is the
    host twin's, carries the family word, and changes when one y changes in its last bit."""
    from stark_amd import engine
    _rng, X, y, _beta = make_data(300, 7)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    y2 = y.copy()
    y2[5] = np.nextafter(y[5], np.inf)
    m2 = engine.Model(ctx, FAM, [{"x": X, "y": y2}])
    lin = engine.Model(ctx, "linear", [{"x": X, "y": y}])
    try:
        back = m.copy_data(0)
        assert back["y"].dtype == np.float64 and np.array_equal(back["y"], y) and np.array_equal(back["x"], X)
        arr = m.device_arrays(0)
        assert set(arr) == {"x", "y"} and arr["x"][1] == 300 * 7 and arr["y"][1] == 300
        fp = int(m.fingerprint(0))
        assert fp == int(engine.shard_fingerprint(FAM, {"x": X, "y": y}))
        assert fp != int(lin.fingerprint(0))
        assert int(m2.fingerprint(0)) != fp and int(m2.fingerprint(0)) == int(engine.shard_fingerprint(FAM, {"x": X, "y": y2}))
        assert np.array_equal(m2.copy_data(0)["y"], y2)
    finally:
        m.close()
        m2.close()
        lin.close()


# ---------------------------------------------------------------- 5. sampling against an exact posterior
def grid_data():
    rng = np.random.default_rng(2026)
    x = rng.uniform(-1.7, 1.7, 300)
    y = np.exp(0.4 + 0.7 * x) * rng.gamma(3.0, 1.0 / 3.0, 300)
    return x, y


@pytest.fixture(scope="module")
def grid_posterior():
    """n = 300, d = 1, y = exp(0.4 + 0.7 x) Gamma(3, 1/3), shape ~ gamma(2, 0.5), flat alpha and beta: the posterior
    of (alpha, beta, u) on an 81 x 81 x 161 tensor grid over alpha 0.4 +- 0.3, beta 0.7 +- 0.3, u = log 3 +- 0.7, from
    the density's formulas in fp64 (H depends on alpha and beta alone, kappa on u alone).  Its every-other-point
    subgrid must agree to 1e-6 relative on all six moments and the mass on the grid's faces must be below 1e-12."""
    x, y = grid_data()
    a = 0.4 + np.linspace(-0.3, 0.3, 81)
    b = 0.7 + np.linspace(-0.3, 0.3, 81)
    u = np.log(3.0) + np.linspace(-0.7, 0.7, 161)
    ly = np.log(y)
    t = ly[None, None, :] - a[:, None, None] - b[None, :, None] * x[None, None, :]
    H = (np.expm1(t) - t).sum(2)
    sh = np.exp(u)
    kap = R.shape_terms(sh)[0].astype(np.float64)
    lp = (300 * kap - ly.sum() + u + (u - 0.5 * sh))[None, None, :] - sh[None, None, :] * H[:, :, None]
    q = np.array([[a[40], b[40], u[80]], [a[3], b[70], u[150]]])
    olp = R.ref_lpgrad(x[:, None], y, q, shape_prior=(2.0, 0.5))[0].astype(np.float64)
    assert np.allclose([lp[40, 40, 80], lp[3, 70, 150]], olp, rtol=1e-12)            # the grid is the reference's density

    def moments(lp, axes):
        w = np.exp(lp - lp.max())
        w /= w.sum()
        face = sum(np.take(w, i, axis=ax).sum() for ax in range(3) for i in (0, -1))
        out = []
        for ax, g in enumerate(axes):
            wm = w.sum(tuple(i for i in range(3) if i != ax))
            mu = (wm * g).sum()
            out.append((mu, (wm * (g - mu) ** 2).sum()))
        return np.array(out), face

    fine, face = moments(lp, (a, b, u))
    coarse, _ = moments(lp[::2, ::2, ::2], (a[::2], b[::2], u[::2]))
    assert face < 1e-12, face
    assert np.all(np.abs(coarse - fine) <= 1e-6 * np.abs(fine)), (coarse, fine)
    assert np.allclose(fine[:, 0], [0.4277, 0.7084, 1.1714], atol=5e-5), fine[:, 0]
    assert np.allclose(np.sqrt(fine[:, 1]), [0.0322, 0.0335, 0.0777], atol=5e-5), np.sqrt(fine[:, 1])
    return x, y, fine[:, 0].copy(), fine[:, 1].copy()


@pytest.mark.parametrize("metric", ["diag_e", "dense_e"])
@pytest.mark.parametrize("chains", [16, 3])
def test_gamma_sampling_exact(ctx, grid_posterior, chains, metric):
    """test_negbin_sampling_exact's criterion for alpha, beta and u = log shape: four-sigma bars from the run's own
    effective sizes, |mean - exact| <= 4 sd / sqrt(n_eff) and |var / exact - 1| <= 4 sqrt(2 / n_eff2), n_eff2 the
    n_eff of the centred squares; no divergences; the lp__ row is the reference density at the drawn point."""
    from stark_amd import diagnostics, engine
    x, y, mean, var = grid_posterior
    X = x[:, None].copy()
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    try:
        m.set_prior(shape=(2.0, 0.5))
        res = m.sample(num_warmup=300, num_samples=1000, chains=chains, seed=2900 + chains, metric=metric)
    finally:
        m.close()
    assert res.info["divergent"] == 0 and res.info["errors"] == 0, res.info
    dr = res.draws[0]
    assert dr.shape == (4, chains * 1000) and np.isfinite(dr).all() and np.all(dr[2] > 0)
    par = np.stack([dr[0], dr[1], np.log(dr[2])])
    for p in range(3):
        ch = par[p].reshape(chains, 1000)
        ne = diagnostics.ess(ch)
        sq = (ch - mean[p]) ** 2
        ne2 = diagnostics.ess(sq)
        em = abs(ch.mean() - mean[p]) / (np.sqrt(var[p]) / np.sqrt(ne))
        ev = abs(sq.mean() / var[p] - 1.0) / np.sqrt(2.0 / ne2)
        print(f"chains={chains} {metric} par {p}: n_eff {ne:.0f} mean z {em:.2f}; n_eff2 {ne2:.0f} var z {ev:.2f}")
        assert em <= 4.0, (p, ch.mean(), mean[p], ne)
        assert ev <= 4.0, (p, sq.mean(), var[p], ne2)
    olp = R.ref_lpgrad(X, y, np.ascontiguousarray(par.T), shape_prior=(2.0, 0.5))[0].astype(np.float64)
    assert np.all(np.abs(dr[3] - olp) <= RTOL * np.maximum(np.abs(olp), 1.0))


# ---------------------------------------------------------------- 6. determinism, checkpoints, metrics
@pytest.fixture(scope="module")
def small_rows():
    """1000 rows, d = 20, shape 2."""
    rng = np.random.default_rng(79)
    X = rng.uniform(-1.7, 1.7, (1000, 20))
    y = np.exp(0.5 + X @ rng.normal(0, 0.2, 20)) * rng.gamma(2.0, 0.5, 1000)
    return X, y


def test_gamma_deterministic_and_resumable(ctx, small_rows):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    X, y = small_rows
    cfg = dict(num_warmup=60, num_samples=60, chains=5, seed=31)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}]).set_prior(shape=(2.0, 0.5))
    mp = engine.Model(ctx, FAM, [{"x": X, "y": y}]).set_prior(shape=(2.0, 0.25))
    lin = engine.Model(ctx, "linear", [{"x": X, "y": np.log(y)}])          # the same x and log-y bits the sweeps read
    try:
        a = m.sample(**cfg)
        b = m.sample(**cfg)
        assert a.info["errors"] == 0
        assert np.array_equal(a.draws[0], b.draws[0]) and np.array_equal(a.stats[0], b.stats[0])
        s1 = m.sampler(**cfg)
        s1.run(40)
        blob = s1.save_state()
        s1.close()
        s2 = m.sampler(**cfg)                       # a fresh sampler of the same model
        s2.load_state(blob)
        s2.run()
        c = s2.result()
        s2.close()
        assert np.array_equal(a.draws[0], c.draws[0]) and np.array_equal(a.stats[0], c.stats[0])
        for other in (mp, lin):                     # the shape prior and the family are part of the state's geometry
            s3 = other.sampler(**cfg)
            before = s3.iterations().copy()
            with pytest.raises(StarkHipError) as e:
                s3.load_state(blob)
            assert e.value.code == -1
            assert np.array_equal(s3.iterations(), before)
            s3.close()
        assert not np.array_equal(mp.sample(**cfg).draws[0], a.draws[0])
    finally:
        m.close()
        mp.close()
        lin.close()


@pytest.mark.parametrize("metric,criterion", [("unit_e", "stan2.19"), ("unit_e", "stan2.23"), ("dense_e", "stan2.19"),
                                              ("dense_e", "stan2.23")])
def test_gamma_metrics_and_criteria_run(ctx, small_rows, metric, criterion):
    """unit_e and dense_e under both U-turn criteria produce finite draws; the fixed-step transition hook's lp is the
    reference's."""
    from stark_amd import engine
    X, y = small_rows
    m = engine.Model(ctx, FAM, [{"x": X[:500], "y": y[:500]}])
    try:
        res = m.sample(num_warmup=100, num_samples=50, chains=2, seed=8, metric=metric, nuts_criterion=criterion)
        assert res.info["errors"] == 0 and np.isfinite(res.draws[0]).all() and np.all(res.draws[0][21] > 0)
        q0 = np.zeros((2, 22))
        # the same effective step under both metrics: eps sqrt(0.01) = 0.005 (at q0 the gradient is of the size of n)
        im = np.eye(22) * 0.01 if metric == "dense_e" else None
        qn, lpn, _st = m.transition(0, q0, seed=3, iteration=0, eps=0.05 if metric == "dense_e" else 0.005, inv_metric=im)
        olp = R.ref_lpgrad(X[:500], y[:500], qn)[0].astype(np.float64)
        assert np.all(np.abs(lpn - olp) <= RTOL * np.maximum(np.abs(olp), 1.0))
        assert not np.array_equal(qn, q0)
    finally:
        m.close()


# ---------------------------------------------------------------- 7. the driver
def driver_rows():
    """1000 rows, d = 3, y = exp(0.5 + x . (0.8, -0.5, 0.3)) Gamma(2, 1/2)."""
    rng = np.random.default_rng(9)
    X = rng.uniform(-1.7, 1.7, (1000, 3))
    y = np.exp(0.5 + X @ [0.8, -0.5, 0.3]) * rng.gamma(2.0, 0.5, 1000)
    return [tuple(float(v) for v in X[i]) + (float(y[i]),) for i in range(1000)]


def test_gamma_through_the_driver(ctx):
    import os
    from stark_amd import engine, frontend, stark
    from stark_amd.rdd import LocalContext
    rows = driver_rows()

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": 3, "x": a[:, :3], "y": a[:, 3]}

    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize(rows, 4), prep)
    st.setStanModel(file=os.path.join(os.path.dirname(frontend.__file__), "models", "gamma_prior.stan"))
    assert st.family == FAM and st.priors == {"alpha": 10.0, "beta": 2.5, "shape": (2.0, 0.5)}
    out = st.concensusWeight(chains=4, iter=600, separate_lp=True, permuted=False, seed=21)
    assert out.shape == (6, 4 * 300)                                # alpha, beta[1..3], shape, lp__
    assert len(st.last_run.draws) == 4 and st.last_run.info["errors"] == 0
    ref, used = engine.consensus(st.last_run.draws, separate_lp=True)
    assert used.all() and np.array_equal(out, ref)
    est = out[:4].mean(1)
    print(f"gamma consensus alpha, beta {est}; shape {out[4].mean():.3f}")
    assert np.all(np.abs(est - [0.5, 0.8, -0.5, 0.3]) < 0.2), est
    assert 1.0 < out[4].mean() < 4.0
    semi = st.concensusWeight(chains=4, iter=600, permuted=False, seed=21, combiner="semiparametric")
    assert semi.shape[0] == 6 and np.isfinite(semi).all() and np.all(np.abs(semi[:4].mean(1) - [0.5, 0.8, -0.5, 0.3]) < 0.2)
    two = st.distribute(n=2, chains=2, iter=200, seed=22)
    assert two.shape == (2 * 6, 2 * 100)
    for call in (lambda: st.concensusWeight(chains=2, iter=100, seed=1, weights="laplace"),
                 lambda: st.concensusWeight(chains=2, iter=100, seed=1, method="laplace"),
                 lambda: st.waic(out), lambda: st.loo(out), lambda: st.ppc(out), lambda: st.bootstrap(n=4)):
        with pytest.raises(ValueError, match="gamma"):
            call()

    def prep_bad(part):
        dd = prep(part)
        dd["y"] = np.where(np.arange(len(part)) == 2, 0.0, dd["y"])
        return dd

    bad = stark.Stark(sc, sc.parallelize(rows, 4), prep_bad)
    bad.setStanModel(model_code=open(os.path.join(os.path.dirname(frontend.__file__), "models", "gamma.stan")).read())
    with pytest.raises(ValueError, match=r"y\[2\]"):
        bad.concensusWeight(chains=2, iter=100, seed=1)


# ---------------------------------------------------------------- 8. the refusals
def test_gamma_refusals(ctx, small_rows):
    """stk_model_create_synthetic, stk_sampler_set_allreduce and the six analysis sweeps refuse the family by name
    with STK_E_ARG; stk_model_create refuses a y that is not finite and > 0 and names the row; the shape prior's
    setter refuses another family by name."""
    import ctypes
    from stark_amd import _lib, engine
    from stark_amd._lib import StarkHipError
    with pytest.raises(StarkHipError) as e:
        engine.Model.synthetic(ctx, FAM, 1, 1000, 10)
    assert e.value.code == -1 and FAM in str(e.value)
    X, y = small_rows
    m = engine.Model(ctx, FAM, [{"x": X[:100], "y": y[:100]}])
    try:
        s = m.sampler(num_warmup=10, num_samples=10, chains=2, seed=1)
        with pytest.raises(StarkHipError) as e:
            s.set_allreduce(lambda ptr, count, stream: None)
        assert e.value.code == -1 and FAM in str(e.value)
        s.close()
        q = np.zeros((16, 22))
        for call in (lambda: m.hessian(0, q[0]), lambda: m.log_predictive(q), lambda: m.loo(q),
                     lambda: m.log_density(q, 0), lambda: m.log_density_grad_boot(q, 0, seed=1),
                     lambda: m.posterior_predict(q, seed=1)):
            with pytest.raises(StarkHipError) as e:
                call()
            assert e.value.code == -1 and FAM in str(e.value), str(e.value)
        assert m.log_density_grad(0, q)[0].shape == (16,)
    finally:
        m.close()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        yb = y[:100].copy()
        yb[37] = bad
        with pytest.raises(StarkHipError) as e:
            engine.Model(ctx, FAM, [{"x": X[:100], "y": y[:100]}, {"x": X[:100], "y": yb}])
        assert e.value.code == -1 and "shard 1" in str(e.value) and "y[37]" in str(e.value), str(e.value)
    lin = engine.Model(ctx, "linear", [{"x": X[:100], "y": y[:100]}])
    try:
        assert _lib.load().stk_model_set_prior_shape(lin._h, 2.0, 0.5) == -1
        assert "linear" in _lib.load().stk_last_error().decode()
        with pytest.raises(StarkHipError) as e:
            lin.set_prior(shape=(2.0, 0.5))
        assert e.value.code == -1
    finally:
        lin.close()
    out = (ctypes.c_double * 2)()
    assert _lib.load().stk_gamma_shape_terms_host(2.0, out) == 0 and out[1] > 0
    assert _lib.load().stk_gamma_shape_terms_host(2.0, None) == -1
