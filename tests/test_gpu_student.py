"""The Student-t (student_t) family on the GPU: every sweep's lp / gradient against the longdouble reference
tests/student_ref.py (the density of include/stark_hip.h, STK_STUDENT) at nu = 1, 4 and 1e6, the nu = 1e6 density
against the linear family's, extreme residuals, priors, chain batches and grouped launches, the data round trip,
sampling against an exact grid posterior, determinism and checkpoints, the metrics and U-turn criteria, the Stark
driver on data with gross outliers, and the family's refusals.

Bars: check_bars of tests/test_gpu_negbin.py (the project's 1e-10 density bars), restated here.

Inputs.  X, alpha and beta are dyadic (X multiples of 2^-6 in [-1.7, 1.7], the coefficients multiples of 2^-10), so
every product x_ij beta_j and every partial sum of eta is exact in fp64 whatever the order of the sum: eta reaches
the residual without rounding error, on the device as in the reference.  That is needed for the bars to be a test
of the kernels at all: d (d lp / d eta) / d eta is (nu + 1) / (nu sigma^2) at |z| < sqrt(nu), 2e6 at nu = 1 and
sigma = 1e-3, so one ulp of an eta of size 1 moves such a row's gradient term by 4e-10 while the bar for a small
component is 1e-13 (max |g| + 1): with arbitrary doubles an fp64 dot product over d = 1024 columns misses the bars
by a factor of 3 on a few (shape, chain) pairs whatever the residual code does (measured with numpy in place of
the kernels).  y, the noise, the outliers and s are arbitrary doubles.
"""
import numpy as np
import pytest

import student_ref as R

pytestmark = pytest.mark.gpu

FAM = "student_t"
RTOL = 1e-10
NUS = [1.0, 4.0, 1e6]


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


A0 = 0.2998046875        # 307 / 1024


def dyadic(v, bits):
    return np.round(np.asarray(v) * 2.0 ** bits) / 2.0 ** bits


def make_data(n, d, seed=None):
    """X ~ U(-1.7, 1.7) and beta ~ N(0, 1/sqrt(d)), dyadic; y = A0 + X beta + t_4 noise (sigma = 1); rows 1 ..
    max(1, n/50) displaced by +-1e3 sigma (alternating signs); row 0 has x = 0 and y = A0, so it sits exactly on the
    fit of every point whose alpha is A0 (z = 0 to the bit: eta = alpha there)."""
    rng = np.random.default_rng(n * 1000 + d if seed is None else seed)
    X = dyadic(rng.uniform(-1.7, 1.7, (n, d)), 6)
    X[0] = 0.0
    beta = dyadic(rng.normal(0, 1 / np.sqrt(d), d), 10)
    y = A0 + X @ beta + rng.standard_t(4, n)
    k = min(max(1, n // 50), n - 1)
    y[1:1 + k] += 1e3 * np.where(np.arange(k) % 2 == 0, 1.0, -1.0)
    y[0] = A0
    return rng, X, y, beta


def points(rng, beta, C, d, lo=1e-3, hi=1e3):
    """C points (alpha, beta, s): point 0 the data's own coefficients (row 0 on the fit), the others within N(0, 0.2)
    of them, dyadic; s spread log-uniformly over sigma in [lo, hi] across the chains (C = 1: sigma = 1)."""
    q = rng.normal(0, 0.2, (C, d + 2))
    q[:, 0] += A0
    q[:, 1:d + 1] += beta
    q[0, :d + 1] = np.concatenate([[A0], beta])
    q[:, :d + 1] = dyadic(q[:, :d + 1], 10)
    q[:, -1] = 0.0 if C == 1 else np.log(lo) + np.log(hi / lo) * np.arange(C) / (C - 1)
    return q


VALU = [(1, 1, 1), (7, 3, 5), (65, 104, 3), (3000, 120, 5), (333, 129, 5), (257, 300, 8)]
S16 = [(1, 1, 16), (7, 3, 16), (300, 113, 16), (333, 128, 16), (4097, 50, 16), (65, 104, 20)]
S16W = [(333, 129, 16), (257, 512, 16), (130, 1023, 16), (200, 1024, 16)]
G64 = [(1, 1, 64), (300, 17, 64), (333, 129, 64), (200, 1024, 64), (130, 1001, 70)]


# ---------------------------------------------------------------- 1. every sweep against the reference
@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("n,d,C", VALU + S16 + S16W + G64)
def test_student_lpgrad(ctx, n, d, C, nu):
    """VALU sweeps (k_sweep3, k_sweep2, k_sweep at odd and wide d), k_sweep16 (masked last sub-tile, the VALU last
    tile, beta in registers or not, several chunks, 16 + 4), k_sweep16w and the 64-chain passes (64 + 4 + 2), each
    with the third partial column and the family's reduce.  Two shards, the first a third of the rows; the second is
    evaluated.  Outliers at 1e3 sigma of the data, z up to 1e6 at the chains with sigma = 1e-3; row 0 at z = 0.
    nu = 1e6: also against the LINEAR family's longdouble density.  Per row (nu + 1)/2 log1p(w) - nu w / 2 lies in
    [-(nu + 1) w^2 / 4, w / 2] (w - w^2 / 2 <= log1p(w) <= w), so the two lp differ by at most
    n (w_max / 2 + (nu + 1) w_max^2 / 4) with w_max the point's largest z^2 / nu: the bar is that plus the
    density bar."""
    from stark_amd import engine
    rng, X, y, beta = make_data(n, d)
    k = max(1, n // 3)
    m = engine.Model(ctx, FAM, [{"x": X[:k], "y": y[:k]}, {"x": X, "y": y}], nu=nu)
    try:
        assert m.D == [d + 2, d + 2] and m.P == [d + 3, d + 3] and m.n_rows == [k, n] and m.nu == nu
        q = points(rng, beta, C, d)
        lp, g = m.log_density_grad(1, q)
    finally:
        m.close()
    olp, og = R.ref_lpgrad(X, y, q, nu)
    assert np.all(np.isfinite(olp.astype(np.float64))) and np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    wl, wg = check_bars(lp, g, olp, og, (n, d, C, nu))
    print(f"student_t {(n, d, C)} nu={nu:g}: lp {wl:.2e} gradient {wg:.2e} of the bars")
    if nu == 1e6:
        lin = R.ref_linear_lp(X, y, q).astype(np.float64)
        wmax = R.max_w(X, y, q, nu)[0].astype(np.float64)
        bound = n * (wmax / 2 + (nu + 1) * wmax * wmax / 4) + RTOL * np.maximum(np.abs(lin), 1.0)
        assert np.all(np.abs(lp - lin) <= bound), (n, d, C, float((np.abs(lp - lin) / bound).max()))
        assert np.any(bound < 1e-3 * np.maximum(np.abs(lin), 1.0)) or C == 1   # the bound bites at the large-sigma chains


# ---------------------------------------------------------------- 2. extreme residuals
SHAPES_X = [(300, 113, 16), (500, 100, 64), (400, 60, 4), (300, 200, 16), (257, 131, 3)]


def extreme_points(n, d, C, scale):
    """Every point's (alpha, beta) times `scale`; sigma log-uniform over [1e-3, 1e3] across the chains, at 1e150
    over [1e-6, 1e3]: z^2 passes the largest double where sigma is below about 2e-4, a quarter of the range."""
    rng, X, y, beta = make_data(n, d, seed=int(scale) % 1000 + n)
    q = points(rng, beta, C, d, lo=1e-6 if scale == 1e150 else 1e-3)
    q[:, : d + 1] *= scale
    return X, y, q


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("scale", [30.0, 1e3, 1e150])
@pytest.mark.parametrize("n,d,C", SHAPES_X)
def test_student_lpgrad_extreme(ctx, scale, n, d, C, nu):
    """At 30 and 1e3 every point is finite and within the bars.  At 1e150 a point may be non-finite only where some
    row's z^2 passes the largest double; it is never +inf, and a finite point meets the bars; the reference alone
    says which points those are, and at least half of them are not."""
    from stark_amd import engine
    X, y, q = extreme_points(n, d, C, scale)
    olp, og = R.ref_lpgrad(X, y, q, nu)
    over = R.max_w(X, y, q, nu)[1]
    assert np.all(np.isfinite(olp.astype(np.float64))) and np.all(np.isfinite(og.astype(np.float64)))
    assert 2 * int((~over).sum()) >= C, (C, int(over.sum()))
    assert scale == 1e150 or not over.any()
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}], nu=nu)
    try:
        lp, g = m.log_density_grad(0, q)
    finally:
        m.close()
    assert not np.any(lp == np.inf), lp
    fin = np.isfinite(lp)
    assert np.all(fin[~over]), (scale, n, d, C, lp[~over])
    assert np.all(np.isfinite(g[fin])), (scale, n, d, C)
    idx = np.flatnonzero(fin)
    check_bars(lp[idx], g[idx], olp[idx], og[idx], (scale, n, d, C, nu))


# ---------------------------------------------------------------- 3. priors
@pytest.mark.parametrize("n,d,C", [(300, 113, 16), (257, 100, 2), (300, 17, 64)])
def test_student_priors(ctx, n, d, C):
    from stark_amd import engine
    rng, X, y, beta = make_data(n, d)
    q = points(rng, beta, C, d)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}], nu=4.0)
    try:
        lp0, g0 = m.log_density_grad(0, q)
        m.set_prior(alpha=2.0, beta=0.5)
        lp1, g1 = m.log_density_grad(0, q)
        m.set_prior()                                              # flat again
        lp2, g2 = m.log_density_grad(0, q)
    finally:
        m.close()
    check_bars(lp0, g0, *R.ref_lpgrad(X, y, q, 4.0), where="flat")
    check_bars(lp1, g1, *R.ref_lpgrad(X, y, q, 4.0, prior=(2.0, 0.5)), where="normal priors")
    assert np.array_equal(lp0, lp2) and np.array_equal(g0, g2) and np.all(lp1 < lp0)


# ---------------------------------------------------------------- 4. batches and grouped launches
def test_student_chain_batches_and_shards_bitwise(ctx):
    """chains = 16 + 4 + 1 and 64 + 4 + 2 are the single launches of their batches, bit for bit; every shard at once
    is the per-shard calls, bit for bit."""
    from stark_amd import engine
    shards = []
    for s in range(3):
        _rng, X, y, _beta = make_data(600, 100, seed=50 + s)
        shards.append({"x": X, "y": y})
    rng = np.random.default_rng(5)
    m = engine.Model(ctx, FAM, shards, nu=4.0)
    try:
        for C in (21, 70):
            assert engine.chain_batches(C, 100) == ([16, 4, 1] if C == 21 else [64, 4, 2])
            q = rng.normal(0, 0.2, (3, C, 102))
            q[:, :, -1] = rng.uniform(-3, 3, (3, C))
            lp, g = m.log_density_grad_chains(q)
            c0 = 0
            for b in engine.chain_batches(C, 100):
                blp, bg = m.log_density_grad_shards(np.ascontiguousarray(q[:, c0:c0 + b]))
                assert np.array_equal(lp[:, c0:c0 + b], blp) and np.array_equal(g[:, c0:c0 + b], bg), (C, c0, b)
                c0 += b
            assert c0 == C
        q = rng.normal(0, 0.2, (3, 16, 102))
        lp, g = m.log_density_grad_shards(q)
        for s in range(3):
            slp, sg = m.log_density_grad(s, q[s])
            assert np.array_equal(lp[s], slp) and np.array_equal(g[s], sg), s
            olp = R.ref_lpgrad(shards[s]["x"], shards[s]["y"], q[s], 4.0)[0].astype(np.float64)
            assert np.all(np.abs(slp - olp) <= RTOL * np.maximum(np.abs(olp), 1.0))
    finally:
        m.close()


# ---------------------------------------------------------------- 5. the data round trip and the fingerprint
def test_student_model_data_round_trip(ctx):
    """copy_data returns the rows; the device fingerprint is the host twin's.  The family word is part of the
    fingerprint today (include/stark_hip.h: words([family, n_rows, n_cols], 0, 0)), so the same rows as a "linear"
    model fingerprint differently; nu is not part of it (the saved state's geometry covers it)."""
    from stark_amd import engine
    _rng, X, y, _beta = make_data(300, 7)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}], nu=4.0)
    m5 = engine.Model(ctx, FAM, [{"x": X, "y": y}], nu=5.0)
    lin = engine.Model(ctx, "linear", [{"x": X, "y": y}])
    try:
        back = m.copy_data(0)
        assert back["y"].dtype == np.float64 and np.array_equal(back["y"], y) and np.array_equal(back["x"], X)
        arr = m.device_arrays(0)
        assert set(arr) == {"x", "y"} and arr["x"][1] == 300 * 7 and arr["y"][1] == 300
        fp = int(m.fingerprint(0))
        assert fp == int(engine.shard_fingerprint(FAM, {"x": X, "y": y}))
        assert fp != int(lin.fingerprint(0)) and int(lin.fingerprint(0)) == int(engine.shard_fingerprint("linear", {"x": X, "y": y}))
        assert fp == int(m5.fingerprint(0))
        assert fp != int(engine.shard_fingerprint(FAM, {"x": X, "y": np.where(np.arange(300) == 5, y + 1, y)}))
    finally:
        m.close()
        m5.close()
        lin.close()


# ---------------------------------------------------------------- 6. sampling against an exact posterior
def grid_data():
    rng = np.random.default_rng(404)
    x = rng.uniform(-1.7, 1.7, 40)
    y = 0.5 + 0.8 * x + 0.6 * rng.standard_t(4, 40)
    y[3] += 25.0                                                   # the two outliers
    y[17] -= 25.0
    return x, y


@pytest.fixture(scope="module")
def grid_posterior():
    """n = 40, d = 1, nu = 4, y = 0.5 + 0.8 x + 0.6 t_4 with two outliers at +-25, flat priors: the posterior of
    (alpha, beta, s) on a 121 x 121 x 161 tensor grid over alpha 0.5 +- 2, beta 0.8 +- 2, s in log 0.6 + [-2, 3],
    from student_ref's formulas in fp64.  Its every-other-point subgrid must agree to 1e-9 relative on all six
    moments, the mass on the grid's faces must be below 1e-12, and the grid has one local maximum (6 neighbours)."""
    x, y = grid_data()
    a = 0.5 + np.linspace(-2.0, 2.0, 121)
    b = 0.8 + np.linspace(-2.0, 2.0, 121)
    s = np.log(0.6) + np.linspace(-2.0, 3.0, 161)
    r = y[None, None, :] - a[:, None, None] - b[None, :, None] * x[None, None, :]
    r2 = r * r
    lp = np.empty((121, 121, 161))
    for k, sk in enumerate(s):
        lp[:, :, k] = -2.5 * np.log1p(r2 * (np.exp(-2 * sk) / 4.0)).sum(2) - 40 * sk + sk
    q = np.array([[a[60], b[60], s[64]], [a[3], b[100], s[150]]])
    olp = R.ref_lpgrad(x[:, None], y, q, 4.0)[0].astype(np.float64)
    assert np.allclose([lp[60, 60, 64], lp[3, 100, 150]], olp, rtol=1e-12)           # the grid is the reference's density

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

    fine, face = moments(lp, (a, b, s))
    coarse, _ = moments(lp[::2, ::2, ::2], (a[::2], b[::2], s[::2]))
    assert face < 1e-12, face
    assert np.all(np.abs(coarse - fine) <= 1e-9 * np.abs(fine)), (coarse, fine)
    p = np.pad(lp, 1, constant_values=-np.inf)
    peak = np.ones(lp.shape, bool)
    for ax in range(3):
        for sh in (1, -1):
            peak &= lp >= np.roll(p, sh, axis=ax)[1:-1, 1:-1, 1:-1]
    assert int(peak.sum()) == 1, np.argwhere(peak)
    return x, y, fine[:, 0].copy(), fine[:, 1].copy()


@pytest.mark.parametrize("metric", ["diag_e", "dense_e"])
@pytest.mark.parametrize("chains", [16, 3])
def test_student_sampling_exact(ctx, grid_posterior, chains, metric):
    """test_negbin_sampling_exact's criterion for alpha, beta and s = log sigma: four-sigma bars from the run's own
    effective sizes, |mean - exact| <= 4 sd / sqrt(n_eff) and |var / exact - 1| <= 4 sqrt(2 / n_eff2), n_eff2 the
    n_eff of the centred squares; no divergences; the lp__ row is the reference density at the drawn point."""
    from stark_amd import diagnostics, engine
    x, y, mean, var = grid_posterior
    X = x[:, None].copy()
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}], nu=4.0)
    try:
        res = m.sample(num_warmup=300, num_samples=1000, chains=chains, seed=4600 + chains, metric=metric)
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
    olp = R.ref_lpgrad(X, y, np.ascontiguousarray(par.T), 4.0)[0].astype(np.float64)
    assert np.all(np.abs(dr[3] - olp) <= RTOL * np.maximum(np.abs(olp), 1.0))


# ---------------------------------------------------------------- 7. determinism, checkpoints, metrics
@pytest.fixture(scope="module")
def small_rows():
    """1000 rows, d = 20, t_4 noise, 2 % outliers."""
    rng = np.random.default_rng(78)
    X = rng.uniform(-1.7, 1.7, (1000, 20))
    y = 0.5 + X @ rng.normal(0, 0.2, 20) + 0.7 * rng.standard_t(4, 1000)
    y[:20] += 30.0
    return X, y


def test_student_deterministic_and_resumable(ctx, small_rows):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    X, y = small_rows
    cfg = dict(num_warmup=60, num_samples=60, chains=5, seed=31)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}], nu=4.0)
    m5 = engine.Model(ctx, FAM, [{"x": X, "y": y}], nu=5.0)
    lin = engine.Model(ctx, "linear", [{"x": X, "y": y}])
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
        for other in (m5, lin):                     # nu and the family are part of the state's geometry
            s3 = other.sampler(**cfg)
            before = s3.iterations().copy()
            with pytest.raises(StarkHipError) as e:
                s3.load_state(blob)
            assert e.value.code == -1
            assert np.array_equal(s3.iterations(), before)
            s3.close()
        assert not np.array_equal(m5.sample(**cfg).draws[0], a.draws[0])
    finally:
        m.close()
        m5.close()
        lin.close()


@pytest.mark.parametrize("metric,criterion", [("unit_e", "stan2.19"), ("unit_e", "stan2.23"), ("dense_e", "stan2.23"),
                                              ("diag_e", "stan2.23")])
def test_student_metrics_and_criteria_run(ctx, small_rows, metric, criterion):
    """unit_e and both U-turn criteria produce finite draws; the fixed-step transition hook's lp is the reference's."""
    from stark_amd import engine
    X, y = small_rows
    m = engine.Model(ctx, FAM, [{"x": X[:500], "y": y[:500]}], nu=4.0)
    try:
        res = m.sample(num_warmup=100, num_samples=50, chains=2, seed=8, metric=metric, nuts_criterion=criterion)
        assert res.info["errors"] == 0 and np.isfinite(res.draws[0]).all() and np.all(res.draws[0][21] > 0)
        q0 = np.zeros((2, 22))
        im = np.eye(22) * 0.01 if metric == "dense_e" else (None if metric == "unit_e" else np.full(22, 0.01))
        qn, lpn, _st = m.transition(0, q0, seed=3, iteration=0, eps=0.05, inv_metric=im)
        olp = R.ref_lpgrad(X[:500], y[:500], qn, 4.0)[0].astype(np.float64)
        assert np.all(np.abs(lpn - olp) <= RTOL * np.maximum(np.abs(olp), 1.0))
        assert not np.array_equal(qn, q0)
    finally:
        m.close()


# ---------------------------------------------------------------- 8. the driver
PROGRAM = """
data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; vector[N] y; real<lower=0> nu; }
parameters { real alpha; vector[K] beta; real<lower=0> sigma; }
model { y ~ student_t(nu, alpha + x * beta, sigma); }
"""
LINEAR = """
data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; vector[N] y; }
parameters { real alpha; vector[K] beta; real<lower=0> sigma; }
model { y ~ normal(alpha + x * beta, sigma); }
"""


def driver_rows():
    """2000 rows, y = 0.5 + 0.8 x + 0.5 t_4; the 5 % of rows with the largest x are displaced by +20 (40 sigma).
    On the CPU (least squares; an EM fit of the t_4 regression): the linear fit's beta is 2.49, 18 of its posterior
    sd (0.094) from 0.8; the Student-t fit's is 0.8001, 0.01 of its sd (0.017) from it."""
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.7, 1.7, 2000)
    y = 0.5 + 0.8 * x + 0.5 * rng.standard_t(4, 2000)
    y[np.argsort(x)[-100:]] += 20.0
    order = rng.permutation(2000)                                   # every partition gets its share of the outliers
    return [(float(x[i]), float(y[i])) for i in order]


def test_student_through_the_driver(ctx):
    """The user-visible point of the family: on data with 5 % gross outliers the consensus mean of beta is within its
    posterior sd of the truth under student_t and more than 5 sd off under the linear family on the same rows."""
    from stark_amd import engine, stark
    from stark_amd.rdd import LocalContext
    rows = driver_rows()

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": 1, "x": a[:, :1], "y": a[:, 1], "nu": 4.0}

    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize(rows, 4), prep)
    st.setStanModel(model_code=PROGRAM)
    assert st.family == FAM and st.priors == {}
    out = st.concensusWeight(chains=4, iter=600, separate_lp=True, permuted=False, seed=21)
    assert out.shape == (4, 4 * 300)                                # alpha, beta, sigma, lp__
    assert len(st.last_run.draws) == 4 and st.last_run.info["errors"] == 0
    ref, used = engine.consensus(st.last_run.draws, separate_lp=True)
    assert used.all() and np.array_equal(out, ref)
    bm, bs = out[1].mean(), out[1].std()
    print(f"student_t consensus beta {bm:.4f} sd {bs:.4f}; sigma {out[2].mean():.3f}")
    assert abs(bm - 0.8) < bs, (bm, bs)
    semi = st.concensusWeight(chains=4, iter=600, permuted=False, seed=21, combiner="semiparametric")
    assert semi.shape[0] == 4 and np.isfinite(semi).all() and abs(semi[1].mean() - 0.8) < 3 * bs
    two = st.distribute(n=2, chains=2, iter=200, seed=22)
    assert two.shape == (2 * 4, 2 * 100)

    def prep_lin(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": 1, "x": a[:, :1], "y": a[:, 1]}

    lin = stark.Stark(sc, sc.parallelize(rows, 4), prep_lin)
    lin.setStanModel(model_code=LINEAR)
    lo = lin.concensusWeight(chains=4, iter=600, separate_lp=True, permuted=False, seed=21)
    lm, ls = lo[1].mean(), lo[1].std()
    print(f"linear consensus beta {lm:.4f} sd {ls:.4f}")
    assert abs(lm - 0.8) > 5 * ls, (lm, ls)

    def prep_bad(part):
        d = prep(part)
        d["nu"] = 4.0 if part[0] == rows[0] else 5.0
        return d

    bad = stark.Stark(sc, sc.parallelize(rows, 4), prep_bad)
    bad.setStanModel(model_code=PROGRAM)
    with pytest.raises(ValueError, match="nu differ"):
        bad.concensusWeight(chains=2, iter=100, seed=1)


# ---------------------------------------------------------------- 9. the refusals
def test_student_refusals(ctx, small_rows):
    """stk_model_create_synthetic, stk_sampler_set_allreduce and the six analysis sweeps refuse the family by name
    with STK_E_ARG; a model whose nu is not set refuses the density hooks, the transition and the sampler; a bad nu
    is refused with its value; the nu setter refuses another family by name."""
    import ctypes
    from stark_amd import _lib, engine
    from stark_amd._lib import StarkHipError
    with pytest.raises(StarkHipError) as e:
        engine.Model.synthetic(ctx, FAM, 1, 1000, 10)
    assert e.value.code == -1 and FAM in str(e.value)
    X, y = small_rows
    m = engine.Model(ctx, FAM, [{"x": X[:100], "y": y[:100]}], nu=4.0)
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
        lib = _lib.load()
        for bad in (0.0, -2.0, float("inf"), float("nan")):
            assert lib.stk_model_set_student_nu(m._h, bad) == -1
            msg = lib.stk_last_error().decode()
            assert "nu must be finite and > 0" in msg and ("%g" % bad) in msg, msg
        assert m.log_density_grad(0, q)[0].shape == (16,)           # the refused values changed nothing
    finally:
        m.close()
    for bad in (None, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            engine.Model(ctx, FAM, [{"x": X[:100], "y": y[:100]}], nu=bad)
    with pytest.raises(ValueError, match="linear"):
        engine.Model(ctx, "linear", [{"x": X[:100], "y": y[:100]}], nu=4.0)
    lin = engine.Model(ctx, "linear", [{"x": X[:100], "y": y[:100]}])
    try:
        assert _lib.load().stk_model_set_student_nu(lin._h, 4.0) == -1
        assert "linear" in _lib.load().stk_last_error().decode()
    finally:
        lin.close()
    # nu not set: straight through the C ABI (engine.Model always sets it)
    lib = _lib.load()
    xs, ys = np.ascontiguousarray(X[:100]), np.ascontiguousarray(y[:100])
    sh = (_lib.Shard * 1)(_lib.Shard(100, 20, xs.ctypes.data, ys.ctypes.data, None, None))
    h = ctypes.c_void_p()
    assert lib.stk_model_create(ctx._h, 6, sh, 1, ctypes.byref(h)) == 0
    try:
        q = np.zeros((4, 22))
        lp, g = np.zeros(4), np.zeros((4, 22))
        cfg = _lib.Config()
        lib.stk_config_default(ctypes.byref(cfg))
        cfg.num_warmup, cfg.num_samples, cfg.chains = 5, 5, 2
        sp = ctypes.c_void_p()
        calls = (lambda: lib.stk_log_density_grad(h, 0, q.ctypes.data, 4, lp.ctypes.data, g.ctypes.data),
                 lambda: lib.stk_log_density_grad_shards(h, q.ctypes.data, 4, lp.ctypes.data, g.ctypes.data),
                 lambda: lib.stk_log_density_grad_chains(h, q.ctypes.data, 4, lp.ctypes.data, g.ctypes.data),
                 lambda: lib.stk_sampler_create(h, ctypes.byref(cfg), ctypes.byref(sp)),
                 lambda: lib.stk_transition(h, 0, q.ctypes.data, 4, 1, 0, 0.05, None, 5, lp.ctypes.data, None))
        for call in calls:
            assert call() == -1
            assert "nu has not been set" in lib.stk_last_error().decode()
        assert lib.stk_model_set_student_nu(h, 4.0) == 0
        assert calls[0]() == 0 and np.isfinite(lp).all()
    finally:
        lib.stk_model_destroy(h)
