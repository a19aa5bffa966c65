"""The Poisson (poisson_log) family on the GPU: every sweep's lp / gradient against a numpy restatement
of the density in np.longdouble, extreme eta, priors, the y >= 0 check, chain batches and grouped
launches, sampling against an exact grid posterior, determinism and checkpoints, the Stark driver
and the family's two refusals.

The reference (include/stark_hip.h; Stan 2.19's poisson_log_lpmf<propto = true>): with
eta = alpha + x . beta and mu = exp(eta),
    lp = sum(y eta - mu) - (pa alpha^2 + pb |beta|^2) / 2,   pa, pb = 1 / s^2 of the normal(0, s) priors
    d lp / d alpha = sum(y - mu) - pa alpha,   d lp / d beta = x^T (y - mu) - pb beta.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-10
DBL_MAX = np.finfo(np.float64).max


def ref_lpgrad(X, y, q, prior=(0.0, 0.0)):
    """lp (C,) and gradient (C, d + 1) at the rows of q, in np.longdouble; a mu past the largest
    double is +inf, as the exp of the fp64 kernels overflows there."""
    L = np.longdouble
    Xl, yl, ql = X.astype(L), y.astype(L)[:, None], q.astype(L)
    pa, pb = (0.0 if s in (0.0, None) else 1.0 / (L(s) * L(s)) for s in prior)
    with np.errstate(over="ignore", invalid="ignore"):
        eta = ql[:, 0][None, :] + Xl @ ql[:, 1:].T                 # (n, C)
        mu = np.exp(eta)
        mu[mu > DBL_MAX] = np.inf
        lp = (yl * eta - mu).sum(0) - 0.5 * (pa * ql[:, 0] ** 2 + pb * (ql[:, 1:] ** 2).sum(1))
        r = yl - mu
        g = np.concatenate([r.sum(0)[:, None] - pa * ql[:, :1], r.T @ Xl - pb * ql[:, 1:]], axis=1)
    return lp, g


def make_data(n, d, seed=None):
    """X ~ U(-1.7, 1.7), beta ~ N(0, 1/sqrt(d)), eta = 0.3 + X beta with the first max(1, n/50) rows'
    eta times 6, clipped to +-20; y ~ Poisson(exp(eta)): counts from 0 to ~5e8 (past 2^24), and one
    count of 2^31 - 1 set by hand where n >= 64."""
    rng = np.random.default_rng(n * 1000 + d if seed is None else seed)
    X = rng.uniform(-1.7, 1.7, (n, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    eta = 0.3 + X @ beta
    eta[: max(1, n // 50)] *= 6.0
    eta = np.clip(eta, -20.0, 20.0)
    y = rng.poisson(np.exp(eta)).astype(np.int64)
    if n >= 64:
        y[n // 2] = 2 ** 31 - 1
    assert y.min() >= 0 and y.max() <= 2 ** 31 - 1
    return rng, X, y.astype(np.int32), beta


def check_bars(lp, g, olp, og, where=""):
    """test_regression_lpgrad's bars: lp within 1e-10 of max(|lp|, 1); every gradient component
    within 1e-10 of max(|g_j|, 1e-3 (max |g| + 1))."""
    for c in range(len(olp)):
        o = np.float64(olp[c])
        elp = abs(lp[c] - o) / max(abs(o), 1.0)
        ogc = og[c].astype(np.float64)
        bar = RTOL * np.maximum(np.abs(ogc), (np.abs(ogc).max() + 1.0) * 1e-3)
        eg = np.abs(g[c] - ogc)
        assert elp < RTOL, (where, c, lp[c], o, elp)
        assert np.all(eg <= bar), (where, c, float((eg / bar).max()))


VALU = [(1, 1, 1), (7, 3, 5), (1000, 100, 1), (777, 100, 2), (20000, 100, 4), (65, 104, 3), (3000, 120, 5),
        (333, 129, 5), (257, 300, 8), (5000, 2, 4)]
S16 = [(1, 1, 16), (7, 3, 16), (1000, 100, 16), (4097, 50, 16), (333, 128, 16), (300, 99, 16), (300, 113, 16),
       (64, 110, 16), (100, 29, 16), (100003, 100, 16), (65, 104, 20)]
S16W = [(333, 129, 16), (150, 200, 16), (257, 512, 16), (130, 1023, 16), (200, 1024, 16)]
G64 = [(1, 1, 64), (7, 3, 64), (300, 16, 64), (300, 17, 64), (4097, 50, 64), (333, 129, 64), (5000, 100, 64),
       (200, 1024, 64), (130, 1001, 70)]


# ---------------------------------------------------------------- 1. every sweep against the reference
@pytest.mark.parametrize("n,d,C", VALU + S16 + S16W + G64)
def test_poisson_lpgrad(ctx, n, d, C):
    """VALU sweeps (k_sweep3's one tile, partial tile and many chunks; k_sweep2; k_sweep at odd and wide
    d), k_sweep16 (masked last sub-tile, the VALU last tile, beta in registers past d = 108, the clamped
    backward column, several chunks, 16 + 4), k_sweep16w, and the 64-chain passes (one and two pass-F
    stages per tile, the parked tile's epilogue across tile ends, 64 + 4 + 2).  Two shards, the first a
    third of the rows; the second is evaluated."""
    from stark_amd import engine
    rng, X, y, beta = make_data(n, d)
    k = max(1, n // 3)
    m = engine.Model(ctx, "poisson", [{"x": X[:k], "y": y[:k]}, {"x": X, "y": y}])
    try:
        assert m.D == [d + 1, d + 1] and m.P == [d + 2, d + 2] and m.n_rows == [k, n]
        q = rng.normal(0, 0.2, (C, d + 1))
        q[0] = np.concatenate([[0.3], 3 * beta])
        if C > 1:
            q[1, 1:] = 12 * beta                    # |eta| up to ~45
        lp, g = m.log_density_grad(1, q)
    finally:
        m.close()
    olp, og = ref_lpgrad(X, y, q)
    assert np.all(np.isfinite(olp.astype(np.float64)))
    check_bars(lp, g, olp, og, (n, d, C))


# ---------------------------------------------------------------- 2. extreme eta
@pytest.mark.parametrize("scale", [30.0, 1e3, 1e8, 1e150])
@pytest.mark.parametrize("n,d,C", [(2000, 100, 16), (300, 113, 16), (500, 100, 64), (400, 60, 4), (300, 200, 16)])
def test_poisson_lpgrad_extreme_eta(ctx, scale, n, d, C):
    """Half of the points scaled by 30 .. 1e150: where the reference lp is finite the bars of test 1
    hold (at scale 30 every point is: the table exp's accuracy at large |eta|); where a row's exp
    overflows, lp is -inf or NaN on the GPU too -- never finite, never +inf."""
    from stark_amd import engine
    rng, X, y, _beta = make_data(n, d, seed=int(scale) % 1000 + n)
    q = rng.normal(0, 1.0 / np.sqrt(d), (C, d + 1))
    q[: C // 2] *= scale
    m = engine.Model(ctx, "poisson", [{"x": X, "y": y}])
    try:
        lp, g = m.log_density_grad(0, q)
    finally:
        m.close()
    olp, og = ref_lpgrad(X, y, q)
    with np.errstate(over="ignore"):
        fin = np.isfinite(olp.astype(np.float64)) & np.all(np.isfinite(og.astype(np.float64)), axis=1)
    if scale == 30.0:
        assert fin.all()
    assert fin[C // 2:].all()
    idx = np.flatnonzero(fin)
    check_bars(lp[idx], g[idx], olp[idx], og[idx], (scale, n, d, C))
    bad = np.flatnonzero(~fin)
    assert not np.any(np.isfinite(lp[bad])) and not np.any(lp[bad] == np.inf), (scale, lp[bad])


# ---------------------------------------------------------------- 3. priors
@pytest.mark.parametrize("n,d,C", [(1000, 100, 16), (777, 100, 2)])
def test_poisson_priors(ctx, n, d, C):
    from stark_amd import engine
    rng, X, y, beta = make_data(n, d)
    q = rng.normal(0, 0.2, (C, d + 1))
    q[0] = np.concatenate([[0.3], 3 * beta])
    m = engine.Model(ctx, "poisson", [{"x": X, "y": y}])
    try:
        lp0, g0 = m.log_density_grad(0, q)
        m.set_prior(alpha=2.0, beta=0.5)
        lp, g = m.log_density_grad(0, q)
    finally:
        m.close()
    check_bars(lp0, g0, *ref_lpgrad(X, y, q), where="flat")
    check_bars(lp, g, *ref_lpgrad(X, y, q, prior=(2.0, 0.5)), where="prior")
    assert np.all(lp < lp0)


# ---------------------------------------------------------------- 4. bad data
def test_poisson_negative_count_refused(ctx):
    """stk_model_create names the first row with y_int < 0 (the Python layers refuse it earlier, so this
    goes through the C ABI)."""
    from stark_amd import _lib
    lib = _lib.load()
    x = np.zeros((100, 2))
    y = np.arange(100, dtype=np.int32)
    y[17] = -3
    y[60] = -1
    sh = (_lib.Shard * 1)(_lib.Shard(100, 2, x.ctypes.data, None, y.ctypes.data, None))
    h = ctypes.c_void_p()
    assert lib.stk_model_create(ctx._h, 4, sh, 1, ctypes.byref(h)) == -1          # STK_E_ARG
    msg = lib.stk_last_error().decode()
    assert "y_int[17] = -3" in msg and "poisson_log needs y >= 0" in msg, msg
    y[17], y[60] = 17, 60
    assert lib.stk_model_create(ctx._h, 4, sh, 1, ctypes.byref(h)) == 0
    lib.stk_model_destroy(h)
    sh[0].y_int = None
    assert lib.stk_model_create(ctx._h, 4, sh, 1, ctypes.byref(h)) == -1
    assert "poisson needs y_int" in lib.stk_last_error().decode()
    yd = np.zeros(100)
    sh[0].y_int, sh[0].y = y.ctypes.data, yd.ctypes.data          # counts as doubles too: refused, not half read
    assert lib.stk_model_create(ctx._h, 4, sh, 1, ctypes.byref(h)) == -1
    assert "y and sigma must be NULL" in lib.stk_last_error().decode()


def test_poisson_model_data_round_trip(ctx):
    """copy_data, the shard arrays and the device fingerprint (family word 4, y_int under tag 3)."""
    from stark_amd import engine
    _rng, X, y, _beta = make_data(300, 7)
    m = engine.Model(ctx, "poisson", [{"x": X, "y": y}])
    try:
        back = m.copy_data(0)
        assert back["y"].dtype == np.int32 and np.array_equal(back["y"], y) and np.array_equal(back["x"], X)
        arr = m.device_arrays(0)
        assert set(arr) == {"x", "y"} and arr["x"][1] == 300 * 7 and arr["y"][1] == 300
        fp = int(m.fingerprint(0))
        assert fp == int(engine.shard_fingerprint("poisson", {"x": X, "y": y}))
        assert fp != int(engine.shard_fingerprint("poisson", {"x": X, "y": np.where(np.arange(300) == 5, y + 1, y)}))
    finally:
        m.close()


# ---------------------------------------------------------------- 5. batches and grouped launches
def test_poisson_chain_batches_and_shards_bitwise(ctx):
    from stark_amd import engine
    shards = []
    for s in range(3):
        _rng, X, y, _beta = make_data(1000, 100, seed=50 + s)
        shards.append({"x": X, "y": y})
    rng = np.random.default_rng(5)
    m = engine.Model(ctx, "poisson", shards)
    try:
        for C in (17, 70):
            q = rng.normal(0, 0.2, (3, C, 101))
            lp, g = m.log_density_grad_chains(q)
            c0 = 0
            for b in engine.chain_batches(C, 100):
                blp, bg = m.log_density_grad_shards(np.ascontiguousarray(q[:, c0:c0 + b]))
                assert np.array_equal(lp[:, c0:c0 + b], blp) and np.array_equal(g[:, c0:c0 + b], bg), (C, c0, b)
                c0 += b
            assert c0 == C
        q = rng.normal(0, 0.2, (3, 16, 101))
        lp, g = m.log_density_grad_shards(q)
        for s in range(3):
            slp, sg = m.log_density_grad(s, q[s])
            assert np.array_equal(lp[s], slp) and np.array_equal(g[s], sg), s
            check_bars(slp, sg, *ref_lpgrad(shards[s]["x"], shards[s]["y"], q[s]), where=("shard", s))
    finally:
        m.close()


# ---------------------------------------------------------------- 6. sampling against an exact posterior
@pytest.fixture(scope="module")
def grid_posterior():
    """n = 300, d = 1, y ~ Poisson(exp(0.4 + 0.7 x)), flat priors: the posterior of (alpha, beta) on a
    401 x 401 tensor grid over +-0.6 around (0.4, 0.7) (grids of 201 and 401 agree to 1e-15 and the
    edge mass is 1e-25)."""
    rng = np.random.default_rng(2024)
    x = rng.uniform(-1.7, 1.7, 300)
    y = rng.poisson(np.exp(0.4 + 0.7 * x)).astype(np.int32)
    L = np.longdouble
    a = (0.4 + np.linspace(-0.6, 0.6, 401)).astype(L)
    b = (0.7 + np.linspace(-0.6, 0.6, 401)).astype(L)
    sb = np.exp(b[:, None] * x.astype(L)[None, :]).sum(1)                         # sum_i exp(b x_i)
    lp = a[:, None] * L(y.sum()) + b[None, :] * L((x * y).sum()) - np.exp(a)[:, None] * sb[None, :]
    w = np.exp(lp - lp.max())
    w /= w.sum()
    edge = w[0].sum() + w[-1].sum() + w[:, 0].sum() + w[:, -1].sum()
    assert edge < 1e-20
    wa, wb = w.sum(1), w.sum(0)
    ma, mb = (wa * a).sum(), (wb * b).sum()
    va, vb = (wa * (a - ma) ** 2).sum(), (wb * (b - mb) ** 2).sum()
    return x, y, np.array([ma, mb], np.float64), np.array([va, vb], np.float64)


@pytest.mark.parametrize("metric", ["diag_e", "dense_e"])
@pytest.mark.parametrize("chains", [16, 3])
def test_poisson_sampling_exact(ctx, grid_posterior, chains, metric):
    """Four-sigma bars from the run's own effective sizes: |mean - exact| <= 4 sd / sqrt(n_eff) and
    |var / exact - 1| <= 4 sqrt(2 / n_eff2), n_eff2 the n_eff of the centred squares; no divergences;
    and the lp__ row is the reference density at the drawn point (the machine samples what test 1
    checked)."""
    from stark_amd import diagnostics, engine
    x, y, mean, var = grid_posterior
    X = x[:, None].copy()
    m = engine.Model(ctx, "poisson", [{"x": X, "y": y}])
    try:
        res = m.sample(num_warmup=300, num_samples=1000, chains=chains, seed=4100 + chains, metric=metric)
    finally:
        m.close()
    assert res.info["divergent"] == 0 and res.info["errors"] == 0, res.info
    dr = res.draws[0]
    assert dr.shape == (3, chains * 1000) and np.isfinite(dr).all()
    for p in range(2):
        ch = dr[p].reshape(chains, 1000)
        ne = diagnostics.ess(ch)
        sq = (ch - mean[p]) ** 2
        ne2 = diagnostics.ess(sq)
        em = abs(ch.mean() - mean[p]) / (np.sqrt(var[p]) / np.sqrt(ne))
        ev = abs(sq.mean() / var[p] - 1.0) / np.sqrt(2.0 / ne2)
        print(f"chains={chains} {metric} par {p}: n_eff {ne:.0f} mean z {em:.2f}; n_eff2 {ne2:.0f} var z {ev:.2f}")
        assert em <= 4.0, (p, ch.mean(), mean[p], ne)
        assert ev <= 4.0, (p, sq.mean(), var[p], ne2)
    olp, _og = ref_lpgrad(X, y, np.ascontiguousarray(dr[:2].T))
    olp = olp.astype(np.float64)
    assert np.all(np.abs(dr[2] - olp) <= RTOL * np.maximum(np.abs(olp), 1.0))


# ---------------------------------------------------------------- 7. determinism and checkpoint
@pytest.fixture(scope="module")
def small_counts():
    """2000 rows, d = 20, counts in {0, 1} only (valid Poisson data whose bits a logistic shard may hold)."""
    rng = np.random.default_rng(77)
    X = rng.uniform(-1.7, 1.7, (2000, 20))
    y = np.minimum(rng.poisson(np.exp(-1.0 + X @ rng.normal(0, 0.2, 20))), 1).astype(np.int32)
    return X, y


def test_poisson_deterministic_and_resumable(ctx, small_counts):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    X, y = small_counts
    cfg = dict(num_warmup=60, num_samples=60, chains=5, seed=31)
    m = engine.Model(ctx, "poisson", [{"x": X, "y": y}])
    lg = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
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
        # the family is part of the state's geometry: a logistic sampler of the same n, d and y bits refuses
        s3 = lg.sampler(**cfg)
        before = s3.iterations().copy()
        with pytest.raises(StarkHipError) as e:
            s3.load_state(blob)
        assert e.value.code == -1
        assert np.array_equal(s3.iterations(), before)
        s3.run(40)
        lblob = s3.save_state()
        s3.close()
        s4 = m.sampler(**cfg)                       # and the reverse
        with pytest.raises(StarkHipError) as e:
            s4.load_state(lblob)
        assert e.value.code == -1
        s4.close()
    finally:
        m.close()
        lg.close()


@pytest.mark.parametrize("metric,criterion", [("unit_e", "stan2.23"), ("dense_e", "stan2.23"), ("diag_e", "stan2.19")])
def test_poisson_metrics_and_criteria_run(ctx, small_counts, metric, criterion):
    """Every metric and both U-turn criteria run the family; the fixed-step transition hooks too."""
    from stark_amd import engine
    X, y = small_counts
    m = engine.Model(ctx, "poisson", [{"x": X[:500], "y": y[:500]}])
    try:
        res = m.sample(num_warmup=100, num_samples=50, chains=2, seed=8, metric=metric, nuts_criterion=criterion)
        assert res.info["errors"] == 0 and np.isfinite(res.draws[0]).all()
        q0 = np.zeros((2, 21))
        im = np.eye(21) * 0.01 if metric == "dense_e" else (None if metric == "unit_e" else np.full(21, 0.01))
        qn, lpn, _st = m.transition(0, q0, seed=3, iteration=0, eps=0.05, inv_metric=im)
        olp, _og = ref_lpgrad(X[:500], y[:500], qn)
        assert np.all(np.abs(lpn - olp.astype(np.float64)) <= RTOL * np.maximum(np.abs(olp.astype(np.float64)), 1.0))
        assert not np.array_equal(qn, q0)
    finally:
        m.close()


# ---------------------------------------------------------------- 8. the driver
PROGRAM = """
data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; int<lower=0> y[N]; }
parameters { real alpha; vector[K] beta; }
model {
  alpha ~ normal(0, 2.5);
  beta ~ normal(0, 1);
  y ~ poisson_log(alpha + x * beta);
}
"""


def test_poisson_through_the_driver(ctx):
    from stark_amd import engine, stark
    from stark_amd.rdd import LocalContext
    rng = np.random.default_rng(12)
    X = rng.uniform(-1.7, 1.7, (1000, 3))
    y = rng.poisson(np.exp(0.5 + X @ np.array([0.4, -0.3, 0.2])))
    rows = [tuple(X[i]) + (int(y[i]),) for i in range(1000)]

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": 3, "x": a[:, :3], "y": a[:, 3].astype(np.int64)}

    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize(rows, 4), prep)
    st.setStanModel(model_code=PROGRAM)
    assert st.family == "poisson" and st.priors == {"alpha": 2.5, "beta": 1.0}
    out = st.concensusWeight(chains=4, iter=600, separate_lp=True, permuted=False, seed=21)
    assert out.shape == (5, 4 * 300)
    assert len(st.last_run.draws) == 4 and st.last_run.info["errors"] == 0
    ref, used = engine.consensus(st.last_run.draws, separate_lp=True)
    assert used.all() and np.array_equal(out, ref)
    assert np.all(np.abs(out[:4].mean(1) - np.array([0.5, 0.4, -0.3, 0.2])) < 0.15)    # the data's coefficients, loosely
    two = st.distribute(n=2, chains=2, iter=200, seed=22)
    assert two.shape == (2 * 5, 2 * 100)


# ---------------------------------------------------------------- 9. the two refusals
def test_poisson_refusals(ctx, small_counts):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    with pytest.raises(StarkHipError) as e:
        engine.Model.synthetic(ctx, "poisson", 1, 1000, 10)
    assert e.value.code == -1 and "poisson" in str(e.value)
    X, y = small_counts
    m = engine.Model(ctx, "poisson", [{"x": X[:100], "y": y[:100]}])
    try:
        s = m.sampler(num_warmup=10, num_samples=10, chains=2, seed=1)
        with pytest.raises(StarkHipError) as e:
            s.set_allreduce(lambda ptr, count, stream: None)
        assert e.value.code == -1 and "poisson" in str(e.value)
        s.close()
    finally:
        m.close()
