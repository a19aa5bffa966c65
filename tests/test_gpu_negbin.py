"""The negative-binomial (neg_binomial_2_log) family on the GPU: every sweep's lp / gradient against the
longdouble reference tests/negbin_ref.py (the density of include/stark_hip.h, STK_NEGBIN), extreme eta and
extreme v, priors, the y >= 0 check, the data round trip, chain batches and grouped launches, sampling against
an exact grid posterior, determinism and checkpoints, the metrics and U-turn criteria, the Stark driver and
the family's refusals.

Bars: tests/test_gpu_poisson.py::check_bars.
"""
import ctypes

import numpy as np
import pytest

import negbin_ref as R
from test_gpu_poisson import RTOL, check_bars

pytestmark = pytest.mark.gpu

FAM = "neg_binomial"


def make_data(n, d, seed=None, big=True):
    """X ~ U(-1.7, 1.7), beta ~ N(0, 1/sqrt(d)), eta = 0.3 + X beta with the first max(1, n/50) rows' eta times
    6, clipped to +-20; y ~ NegBin(mean exp(eta), phi = 1.5) (a gamma-Poisson mixture: overdispersed), clipped
    to int32, row 0 set to 0; big: one count of 2^31 - 1 where n >= 64."""
    rng = np.random.default_rng(n * 1000 + d if seed is None else seed)
    X = rng.uniform(-1.7, 1.7, (n, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    eta = 0.3 + X @ beta
    eta[: max(1, n // 50)] *= 6.0
    eta = np.clip(eta, -20.0, 20.0)
    lam = np.exp(eta) * rng.gamma(1.5, 1 / 1.5, n)
    y = np.minimum(rng.poisson(np.minimum(lam, 2.0 ** 31)), 2 ** 31 - 1).astype(np.int64)
    y[0] = 0
    if big and n >= 64:
        y[n // 2] = 2 ** 31 - 1
    assert y.min() == 0 and y.max() <= 2 ** 31 - 1
    return rng, X, y.astype(np.int32), beta


def points(rng, beta, C, d):
    """C points (alpha, beta, v): v spread log-uniformly over phi in [1e-3, 1e6] across the chains."""
    q = rng.normal(0, 0.2, (C, d + 2))
    q[0, : d + 1] = np.concatenate([[0.3], 3 * beta])
    if C > 1:
        q[1, 1: d + 1] = 12 * beta                    # |eta| up to ~45
    q[:, -1] = np.log(1.5) if C == 1 else np.log(1e-3) + np.log(1e9) * np.arange(C) / (C - 1)
    return q


VALU = [(1, 1, 1), (7, 3, 5), (65, 104, 3), (3000, 120, 5), (333, 129, 5), (257, 300, 8)]
S16 = [(1, 1, 16), (7, 3, 16), (300, 113, 16), (333, 128, 16), (4097, 50, 16), (65, 104, 20)]
S16W = [(333, 129, 16), (257, 512, 16), (130, 1023, 16), (200, 1024, 16)]
G64 = [(1, 1, 64), (300, 17, 64), (333, 129, 64), (200, 1024, 64), (130, 1001, 70)]


# ---------------------------------------------------------------- 1. every sweep against the reference
@pytest.mark.parametrize("big", [True, False], ids=["int32max", "twin"])
@pytest.mark.parametrize("n,d,C", VALU + S16 + S16W + G64)
def test_negbin_lpgrad(ctx, n, d, C, big):
    """VALU sweeps (k_sweep3, k_sweep2, k_sweep at odd and wide d), k_sweep16 (masked last sub-tile, the VALU
    last tile, beta in registers or not, several chunks, 16 + 4), k_sweep16w and the 64-chain passes (64 + 4 +
    2), each with the third partial column and the count table's terms in the reduce.  Two shards, the first a
    third of the rows; the second is evaluated.  twin: the same rows without the count of 2^31 - 1, so that the
    bars are not set by one row."""
    from stark_amd import engine
    rng, X, y, beta = make_data(n, d, big=big)
    k = max(1, n // 3)
    m = engine.Model(ctx, FAM, [{"x": X[:k], "y": y[:k]}, {"x": X, "y": y}])
    try:
        assert m.D == [d + 2, d + 2] and m.P == [d + 3, d + 3] and m.n_rows == [k, n]
        q = points(rng, beta, C, d)
        lp, g = m.log_density_grad(1, q)
    finally:
        m.close()
    olp, og = R.ref_lpgrad(X, y, q)
    assert np.all(np.isfinite(olp.astype(np.float64)))
    check_bars(lp, g, olp, og, (n, d, C, big))


# ---------------------------------------------------------------- 2. extreme eta, extreme v
def either_or(lp, g, olp, og, where):
    """A point whose reference is finite meets the bars or is non-finite, never +inf; one whose reference is
    not finite is non-finite."""
    with np.errstate(over="ignore", invalid="ignore"):
        fin = np.isfinite(olp.astype(np.float64)) & np.all(np.isfinite(og.astype(np.float64)), axis=1)
    assert not np.any(lp == np.inf), (where, lp)
    assert not np.any(np.isfinite(lp[~fin])), (where, lp[~fin])
    idx = np.flatnonzero(fin & np.isfinite(lp))
    check_bars(lp[idx], g[idx], olp[idx], og[idx], where)
    return fin, idx


SHAPES_X = [(300, 113, 16), (500, 100, 64), (400, 60, 4), (300, 200, 16), (257, 131, 3)]


@pytest.mark.parametrize("scale", [30.0, 1e3, 1e150])
@pytest.mark.parametrize("n,d,C", SHAPES_X)
def test_negbin_lpgrad_extreme_eta(ctx, scale, n, d, C):
    """Half of the points' (alpha, beta) scaled by 30, 1e3, 1e150.  sp(t) grows like t, not like e^t, so the
    reference stays finite; at scale 30 the GPU must be too and meet the bars at every point."""
    from stark_amd import engine
    rng, X, y, beta = make_data(n, d, seed=int(scale) % 1000 + n)
    q = points(rng, beta, C, d)
    q[:, : d + 1] = rng.normal(0, 1.0 / np.sqrt(d), (C, d + 1))
    q[: C // 2, : d + 1] *= scale
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    try:
        lp, g = m.log_density_grad(0, q)
    finally:
        m.close()
    olp, og = R.ref_lpgrad(X, y, q)
    fin, idx = either_or(lp, g, olp, og, (scale, n, d, C))
    assert fin[C // 2:].all() and set(range(C // 2, C)) <= set(idx.tolist())
    if scale == 30.0:
        assert fin.all() and len(idx) == C


@pytest.mark.parametrize("n,d,C", SHAPES_X)
def test_negbin_lpgrad_extreme_v(ctx, n, d, C):
    """v = +-40 and +-700 (phi from 1e-304 to 1e304: inside the doubles, the reference is finite), and +-800,
    where e^v is 0 or inf in fp64: lp must be NaN or -inf there."""
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
    fin, _idx = either_or(lp, g, olp, og, ("v", n, d, C))
    assert np.array_equal(fin, np.abs(q[:, -1]) < 750)
    assert not np.any(np.isfinite(g[~fin, -1]))


# ---------------------------------------------------------------- 3. priors
@pytest.mark.parametrize("n,d,C", [(300, 113, 16), (257, 100, 2), (300, 17, 64)])
def test_negbin_priors(ctx, n, d, C):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    rng, X, y, beta = make_data(n, d, big=False)
    q = points(rng, beta, C, d)
    q[:, -1] = rng.uniform(-2, 3, C)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    try:
        lp0, g0 = m.log_density_grad(0, q)
        m.set_prior(alpha=2.0, beta=0.5, phi=(2.0, 0.5))
        lp1, g1 = m.log_density_grad(0, q)
        m.set_prior(phi=(1.0, 0.25))                               # exponential(0.25); alpha, beta flat again
        lp2, g2 = m.log_density_grad(0, q)
        for bad in ((0.0, 1.0), (-1.0, 1.0), (2.0, -0.5), (np.inf, 1.0)):
            with pytest.raises(StarkHipError) as e:
                m.set_prior(phi=bad)
            assert e.value.code == -1
    finally:
        m.close()
    check_bars(lp0, g0, *R.ref_lpgrad(X, y, q), where="flat")
    check_bars(lp1, g1, *R.ref_lpgrad(X, y, q, prior=(2.0, 0.5), phi_prior=(2.0, 0.5)), where="all three")
    check_bars(lp2, g2, *R.ref_lpgrad(X, y, q, phi_prior=(1.0, 0.25)), where="exponential")
    assert np.all(lp2 < lp0)


def test_negbin_phi_prior_is_the_familys(ctx):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    m = engine.Model(ctx, "poisson", [{"x": np.zeros((4, 1)), "y": np.arange(4)}])
    try:
        with pytest.raises(StarkHipError) as e:
            m.set_prior(phi=(2.0, 0.5))
        assert e.value.code == -1 and "poisson" in str(e.value)
    finally:
        m.close()


# ---------------------------------------------------------------- 4. bad data, the round trip
def test_negbin_negative_count_refused(ctx):
    from stark_amd import _lib
    lib = _lib.load()
    x = np.zeros((100, 2))
    y = np.arange(100, dtype=np.int32)
    y[17] = -3
    y[60] = -1
    sh = (_lib.Shard * 1)(_lib.Shard(100, 2, x.ctypes.data, None, y.ctypes.data, None))
    h = ctypes.c_void_p()
    assert lib.stk_model_create(ctx._h, 5, sh, 1, ctypes.byref(h)) == -1          # STK_E_ARG
    msg = lib.stk_last_error().decode()
    assert "y_int[17] = -3" in msg and "neg_binomial_2_log needs y >= 0" in msg, msg
    y[17], y[60] = 17, 60
    assert lib.stk_model_create(ctx._h, 5, sh, 1, ctypes.byref(h)) == 0
    lib.stk_model_destroy(h)
    sh[0].y_int = None
    assert lib.stk_model_create(ctx._h, 5, sh, 1, ctypes.byref(h)) == -1
    assert "neg_binomial needs y_int" in lib.stk_last_error().decode()
    yd = np.zeros(100)
    sh[0].y_int, sh[0].y = y.ctypes.data, yd.ctypes.data          # counts as doubles too: refused, not half read
    assert lib.stk_model_create(ctx._h, 5, sh, 1, ctypes.byref(h)) == -1
    assert "y and sigma must be NULL" in lib.stk_last_error().decode()


def test_negbin_model_data_round_trip(ctx):
    """copy_data, the shard arrays (the count table is not among them) and the device fingerprint (family word 5,
    y_int under tag 3: the table is derived data and no part of it)."""
    from stark_amd import engine
    _rng, X, y, _beta = make_data(300, 7)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    try:
        back = m.copy_data(0)
        assert back["y"].dtype == np.int32 and np.array_equal(back["y"], y) and np.array_equal(back["x"], X)
        arr = m.device_arrays(0)
        assert set(arr) == {"x", "y"} and arr["x"][1] == 300 * 7 and arr["y"][1] == 300
        fp = int(m.fingerprint(0))
        assert fp == int(engine.shard_fingerprint(FAM, {"x": X, "y": y}))
        assert fp != int(engine.shard_fingerprint("poisson", {"x": X, "y": y}))
        assert fp != int(engine.shard_fingerprint(FAM, {"x": X, "y": np.where(np.arange(300) == 5, y + 1, y)}))
    finally:
        m.close()


# ---------------------------------------------------------------- 5. batches and grouped launches
def test_negbin_chain_batches_and_shards_bitwise(ctx):
    from stark_amd import engine
    shards = []
    for s in range(3):
        _rng, X, y, _beta = make_data(600, 100, seed=50 + s, big=False)
        shards.append({"x": X, "y": y})
    rng = np.random.default_rng(5)
    m = engine.Model(ctx, FAM, shards)
    try:
        for C in (17, 70):
            q = rng.normal(0, 0.2, (3, C, 102))
            q[:, :, -1] = rng.uniform(-3, 6, (3, C))
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
            check_bars(slp, sg, *R.ref_lpgrad(shards[s]["x"], shards[s]["y"], q[s]), where=("shard", s))
    finally:
        m.close()


# ---------------------------------------------------------------- 6. sampling against an exact posterior
PHI_PRIOR = (2.0, 0.5)


@pytest.fixture(scope="module")
def grid_posterior():
    """n = 300, d = 1, y ~ NegBin(mean exp(0.4 + 0.7 x), phi = 1.5), phi ~ gamma(2, 0.5), flat alpha and beta: the
    posterior of (alpha, beta, v) on an 81 x 81 x 161 tensor grid over alpha 0.4 +- 0.8, beta 0.7 +- 0.7,
    v in log 1.5 + [-1.6, 2.4]; its every-other-point 41 x 41 x 81 subgrid must agree to 1e-6 relative on all six
    moments and the mass on the grid's faces must be below 1e-12."""
    rng = np.random.default_rng(2025)
    x = rng.uniform(-1.7, 1.7, 300)
    y = rng.negative_binomial(1.5, 1.5 / (1.5 + np.exp(0.4 + 0.7 * x))).astype(np.int32)
    assert y.max() == 18
    a = 0.4 + np.linspace(-0.8, 0.8, 81)
    b = 0.7 + np.linspace(-0.7, 0.7, 81)
    v = np.log(1.5) + np.linspace(-1.6, 2.4, 161)
    eta = a[:, None, None] + b[None, :, None] * x[None, None, :]            # (81, 81, 300)
    E = np.exp(eta)
    lin = eta @ y.astype(np.float64)                                         # sum_i y_i eta_i
    lp = np.empty((81, 81, 161))
    for k, vk in enumerate(v):
        phi = np.exp(vk)
        a1, _s2 = R.phi_terms(y, phi)
        sp = np.log1p(E / phi)                                               # sp(eta - v)
        lp[:, :, k] = float(a1) + lin - sp @ (y + phi) + (PHI_PRIOR[0] - 1) * vk - PHI_PRIOR[1] * phi + vk

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

    fine, face = moments(lp, (a, b, v))
    coarse, _ = moments(lp[::2, ::2, ::2], (a[::2], b[::2], v[::2]))
    assert face < 1e-12, face
    assert np.all(np.abs(coarse - fine) <= 1e-6 * np.abs(fine)), (coarse, fine)
    return x, y, fine[:, 0].copy(), fine[:, 1].copy()


@pytest.mark.parametrize("metric", ["diag_e", "dense_e"])
@pytest.mark.parametrize("chains", [16, 3])
def test_negbin_sampling_exact(ctx, grid_posterior, chains, metric):
    """test_poisson_sampling_exact's criterion for alpha, beta and v = log phi: four-sigma bars from the run's own
    effective sizes, |mean - exact| <= 4 sd / sqrt(n_eff) and |var / exact - 1| <= 4 sqrt(2 / n_eff2), n_eff2 the
    n_eff of the centred squares; no divergences; the lp__ row is the reference density at the drawn point."""
    from stark_amd import diagnostics, engine
    x, y, mean, var = grid_posterior
    X = x[:, None].copy()
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    try:
        m.set_prior(phi=PHI_PRIOR)
        res = m.sample(num_warmup=300, num_samples=1000, chains=chains, seed=4100 + chains, metric=metric)
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
    olp, _og = R.ref_lpgrad(X, y, np.ascontiguousarray(par.T), phi_prior=PHI_PRIOR)
    olp = olp.astype(np.float64)
    assert np.all(np.abs(dr[3] - olp) <= RTOL * np.maximum(np.abs(olp), 1.0))


# ---------------------------------------------------------------- 7. determinism and checkpoint
@pytest.fixture(scope="module")
def small_counts():
    """1000 rows, d = 20, overdispersed counts."""
    rng = np.random.default_rng(77)
    X = rng.uniform(-1.7, 1.7, (1000, 20))
    mu = np.exp(0.5 + X @ rng.normal(0, 0.2, 20))
    y = rng.negative_binomial(2.0, 2.0 / (2.0 + mu)).astype(np.int32)
    return X, y


def test_negbin_deterministic_and_resumable(ctx, small_counts):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    X, y = small_counts
    cfg = dict(num_warmup=60, num_samples=60, chains=5, seed=31)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}])
    po = engine.Model(ctx, "poisson", [{"x": X, "y": y}])
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
        # the family is part of the state's geometry: a Poisson sampler on the same bits refuses the blob
        s3 = po.sampler(**cfg)
        before = s3.iterations().copy()
        with pytest.raises(StarkHipError) as e:
            s3.load_state(blob)
        assert e.value.code == -1
        assert np.array_equal(s3.iterations(), before)
        s3.run(40)
        pblob = s3.save_state()
        s3.close()
        s4 = m.sampler(**cfg)                       # and the reverse
        with pytest.raises(StarkHipError) as e:
            s4.load_state(pblob)
        assert e.value.code == -1
        s4.close()
        m.set_prior(phi=(2.0, 0.5))                 # the phi prior is part of the geometry too
        s5 = m.sampler(**cfg)
        with pytest.raises(StarkHipError) as e:
            s5.load_state(blob)
        assert e.value.code == -1
        s5.close()
    finally:
        m.close()
        po.close()


@pytest.mark.parametrize("metric,criterion", [("unit_e", "stan2.19"), ("unit_e", "stan2.23"), ("dense_e", "stan2.19"),
                                              ("dense_e", "stan2.23"), ("diag_e", "stan2.19")])
def test_negbin_metrics_and_criteria_run(ctx, small_counts, metric, criterion):
    """unit_e and dense_e under both U-turn criteria; the fixed-step transition hook's lp is the reference's."""
    from stark_amd import engine
    X, y = small_counts
    m = engine.Model(ctx, FAM, [{"x": X[:500], "y": y[:500]}])
    try:
        res = m.sample(num_warmup=100, num_samples=50, chains=2, seed=8, metric=metric, nuts_criterion=criterion)
        assert res.info["errors"] == 0 and np.isfinite(res.draws[0]).all() and np.all(res.draws[0][21] > 0)
        q0 = np.zeros((2, 22))
        im = np.eye(22) * 0.01 if metric == "dense_e" else (None if metric == "unit_e" else np.full(22, 0.01))
        qn, lpn, _st = m.transition(0, q0, seed=3, iteration=0, eps=0.05, inv_metric=im)
        olp, _og = R.ref_lpgrad(X[:500], y[:500], qn)
        assert np.all(np.abs(lpn - olp.astype(np.float64)) <= RTOL * np.maximum(np.abs(olp.astype(np.float64)), 1.0))
        assert not np.array_equal(qn, q0)
    finally:
        m.close()


# ---------------------------------------------------------------- 8. the driver
PROGRAM = """
data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; int<lower=0> y[N]; }
parameters { real alpha; vector[K] beta; real<lower=0> phi; }
model {
  alpha ~ normal(0, 2.5);
  beta ~ normal(0, 1);
  phi ~ gamma(2, 0.5);
  y ~ neg_binomial_2_log(alpha + x * beta, phi);
}
"""


def test_negbin_through_the_driver(ctx):
    from stark_amd import engine, stark
    from stark_amd.rdd import LocalContext
    rng = np.random.default_rng(12)
    X = rng.uniform(-1.7, 1.7, (1000, 3))
    mu = np.exp(0.5 + X @ np.array([0.4, -0.3, 0.2]))
    y = rng.negative_binomial(2.0, 2.0 / (2.0 + mu))
    rows = [tuple(X[i]) + (int(y[i]),) for i in range(1000)]

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": 3, "x": a[:, :3], "y": a[:, 3].astype(np.int64)}

    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize(rows, 4), prep)
    st.setStanModel(model_code=PROGRAM)
    assert st.family == FAM and st.priors == {"alpha": 2.5, "beta": 1.0, "phi": (2.0, 0.5)}
    out = st.concensusWeight(chains=4, iter=600, separate_lp=True, permuted=False, seed=21)
    assert out.shape == (6, 4 * 300)
    assert len(st.last_run.draws) == 4 and st.last_run.info["errors"] == 0
    ref, used = engine.consensus(st.last_run.draws, separate_lp=True)
    assert used.all() and np.array_equal(out, ref)
    assert np.all(np.abs(out[:4].mean(1) - np.array([0.5, 0.4, -0.3, 0.2])) < 0.2)    # the data's coefficients, loosely
    assert 1.0 < out[4].mean() < 4.0                                                  # and phi = 2
    two = st.distribute(n=2, chains=2, iter=200, seed=22)
    assert two.shape == (2 * 6, 2 * 100)


# ---------------------------------------------------------------- 9. the refusals
def test_negbin_refusals(ctx, small_counts):
    """stk_model_create_synthetic, stk_sampler_set_allreduce and the six analysis sweeps refuse the family by
    name with STK_E_ARG (the driver's own refusals: tests/test_host_negbin.py)."""
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    with pytest.raises(StarkHipError) as e:
        engine.Model.synthetic(ctx, FAM, 1, 1000, 10)
    assert e.value.code == -1 and FAM in str(e.value)
    X, y = small_counts
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
    finally:
        m.close()
