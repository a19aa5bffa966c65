"""Host side of the semiparametric density-product combiner: the chains' host twin (stk_dpe_sample_host, compiled
from csrc/dpe_math.h, the header the kernel uses) against tests/dpe_ref.py's longdouble restatement, the limits of
the estimator, and its stationary distribution on a skewed case.  No GPU.

Shapes with S <= p cannot come from draws (the sample covariance is singular, and the prepare refuses them), so
their prepared arrays are dpe_ref.synthetic_prep's; the others are dpe_ref.prepare's of random draws."""
import numpy as np
import pytest

import dpe_ref as dr

LD = np.longdouble


def shard_draws(rng, M, S, p, lp_row=True):
    X = rng.standard_normal((M, p + (1 if lp_row else 0), S))
    X[:, :p] = X[:, :p] * rng.uniform(0.5, 2.0, (M, p, 1)) + rng.standard_normal((M, p, 1))
    if lp_row:
        X[:, p] -= 40.0
    return X


def ref_prep(rng, M, S, p):
    if S > p + 1:
        return dr.as_float64(dr.prepare(shard_draws(rng, M, S, p), lp_row=True))
    return dr.synthetic_prep(rng, M, S, p, lp_row=True)


def test_launch_info_is_a_function_of_its_arguments():
    from stark_amd import engine
    a = engine.dpe_launch(8, 103, 16000, 16000, 1024)
    assert a == engine.dpe_launch(8, 103, 16000, 16000, 1024)
    assert (a["p"], a["ldp"], a["coords_per_lane"], a["draws_per_chain"], a["blocks"]) == (102, 104, 2, 16, 1024)
    assert a["lds_bytes"] == 8 * 8 and a["prepare_ws_bytes"] == 8 * 16000 * 104 * 8
    assert engine.dpe_launch(8, 102, 16000, 16000, 1024, lp_row=False)["p"] == 102
    for p, nc in ((1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (257, 8), (513, 16), (1024, 16)):
        assert engine.dpe_launch(2, p, 10, 5, 2, lp_row=False)["coords_per_lane"] == nc
    assert engine.dpe_launch(2, 3, 10, 7, 3)["draws_per_chain"] == 3


def test_every_refusal_names_its_value():
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    prep = dr.synthetic_prep(np.random.default_rng(0), 2, 6, 3)
    for kw, word in ((dict(T=0), "T = 0"), (dict(chains=0), "K = 0"), (dict(thin=0), "thin = 0"),
                     (dict(burn=-1), "burn = -1"), (dict(bandwidth=0.0), "h[0] = 0"), (dict(bandwidth=-0.5), "h[0] = -0.5"),
                     (dict(bandwidth=float("inf")), "h[0] = inf"), (dict(bandwidth=float("nan")), "h[0] = nan"),
                     (dict(stream=2 ** 24), "stream = 16777216")):
        args = dict(T=4, chains=2, burn=0, thin=1)
        args.update(kw)
        with pytest.raises(StarkHipError, match="STK_E_ARG") as e:
            engine.dpe_sample_host(prep, **args)
        assert word in str(e.value), (kw, str(e.value))
    with pytest.raises(StarkHipError, match="p = 1025"):
        engine.dpe_launch(2, 1025, 2000, 5, 2, lp_row=False)
    with pytest.raises(StarkHipError, match="p = 1025"):
        engine.dpe_sample_host(dict(prep, p=1025), T=4, chains=2, burn=0, thin=1)
    with pytest.raises(StarkHipError, match="T = 0"):
        engine.dpe_launch(2, 3, 10, 0, 2)
    with pytest.raises(StarkHipError, match="K = -1"):
        engine.dpe_launch(2, 3, 10, 5, -1)
    with pytest.raises(ValueError, match="sweeps"):
        engine.dpe_sample_host(prep, T=4, chains=2, burn=0, thin=1, bandwidth=np.ones(5))


@pytest.mark.parametrize("K,T", ((1, 5), (3, 7)))
@pytest.mark.parametrize("bandwidth", (0.3, 1.0, None))
@pytest.mark.parametrize("M,S,p", ((1, 5, 1), (2, 6, 3), (3, 17, 65)))
def test_twin_agrees_with_the_longdouble_replay(M, S, p, bandwidth, K, T):
    """burn = 0, thin = 2, T not a multiple of K (K = 3).  Every log W of the trace within 1e-10 of max |log W|, every
    accept decision that of the recomputed margin, every draw within 1e-12 of the draws' scale.  No proposal's
    |margin| may be below 1e-9 (a condition on the inputs: change the seed if one is)."""
    from stark_amd import engine
    seed, stream, thin = 1234 + 17 * M + p, 5, 2
    prep = ref_prep(np.random.default_rng(seed), M, S, p)
    out, info = engine.dpe_sample_host(prep, T=T, chains=K, burn=0, thin=thin, bandwidth=bandwidth, seed=seed,
                                       stream=stream, trace=True)
    sweeps = info["sweeps"]
    assert sweeps == thin * (-(-T // K))
    h = engine.dpe_bandwidths(bandwidth, sweeps, p)
    if bandwidth is None:
        assert np.array_equal(h, np.arange(1, sweeps + 1, dtype=np.float64) ** (-1.0 / (4 + p)))
    rp = dr.replay(prep, h, seed, stream, T, K, 0, thin, info["trace_idx"])
    assert rp["min_margin"] >= 1e-9, rp["min_margin"]
    assert rp["wrong"] == 0
    scale = float(np.abs(rp["logw"]).max())
    err_w = float(np.abs(info["trace_logw"] - rp["logw"]).max()) / scale
    oscale = float(np.abs(rp["out"]).max())
    err_o = float(np.abs(out - rp["out"]).max()) / oscale
    print(f"MAXERR host twin M={M} S={S} p={p} h={bandwidth} K={K}: logw {err_w:.3e} theta {err_o:.3e}")
    assert np.isfinite(out).all() and out.shape == (p + 1, T)
    assert err_w <= 1e-10
    assert err_o <= 1e-12
    moved = (np.diff(np.concatenate([dr.init_indices(seed, stream, K, M, S)[:, None, :], info["trace_idx"]], axis=1),
                     axis=1) != 0).reshape(-1, M).sum(axis=0)
    assert np.all(info["accept"] >= moved)       # a proposal of the current index may count, and moves nothing


def test_chains_do_not_depend_on_the_chain_count():
    from stark_amd import engine
    prep = dr.synthetic_prep(np.random.default_rng(3), 3, 17, 5)
    a = engine.dpe_sample_host(prep, T=12, chains=3, burn=2, thin=1, bandwidth=0.5, seed=9, trace=True)[1]
    b = engine.dpe_sample_host(prep, T=24, chains=6, burn=2, thin=1, bandwidth=0.5, seed=9, trace=True)[1]
    assert a["sweeps"] == b["sweeps"] == 6
    assert np.array_equal(a["trace_idx"], b["trace_idx"][:3])
    assert np.array_equal(a["trace_logw"], b["trace_logw"][:3])
    c = engine.dpe_sample_host(prep, T=12, chains=3, burn=2, thin=1, bandwidth=0.5, seed=10, trace=True)[1]
    assert not np.array_equal(a["trace_idx"], c["trace_idx"])


def chain_stats(x, K):
    """Per-chain means of the rows of x [rows, T] (chain k owns columns k, k + K, ..) and their MCSE."""
    J = x.shape[1] // K
    per = x[:, :J * K].reshape(x.shape[0], J, K).mean(axis=1)
    return per.mean(axis=1), per.std(axis=1, ddof=1) / np.sqrt(K)


def test_huge_bandwidth_is_the_parametric_product():
    """h = 1e6: every component is N(0, I / M) in y, so theta ~ N(mu_M, Sigma_M) whatever the indices do."""
    from stark_amd import engine
    rng = np.random.default_rng(11)
    prep = dr.as_float64(dr.prepare(shard_draws(rng, 3, 50, 2, lp_row=False), lp_row=False))
    K = 32
    out, _ = engine.dpe_sample_host(prep, T=K * 60, chains=K, burn=0, thin=1, bandwidth=1e6, seed=4)
    mean, mcse = chain_stats(out, K)
    assert np.all(np.abs(mean - prep["mu"]) <= 5 * mcse), (mean, prep["mu"], mcse)
    d = out - prep["mu"][:, None]
    second = np.stack([d[0] * d[0], d[0] * d[1], d[1] * d[1]])
    m2, mcse2 = chain_stats(second, K)
    Sig = prep["L"] @ prep["L"].T
    assert np.all(np.abs(m2 - np.array([Sig[0, 0], Sig[0, 1], Sig[1, 1]])) <= 5 * mcse2), (m2, Sig, mcse2)


def test_one_shard_tiny_bandwidth_returns_its_draws():
    from stark_amd import engine
    rng = np.random.default_rng(12)
    X = shard_draws(rng, 1, 40, 3, lp_row=False)
    prep = dr.as_float64(dr.prepare(X, lp_row=False))
    out, _ = engine.dpe_sample_host(prep, T=64, chains=8, burn=3, thin=1, bandwidth=1e-8, seed=2)
    sd = X[0].std(axis=1, ddof=1)
    dist = np.abs(out[:, :, None] - X[0][:, None, :]) / sd[:, None, None]       # [p, T, S]
    assert dist.max(axis=0).min(axis=1).max() <= 1e-6


def test_sampler_matches_the_enumerated_mixture():
    """(M, S, p) = (2, 6, 3): the 36 components are enumerated; the chains' mean is within 5 between-chain MCSEs."""
    from stark_amd import engine
    rng = np.random.default_rng(21)
    prep = dr.as_float64(dr.prepare(shard_draws(rng, 2, 6, 3, lp_row=False), lp_row=False))
    K = 32
    out, info = engine.dpe_sample_host(prep, T=K * 150, chains=K, burn=20, thin=2, bandwidth=0.5, seed=6)
    mean, mcse = chain_stats(out, K)
    ref_mean, ref_cov = dr.mixture_moments(prep, 0.5)
    assert np.all(np.abs(mean - np.asarray(ref_mean, np.float64)) <= 5 * mcse), (mean, ref_mean, mcse)
    d = out - np.asarray(ref_mean, np.float64)[:, None]
    var, mcse_v = chain_stats(d * d, K)
    assert np.all(np.abs(var - np.diag(np.asarray(ref_cov, np.float64))) <= 5 * mcse_v), (var, np.diag(ref_cov), mcse_v)
    assert np.all(info["accept_rate"] > 0) and np.all(info["accept_rate"] < 1)


def test_stationary_distribution_on_gamma_shards():
    """Four Gamma(3, 1) subposteriors of 4,000 draws (product Gamma(9, 4): mean 2.25), h = 0.3, K = 32, burn 200,
    thin 5, T = 2,000.  Mean and sd of the output within 5 MCSEs (sd of the 32 chain values / sqrt(32)) of the
    estimator's own moments by quadrature; a numpy prototype of the algorithm gave 2.368 against 2.366.  The
    mean is nearer 2.25 than the weighted average of the same draws is (2.98 in the prototype)."""
    from stark_amd import engine
    rng = np.random.default_rng(2024)
    X = rng.gamma(3.0, 1.0, (4, 1, 4000))
    prep = dr.as_float64(dr.prepare(X, lp_row=False))
    K, T = 32, 2000
    out, info = engine.dpe_sample_host(prep, T=T, chains=K, burn=200, thin=5, bandwidth=0.3, seed=1)
    q_mean, q_sd = dr.quadrature_1d(X[:, 0, :], 0.3, grid=np.linspace(-2.0, 9.0, 1101))
    J = T // K
    per = out[0, :J * K].reshape(J, K)
    means, sds = per.mean(axis=0), per.std(axis=0, ddof=1)
    mean, sd = float(out[0].mean()), float(out[0].std(ddof=1))
    mcse_m, mcse_s = means.std(ddof=1) / np.sqrt(K), sds.std(ddof=1) / np.sqrt(K)
    print(f"gamma case: mean {mean:.4f} (quadrature {q_mean:.4f}, mcse {mcse_m:.4f}), sd {sd:.4f} "
          f"(quadrature {q_sd:.4f}, mcse {mcse_s:.4f}), accept {info['accept_rate']}")
    assert abs(means.mean() - q_mean) <= 5 * mcse_m
    assert abs(sds.mean() - q_sd) <= 5 * mcse_s
    w = 1.0 / X[:, 0, :].var(axis=1, ddof=1)
    averaged = float((w[:, None] * X[:, 0, :]).sum(axis=0).mean() / w.sum())
    assert abs(mean - 2.25) < abs(averaged - 2.25)
