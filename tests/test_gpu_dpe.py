"""The semiparametric density-product combiner on the GPU: stk_dpe_prepare against tests/dpe_ref.py's longdouble
restatement, k_dpe_img against its host twin (identical index traces and accept counts), the bit-level contract,
and Stark.concensusWeight(combiner="semiparametric") end to end.

Every accuracy case prints a MAXERR line; the largest are kept in profiles/*_dpe_errors.json.

The sampler cases list S in {1, 17} with p up to 129: draws with S <= p have a singular covariance and the
prepare refuses them, so those cases run on dpe_ref.synthetic_prep's arrays (the sampler does not care where its
arrays came from); every S > p case, and the extra S = p + 2 cases, run on the device-prepared arrays."""
import os

import numpy as np
import pytest

import dpe_ref as dr

pytestmark = pytest.mark.gpu
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def conditioned_draws(rng, M, S, p, lp_row=True):
    """[M, P, S] draws whose sample covariance (of the p parameter rows) has condition number 100 exactly up to
    rounding: theta = mu + U diag(sigma) Q sqrt(S - 1), Q's p rows orthonormal and orthogonal to 1, sigma in [1, 10]."""
    X = np.zeros((M, p + (1 if lp_row else 0), S))
    for m in range(M):
        G = rng.standard_normal((S, p))
        G -= G.mean(axis=0)
        Q = np.linalg.qr(G)[0].T                               # p x S, rows orthonormal, each summing to 0
        U = np.linalg.qr(rng.standard_normal((p, p)))[0]
        sig = np.linspace(1.0, 10.0, p) if p > 1 else np.ones(1)
        X[m, :p] = rng.standard_normal((p, 1)) + (U * sig) @ Q * np.sqrt(S - 1)
        if lp_row:
            X[m, p] = rng.standard_normal(S) * rng.uniform(0.5, 2.0) - 40.0 - m
    return X


def rel(a, b):
    b = np.asarray(b, LD)
    return float(np.abs(np.asarray(a, LD) - b).max() / np.abs(b).max())


def check_prepare(got, ref, tag):
    M, p = ref["M"], ref["p"]
    assert got["M"] == M and got["p"] == p and got["ldp"] == ref["ldp"]
    errs = {k: rel(got[k], ref[k]) for k in ("Y", "n", "g", "mu", "L")}
    if ref["lp_row"]:
        errs["lp_w"] = rel(got["lp_w"], ref["lp_w"])
        assert np.array_equal(np.asarray(got["lpv"]), np.asarray(ref["lpv"], np.float64))
    print(f"MAXERR dpe_prepare {tag}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert np.all(np.asarray(got["Y"])[:, :, p:] == 0.0)      # pads
    assert np.all(np.triu(np.asarray(got["L"]), 1) == 0.0)
    for k in ("Y", "n", "g"):
        assert errs[k] <= 1e-10, (k, errs[k])
    for k in ("mu", "L"):
        assert errs[k] <= 1e-12, (k, errs[k])
    if ref["lp_row"]:
        assert errs["lp_w"] <= 1e-12
    return errs


@pytest.mark.parametrize("big_S", (False, True))
@pytest.mark.parametrize("p", (1, 2, 15, 16, 17, 63, 64, 65, 101, 128, 129))
@pytest.mark.parametrize("M", (1, 2, 8, 65))
def test_prepare_matches_the_longdouble_restatement(ctx, M, p, big_S):
    """S = p + 2 and S = 300, shard covariances of condition number 100: Y, n, g within 1e-10 of their largest
    magnitude, mu_M and L within 1e-12."""
    from stark_amd import engine
    S = 300 if big_S else p + 2
    X = conditioned_draws(np.random.default_rng(1000 * M + p), M, S, p)
    got = engine.dpe_prepare(list(X), ctx=ctx)
    assert got["shard_used"].all()
    check_prepare(got, dr.prepare(X), f"M={M} p={p} S={S}")


def test_prepare_without_an_lp_row(ctx):
    from stark_amd import engine
    X = conditioned_draws(np.random.default_rng(5), 3, 40, 17, lp_row=False)
    got = engine.dpe_prepare(list(X), lp_row=False, ctx=ctx)
    assert got["lpv"] is None and got["lp_w"] is None
    check_prepare(got, dr.prepare(X, lp_row=False), "no lp row M=3 p=17 S=40")


def test_a_nan_shard_is_left_out_and_changes_no_other_bit(ctx):
    from stark_amd import engine
    X = conditioned_draws(np.random.default_rng(6), 4, 30, 9)
    bad = X.copy()
    bad[2, 3, 11] = np.nan
    a = engine.dpe_prepare(list(bad), ctx=ctx)
    b = engine.dpe_prepare(list(X[[0, 1, 3]]), ctx=ctx)
    assert list(a["shard_used"]) == [True, True, False, True] and a["M"] == 3
    for k in ("mu", "L", "lp_w", "Y", "n", "g", "lpv"):
        assert np.array_equal(a[k], b[k]), k


def test_too_few_draws_raise_linalgerror(ctx):
    from stark_amd import engine
    from stark_amd._lib import LinAlgError
    rng = np.random.default_rng(7)
    with pytest.raises(LinAlgError, match="5 draws"):
        engine.dpe_prepare(list(rng.standard_normal((2, 6, 5))), ctx=ctx)          # S = p
    with pytest.raises(LinAlgError):
        engine.consensus_dpe(list(rng.standard_normal((2, 6, 4))), ctx=ctx)
    engine.dpe_prepare(list(rng.standard_normal((2, 6, 6))), ctx=ctx)                  # S = p + 1 is enough


def device_prep(ctx, M, S, p, seed):
    import torch
    from stark_amd import engine
    X = conditioned_draws(np.random.default_rng(seed), M, S, p)
    return engine.dpe_prepare(torch.as_tensor(X, device=f"cuda:{ctx.device}"), ctx=ctx)


def check_sampler(ctx, prep, tag, seed):
    """K in {1, 3, 130} x T in {1, K - 1, 2K + 1}, burn 0 / 5 and thin 1 / 3 alternating: traces and accept counts
    identical to the twin's, draws within 1e-12 of their scale."""
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    worst, i = 0.0, 0
    for K in (1, 3, 130):
        for T in (1, K - 1, 2 * K + 1):
            burn, thin = (0, 5)[i & 1], (1, 3)[(i >> 1) & 1]
            i += 1
            kw = dict(T=T, chains=K, burn=burn, thin=thin, bandwidth=(0.4, None)[i % 2], seed=seed + i, stream=i,
                      trace=True)
            if T == 0:
                with pytest.raises(StarkHipError, match="T = 0"):
                    engine.dpe_sample(prep, ctx=ctx, **kw)
                continue
            out, info = engine.dpe_sample(prep, ctx=ctx, **kw)
            ref, rinfo = engine.dpe_sample_host(prep, **kw)
            out = out.cpu().numpy() if hasattr(out, "cpu") else out
            assert out.shape == ref.shape == (prep["p"] + 1, T)
            assert np.array_equal(info["trace_idx"], rinfo["trace_idx"]), (tag, K, T)
            assert np.array_equal(info["accept"], rinfo["accept"]), (tag, K, T)
            assert np.array_equal(info["trace_logw"], rinfo["trace_logw"]), (tag, K, T)
            worst = max(worst, float(np.abs(out - ref).max() / np.abs(ref).max()))
    print(f"MAXERR dpe_sample {tag}: theta {worst:.3e}")
    assert worst <= 1e-12
    return worst


@pytest.mark.parametrize("S", (1, 17))
@pytest.mark.parametrize("M", (1, 2, 65))
@pytest.mark.parametrize("p", (1, 63, 64, 65, 129))
def test_sampler_matches_the_host_twin(ctx, p, M, S):
    if S > p + 1:
        prep = device_prep(ctx, M, S, p, 31 * p + M)
    else:
        prep = dr.synthetic_prep(np.random.default_rng(31 * p + M), M, S, p)
    check_sampler(ctx, prep, f"p={p} M={M} S={S}", 100 * p + M)


@pytest.mark.parametrize("p", (63, 64, 65, 129))
def test_sampler_matches_the_host_twin_on_device_prepared_arrays(ctx, p):
    check_sampler(ctx, device_prep(ctx, 2, p + 2, p, p), f"device-prepared p={p} M=2 S={p + 2}", 7 * p)


def test_bit_contract(ctx):
    """Host draws and device draws, a repeated call, the one-call path against prepare + sample: the same bits.
    Chains 0 .. 7 are the same under K = 8 and K = 16."""
    import torch
    from stark_amd import engine
    X = conditioned_draws(np.random.default_rng(8), 3, 50, 20)
    Xd = torch.as_tensor(X, device=f"cuda:{ctx.device}")
    kw = dict(T=37, chains=8, burn=3, thin=2, seed=11, stream=2)
    a, used, info = engine.consensus_dpe(list(X), ctx=ctx, **kw)
    b, used_b, info_b = engine.consensus_dpe(Xd, ctx=ctx, **kw)
    assert isinstance(a, np.ndarray) and b.is_cuda and used.all() and used_b.all()
    assert np.array_equal(a, b.cpu().numpy()) and np.array_equal(info["accept"], info_b["accept"])
    c, _, _ = engine.consensus_dpe(list(X), ctx=ctx, **kw)
    assert np.array_equal(a, c)
    prep = engine.dpe_prepare(list(X), ctx=ctx)
    d, info_d = engine.dpe_sample(prep, ctx=ctx, **kw)
    assert np.array_equal(a, d) and np.array_equal(info["accept"], info_d["accept"])
    assert info["h_first"] == 1.0 and 0 < info["h_last"] < 1 and info["sweeps"] == 3 + 2 * 5
    prep_d = engine.dpe_prepare(Xd, ctx=ctx)
    for k in ("mu", "L", "lp_w", "Y", "n", "g", "lpv"):
        assert np.array_equal(prep[k], prep_d[k].cpu().numpy()), k
    # chains 0 .. 7 under K = 8 and K = 16: the same sweeps (5 draws per chain), the same trajectories and draws
    e, info_e = engine.dpe_sample(prep, ctx=ctx, T=40, chains=8, burn=3, thin=2, seed=11, stream=2, trace=True)
    f, info_f = engine.dpe_sample(prep, ctx=ctx, T=80, chains=16, burn=3, thin=2, seed=11, stream=2, trace=True)
    assert np.array_equal(info_e["trace_idx"], info_f["trace_idx"][:8])
    assert np.array_equal(info_e["trace_logw"], info_f["trace_logw"][:8])
    assert np.array_equal(e.reshape(21, 5, 8), f.reshape(21, 5, 16)[:, :, :8])
    g, _, _ = engine.consensus_dpe(list(X), ctx=ctx, **dict(kw, seed=12))
    assert not np.array_equal(a, g)


def test_gaussian_shards_recover_the_product_moments(ctx):
    """Five-dimensional Gaussian shards: the combiner's draws have the parametric product's mean within 5
    between-chain MCSEs."""
    from stark_amd import engine
    rng = np.random.default_rng(9)
    X = rng.standard_normal((4, 5, 2000)) * rng.uniform(0.5, 2.0, (4, 5, 1)) + rng.standard_normal((4, 5, 1)) * 0.3
    K = 64
    out, used, info = engine.consensus_dpe(list(X), T=K * 40, chains=K, burn=100, thin=3, lp_row=False, ctx=ctx)
    ref = dr.prepare(X, lp_row=False)
    per = out.reshape(5, 40, K).mean(axis=1)
    mcse = per.std(axis=1, ddof=1) / np.sqrt(K)
    # the estimator's mean differs from mu_M by its own finite-S error, of the order of the shards' Monte Carlo error
    slack = np.sqrt(np.diag(np.asarray(ref["Sigma"], np.float64)) / 2000 * 4)
    assert np.all(np.abs(per.mean(axis=1) - np.asarray(ref["mu"], np.float64)) <= 5 * mcse + 5 * slack)
    assert np.all(info["accept_rate"] > 0)


def _schools(nparts=2):
    from stark_amd import stark
    from stark_amd.rdd import LocalContext
    sc = LocalContext()
    school = list(zip([28, 8, -3, 7, -1, 1, 18, 12], [15, 10, 16, 11, 9, 11, 10, 18]))
    st = stark.Stark(sc, sc.parallelize(school, nparts),
                     lambda p: {"J": len(p), "y": [v[0] for v in p], "sigma": [v[1] for v in p]})
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "schools.stan"))
    return st


def test_driver_end_to_end_on_eight_schools(ctx, monkeypatch):
    from stark_amd import engine
    st = _schools()
    kw = dict(iter=400, chains=2, seed=3)
    base = st.concensusWeight(**kw)
    assert np.array_equal(base, st.concensusWeight(combiner="consensus", **kw))     # the default path, bit for bit
    out = st.concensusWeight(combiner="semiparametric", combiner_args=dict(T=300, chains=32, burn=50, thin=2), **kw)
    assert out.shape == (base.shape[0], 300) and np.isfinite(out).all()
    assert np.array_equal(out, st.concensusWeight(combiner="semiparametric",
                                                  combiner_args=dict(T=300, chains=32, burn=50, thin=2), **kw))
    assert abs(out[-1].mean() - base[-1].mean()) < 10 * base[-1].std()             # lp__ is the last row
    assert st.combiner_info["accept_rate"].shape == (2,) and st.combiner_info["h_max"] == 1.0
    full = st.concensusWeight(combiner="semiparametric", **kw)                      # defaults: T = S, chains = min(T, 1024)
    assert full.shape == base.shape

    def boom(*a, **k):
        raise AssertionError("work was done")

    monkeypatch.setattr(engine, "Model", boom)
    with pytest.raises(ValueError, match="separate_lp"):
        st.concensusWeight(combiner="semiparametric", separate_lp=True, **kw)
    with pytest.raises(ValueError, match="weights"):
        st.concensusWeight(combiner="semiparametric", weights="laplace", **kw)
    with pytest.raises(ValueError, match="combiner"):
        st.concensusWeight(combiner="kde", **kw)
    with pytest.raises(ValueError, match="combiner_args"):
        st.concensusWeight(combiner_args=dict(T=5), **kw)
    with pytest.raises(ValueError, match="bandwith"):
        st.concensusWeight(combiner="semiparametric", combiner_args=dict(bandwith=0.3), **kw)
