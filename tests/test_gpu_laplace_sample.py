"""Laplace sampling end to end: engine.laplace_sample against a numpy replay of its pipeline, both sides of
the PSIS diagnostic, agreement with a NUTS run, and concensusWeight(method="laplace").

The replay takes the DEVICE's proposals and restates everything after them: lp in np.longdouble
(tests/test_gpu_logdens.py), log_q from the generator's restatement (Philox, Box-Muller), the PSIS fit
in np.longdouble (tests/test_host_laplace_sample.py).  Bars: log_ratio within 1e-10 of the density's
scale plus 1e-12 of max |theta - mode| (the two kernels' bars); khat within 1e-6 and ess within 1e-6
relative -- the log ratios entering the fit differ by about 2e-8 at these sizes, ess = 1 / sum w^2 moves by
at most twice that relatively, and the fit of at most 96 tail values is a smooth function of them; the
two orders on top cover its amplification.

The two shards of the diagnostic test: logistic, X ~ U(-1.7, 1.7), normal(0, 5) priors, S = 2000.  A numpy
prototype of the whole pipeline (its own Newton fit, the generator's restatement, the longdouble PSIS) gave,
over data seeds 1..3 x proposal seeds 1..4: 4000 rows, d = 5: ess / S in [0.996, 0.999], khat in
[0.05, 0.37]; 25 rows, d = 8: ess / S in [0.012, 0.172], khat in [0.48, 1.07].  The large shard is data seed
2, proposal seed 1 (prototype: 0.999, khat 0.21); the tiny one data seed 1, proposal seed 3 (prototype:
0.018, khat 1.07, so the warning fires with room).
"""
import os
import warnings

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_logdens import L, ref_laplace_draws, ref_ll, ref_lp
from test_host_laplace_sample import psis_ref

pytestmark = pytest.mark.gpu


def logistic_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.7, 1.7, (n, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    y = (rng.uniform(size=n) < 1 / (1 + np.exp(-(0.3 + X @ beta)))).astype(np.int32)
    return X, y


def small_model(family, n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.7, 1.7, (n, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    eta = 0.3 + X @ beta
    if family == "logistic":
        y = (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.int32)
    elif family == "poisson":
        y = rng.poisson(np.exp(eta)).astype(np.int32)
    else:
        y = eta + 0.7 * rng.normal(size=n)
    return X, y


@pytest.mark.parametrize("family,n,d,prior", (("logistic", 300, 3, (2.5, 1.5)), ("poisson", 200, 4, None),
                                              ("linear", 150, 3, None)))
def test_pipeline_replay(ctx, family, n, d, prior):
    from stark_amd import engine
    X, y = small_model(family, n, d, 40 + n)
    S, seed, stream = 500, 2024, 5
    m = engine.Model(ctx, family, [{"x": X, "y": y}])
    try:
        if prior:
            m.set_prior(*prior)
        res = engine.laplace_sample(m, 0, S, seed, stream=stream)
        again = engine.laplace_sample(m, 0, S, seed, stream=stream, fit=(res["mode"], res["cov"], res["info"]))
        for k in ("draws", "lp", "proposals", "log_ratio", "log_w"):
            assert np.array_equal(res[k], again[k]), k                          # a given fit is reused, bit for bit
    finally:
        m.close()
    D = res["mode"].size
    assert res["draws"].shape == (S, D) and res["proposals"].shape == (S, D) and res["lp"].shape == (S,)
    rlp, scale = ref_lp(family, ref_ll(family, X, y, res["proposals"]), res["proposals"], d, prior)
    rq, rlq = ref_laplace_draws(res["mode"], engine.laplace_factor(res["cov"]), S, seed, stream)
    spread = float(np.abs(rq - res["mode"].astype(L)).max())
    assert float(np.abs(res["proposals"] - rq).max()) <= 1e-12 * spread
    rratio = rlp - rlq
    bar = 1e-10 * scale + 1e-12 * spread
    err = float((np.abs(res["log_ratio"].astype(L) - rratio) / bar).max())
    rw, rk = psis_ref(rratio.astype(np.float64))
    ress = float(1 / (np.exp(rw) ** 2).sum())
    print(f"MAXERR laplace_replay family={family} log_ratio={err:.3e} (units of its bar) khat={res['khat']:.4f} "
          f"khat_err={abs(res['khat'] - float(rk)):.3e} ess={res['ess']:.1f} ess_rel_err={abs(res['ess'] / ress - 1):.3e}")
    assert err <= 1.0
    assert abs(res["khat"] - float(rk)) <= 1e-6
    assert abs(res["ess"] / ress - 1) <= 1e-6
    assert float(np.abs(res["log_w"].astype(L) - rw).max()) <= 1e-6
    # the resampled draws are rows of the proposals, drawn by engine.resample from the smoothed weights
    idx = engine.resample(res["log_w"], S, seed, stream)
    assert np.array_equal(res["draws"], res["proposals"][idx])
    assert float(np.abs(res["lp"].astype(L) - rlp[idx]).max()) <= 1e-10 * float(scale.max())


@pytest.fixture(scope="module")
def large_shard(ctx):
    """The 4000 x 5 logistic shard under normal(0, 5) priors, its Laplace sample and a short NUTS run."""
    from stark_amd import engine
    X, y = logistic_rows(4000, 5, 2)
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        m.set_prior(5.0, 5.0)
        res = engine.laplace_sample(m, 0, 2000, 1)
        nuts = m.sample(num_warmup=300, num_samples=500, chains=4, seed=17)
    finally:
        m.close()
    return res, nuts


def test_large_shard_has_a_trustworthy_proposal(large_shard):
    res, _ = large_shard
    print(f"MAXERR laplace_large ess_over_S={res['ess'] / 2000:.4f} khat={res['khat']:.4f}")
    assert res["ess"] / 2000 > 0.9


def test_tiny_shard_is_flagged(ctx):
    from stark_amd import engine, stark
    from stark_amd.rdd import LocalContext
    X, y = logistic_rows(25, 8, 1)
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        m.set_prior(5.0, 5.0)
        res = engine.laplace_sample(m, 0, 2000, 3)
    finally:
        m.close()
    print(f"MAXERR laplace_tiny ess_over_S={res['ess'] / 2000:.4f} khat={res['khat']:.4f}")
    assert res["ess"] / 2000 < 0.2
    # the front end names the partition and sends the user to NUTS
    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize([tuple(r) for r in np.column_stack([X, y])], 1),
                     lambda p: {"N": len(p), "K": 8, "x": np.array(p)[:, :8], "y": np.array(p)[:, 8].astype(np.int64)})
    st.setStanModel(family="logistic", priors={"alpha": 5.0, "beta": 5.0})
    with pytest.warns(RuntimeWarning, match=r"partition 0.*NUTS"):
        out = st.concensusWeight(method="laplace", iter=4000, warmup=2000, chains=1, seed=3)
    assert out.shape == (10, 2000)
    assert st.laplace_diagnostics["khat"][0] == res["khat"] and st.laplace_diagnostics["ess"][0] == res["ess"]


def test_weighted_means_agree_with_nuts(large_shard):
    from stark_amd import diagnostics
    res, nuts = large_shard
    assert nuts.info["errors"] == 0
    w = np.exp(res["log_w"])
    lap = w @ res["proposals"]
    d = nuts.draws[0][:6]
    mcse = d.std(axis=1, ddof=1) / np.sqrt(diagnostics.ess_matrix(d, 4))
    z = (lap - d.mean(axis=1)) / mcse
    print(f"MAXERR laplace_vs_nuts max_abs_z_in_nuts_mcse={np.abs(z).max():.3f}")
    assert np.all(np.abs(z) < 5.0)
    assert np.all(np.abs(res["draws"].mean(axis=0) - lap) < 5.0 * d.std(axis=1, ddof=1) / np.sqrt(res["ess"]))


PROGRAM = os.path.join(ROOT, "stark_amd", "models", "logistic.stan")


def _stark(rows, k, nparts, program=PROGRAM):
    from stark_amd import stark
    from stark_amd.rdd import LocalContext

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": k, "x": a[:, :k], "y": a[:, k].astype(np.int64)}

    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize(rows, nparts), prep)
    st.setStanModel(file=program)
    return st, prep


def test_front_end(ctx):
    from stark_amd import rdd as _rdd
    rng = np.random.default_rng(4)
    X = rng.uniform(-1.7, 1.7, (1600, 4))
    y = (rng.uniform(size=1600) < 1 / (1 + np.exp(-(0.2 + X @ np.array([0.5, -0.4, 0.3, 0.1]))))).astype(np.int64)
    st, prep = _stark([tuple(r) for r in np.column_stack([X, y])], 4, 4)
    a = st.concensusWeight(chains=4, iter=300, seed=5)
    b = st.concensusWeight(chains=4, iter=300, seed=5, method="nuts")
    assert np.array_equal(a, b)                                                 # the default path, bit for bit
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                          # 400 rows, d = 4: no partition is flagged
        lap = st.concensusWeight(chains=4, iter=300, seed=5, method="laplace")
    assert lap.shape == a.shape == (6, 600) and np.isfinite(lap).all()
    diag = st.laplace_diagnostics
    assert len(diag["khat"]) == len(diag["ess"]) == 4 and all(1.0 <= e <= 600.0 * (1 + 1e-12) for e in diag["ess"])
    assert np.all(np.abs(lap[:5].mean(1) - a[:5].mean(1)) < 0.1)                # the same posterior, loosely
    assert st.concensusWeight(chains=2, iter=300, thin=3, seed=5, method="laplace").shape == (6, 100)
    sel = st.concensusWeight(chains=4, iter=300, seed=5, method="laplace", pars=["beta"])
    assert sel.shape == (5, 600)                                                # beta[4] + lp__
    full_sep = st.concensusWeight(chains=4, iter=300, seed=5, method="laplace", separate_lp=True)
    lw = st.concensusWeight(chains=4, iter=300, seed=5, method="laplace", weights="laplace")
    assert full_sep.shape == lw.shape == a.shape and np.isfinite(lw).all()
    assert np.all(np.abs(lw[:5].mean(1) - full_sep[:5].mean(1)) < 0.05)
    # rows: lp__ is the log density at the draw; two partitions in one model equal the same two run apart
    datas = [prep(list(p)) for p in _rdd.partitions_of(st.rdd)]
    kw = dict(chains=4, iter=300, seed=5, n_jobs=1)
    both, _, dboth = st._laplace_partitions([datas[1], datas[3]], shard_ids=[1, 3], **kw)
    one, _, d1 = st._laplace_partitions([datas[1]], shard_ids=[1], **kw)
    three, _, d3 = st._laplace_partitions([datas[3]], shard_ids=[3], **kw)
    assert np.array_equal(both[0], one[0]) and np.array_equal(both[1], three[0])
    assert np.array_equal(dboth[0], d1[0]) and np.array_equal(dboth[1], d3[0])
    other, _, _ = st._laplace_partitions([datas[1]], shard_ids=[2], **kw)        # the stream is the global index
    assert not np.array_equal(other[0], one[0])
    from stark_amd import engine
    m = engine.Model(ctx, "logistic", [{"x": datas[1]["x"], "y": datas[1]["y"].astype(np.int32)}])
    try:
        assert np.array_equal(m.log_density(np.ascontiguousarray(one[0][:5].T), 0), one[0][5])
    finally:
        m.close()


def test_laplace_method_refuses_schools_and_wide_models_before_any_work(monkeypatch):
    from stark_amd import engine, stark
    from stark_amd.rdd import LocalContext
    sc = LocalContext()
    school = list(zip([28, 8, -3, 7, -1, 1, 18, 12], [15, 10, 16, 11, 9, 11, 10, 18]))
    st = stark.Stark(sc, sc.parallelize(school, 2),
                     lambda p: {"J": len(p), "y": [v[0] for v in p], "sigma": [v[1] for v in p]})
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "schools.stan"))

    def boom(*a, **k):
        raise AssertionError("work was done")

    monkeypatch.setattr(engine, "Model", boom)
    with pytest.raises(ValueError, match="schools"):
        st.concensusWeight(method="laplace", iter=200)
    with pytest.raises(ValueError, match="method"):
        st.concensusWeight(method="pathfinder", iter=200)
    rng = np.random.default_rng(0)
    rows = [tuple(r) for r in np.column_stack([rng.normal(size=(300, 129)), rng.integers(0, 2, 300)])]
    st, _ = _stark(rows, 129, 2)
    with pytest.raises(ValueError, match="K = 129"):
        st.concensusWeight(method="laplace", iter=200)
