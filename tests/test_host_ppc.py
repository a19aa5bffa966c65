"""The posterior predictive generator's host twin (stk_yrep_host, compiled from csrc/yrep_math.h) against the
numpy restatement of include/stark_hip.h in tests/ppc_ref.py, its distribution, and the launch info.  No GPU.

An element is FRAGILE when the twin's margin -- the smallest relative gap of any comparison that decided it --
is below 1e-10: twin and restatement (whose exponentials differ in the last bits) must agree everywhere else,
and at most 1e-4 of a case's elements may be fragile."""
import math

import numpy as np
import pytest

import ppc_ref as R

MUS = (0.5, 9.99, 10.0, 50.0, 1e3, 1e6, 2.0 ** 30 * (1 - 2.0 ** -20), 2.0 ** 30 * (1 + 2.0 ** -20), 1e12)
GS = (1e-3, 0.5, 0.9)
NR, NS = 2048, 128
SEED = 20260


def test_counter_layout_is_pinned():
    """Three hand-computed counters: the linear replicate is eta + sigma sqrt(-2 log U) cos(2 pi V) of exactly these."""
    from stark_amd import engine
    cases = [  # (stream, row, draw), (c0, c1, c2, c3)
        ((5, 3, 7), (3, 0x700, 0x5000, 0x26)),
        ((2 ** 20 - 1, 2 ** 32 + 5, 2 ** 24 - 1), (5, 0xFFFFFF01, 0xFFFFF000, 0x26)),
        ((0, 2 ** 39 + 2 ** 31, 256), (0x80000000, 0x10080, 0, 0x26)),
    ]
    for (stream, row, draw), ctr in cases:
        ra, rb = engine.philox_words(SEED, *(np.uint64(c) for c in ctr))
        U, V = (((int(x) >> 11) + 0.5) * 2.0 ** -53 for x in (ra, rb))
        want = 0.25 + 2.0 * math.sqrt(-2.0 * math.log(U)) * math.cos(6.283185307179586 * V)
        got = engine.yrep_host("linear", SEED, stream, row, draw, [[0.25]], u=[math.log(2.0)])[0, 0]
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (stream, row, draw, got, want)
        assert tuple(int(c[0, 0]) for c in R.counters(stream, [row], [draw], 0)) == ctr
    # call j sits in the low 12 bits of the third word
    assert int(R.counters(9, [1], [2], 3)[2][0, 0]) == (9 << 12) | 3


def _eta_for(family, rng, n, S):
    if family == "poisson":          # mu from 0.01 to 1e3, both sides of 10, and the edges
        eta = rng.uniform(math.log(0.01), math.log(1e3), (n, S))
        eta[0, :8] = [-800.0, -40.0, math.log(10.0), math.log(9.999), 0.0, math.log(999.0), -1e-3, 2.0]
        return eta
    return rng.normal(0.0, 2.5, (n, S))


@pytest.mark.parametrize("family", R.FAMILIES)
def test_twin_equals_the_restatement(family):
    from stark_amd import engine
    rng = np.random.default_rng(11)
    n, S, row0, draw0, stream = 300, 64, 2 ** 33 + 17, 1000, 4
    eta = _eta_for(family, rng, n, S)
    u = rng.normal(-0.3, 0.5, S) if family == "linear" else None
    y, mg = engine.yrep_host(family, SEED, stream, row0, draw0, eta, u=u, margin=True)
    ref, att = R.yrep_np(family, SEED, stream, row0, draw0, eta, u)
    assert np.all(np.isfinite(y))
    if family == "linear":
        scale = np.maximum(1.0, np.abs(eta) + np.abs(ref - eta))
        assert np.all(np.abs(y - ref) <= 1e-12 * scale), float((np.abs(y - ref) / scale).max())
        return
    fragile = mg < R.FRAGILE
    print(f"{family}: fragile {int(fragile.sum())} of {fragile.size}, smallest margin {mg.min():.3g}, "
          f"most attempts {int(att.max())}")
    assert fragile.mean() <= 1e-4
    assert np.array_equal(y[~fragile], ref[~fragile])
    assert np.all(y == np.floor(y)) and y.min() >= 0
    if family == "poisson":
        assert y[0, 0] == 0.0 and y[0, 1] == 0.0          # mu = 0 and mu = 4e-18


def test_twin_non_finite_and_seeds():
    from stark_amd import engine
    bad = np.array([[np.nan, np.inf, -np.inf, 800.0]])
    assert np.all(np.isnan(engine.yrep_host("poisson", 1, 0, 0, 0, bad)[0, [0, 1, 3]]))
    assert engine.yrep_host("poisson", 1, 0, 0, 0, bad)[0, 2] == 0.0          # mu = 0
    assert np.all(np.isnan(engine.yrep_host("logistic", 1, 0, 0, 0, bad)[0, :1]))
    assert np.array_equal(engine.yrep_host("logistic", 1, 0, 0, 0, bad)[0, 1:], [1.0, 0.0, 1.0])
    assert np.all(np.isnan(engine.yrep_host("linear", 1, 0, 0, 0, bad, u=np.zeros(4))[0, :3]))
    assert np.all(np.isnan(engine.yrep_host("linear", 1, 0, 0, 0, np.zeros((1, 2)), u=[np.inf, np.nan])))
    eta = np.zeros((64, 32))
    a = engine.yrep_host("logistic", 1, 0, 0, 0, eta)
    assert not np.array_equal(a, engine.yrep_host("logistic", 2, 0, 0, 0, eta))
    assert not np.array_equal(a, engine.yrep_host("logistic", 1, 1, 0, 0, eta))
    # a window of rows and draws is the window of the whole
    assert np.array_equal(engine.yrep_host("logistic", 1, 0, 10, 5, eta[:20, :8]), a[10:30, 5:13])
    from stark_amd._lib import StarkHipError
    for kw, pat in ((dict(stream=2 ** 20), "stream"), (dict(draw0=2 ** 24 - 31), "draw")):
        args = dict(family="logistic", seed=1, stream=0, row0=0, draw0=0, eta=eta)
        args.update(kw)
        with pytest.raises(StarkHipError, match=pat):
            engine.yrep_host(**args)


def _moments(y, mean, var, mu4):
    """|z| of the sample mean and of the sample variance (exact variance of s^2: (mu4 - var^2 (N-3)/(N-1)) / N)."""
    N = y.size
    zm = abs(y.mean() - mean) / math.sqrt(var / N)
    zv = abs(y.var(ddof=1) - var) / math.sqrt((mu4 - var * var * (N - 3) / (N - 1)) / N)
    return zm, zv


@pytest.mark.parametrize("mu", MUS)
def test_poisson_distribution(mu):
    """2,048 rows x 128 draws at constant eta: mean and variance within 5 standard errors; for mu <= 50 every pmf
    cell of expected count >= 20 within 5 binomial sd; PTRS never needs more than 16 attempts."""
    from stark_amd import engine
    eta = np.full((NR, NS), math.log(mu))
    y = engine.yrep_host("poisson", SEED, 3, 0, 0, eta)
    mu_t = math.exp(math.log(mu))
    var = mu_t + (1.0 / 12.0 if mu_t >= R.NORMAL_MIN else 0.0)
    zm, zv = _moments(y, mu_t, var, mu_t + 3 * mu_t * mu_t)
    print(f"mu = {mu:g}: |z| mean {zm:.2f}, variance {zv:.2f}")
    assert zm <= 5 and zv <= 5
    assert np.all(y == np.floor(y)) and y.min() >= 0
    N = y.size
    if mu <= 50:
        worst = 0.0
        for k in range(int(y.max()) + 2):
            p = math.exp(-mu_t + k * math.log(mu_t) - math.lgamma(k + 1))
            if N * p >= 20:
                worst = max(worst, abs((y == k).sum() - N * p) / math.sqrt(N * p * (1 - p)))
        print(f"  largest pmf cell |z| {worst:.2f}")
        assert worst <= 5
    ref, att = R.yrep_np("poisson", SEED, 3, 0, 0, eta)
    if R.PTRS_MIN <= mu_t < R.NORMAL_MIN:
        print(f"  PTRS attempts: mean {att.mean():.3f}, most {int(att.max())}")
        assert 1 <= att.min() and att.max() <= 16
    else:
        assert att.max() == 0
    if mu <= 1e3:
        assert np.mean(y != ref) <= 1e-4
    else:                       # the restatement's distribution as well: its attempts are the ones counted
        assert all(z <= 5 for z in _moments(ref, mu_t, var, mu_t + 3 * mu_t * mu_t))


@pytest.mark.parametrize("g", GS)
def test_bernoulli_distribution(g):
    from stark_amd import engine
    y = engine.yrep_host("logistic", SEED, 3, 0, 0, np.full((NR, NS), math.log(g / (1 - g))))
    v = g * (1 - g)
    zm, zv = _moments(y, g, v, v * (1 - 3 * v))
    print(f"g = {g:g}: |z| mean {zm:.2f}, variance {zv:.2f}")
    assert zm <= 5 and zv <= 5 and set(np.unique(y)) <= {0.0, 1.0}


def test_normal_distribution():
    from stark_amd import engine
    y = engine.yrep_host("linear", SEED, 3, 0, 0, np.full((NR, NS), 1.5), u=np.full(NS, math.log(3.0)))
    zm, zv = _moments(y, 1.5, 9.0, 3 * 81.0)
    assert zm <= 5 and zv <= 5
    assert abs(np.mean(np.abs(y - 1.5) > 3 * 1.959963984540054) - 0.05) <= 5 * math.sqrt(0.05 * 0.95 / y.size)


def test_launch_info_and_refusals():
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    a, b = engine.ppc_launch(1000, 100, 16), engine.ppc_launch(1000, 100, 1024)
    assert a["T"] == 16 and a["waves"] == 4 and a["G"] >= 1
    assert all(a[k] == b[k] for k in ("T", "G", "waves", "lds_bytes"))        # none depends on S
    assert b["ws_bytes_per_shard"] == 8 * (128 * 64 + 8) * b["G"] and b["image_bytes"] > a["image_bytes"]
    assert a["G"] == engine.logdens_launch(1000, 100, 16)["G"]
    assert engine.ppc_launch(10 ** 7, 128, 16)["G"] == 256
    assert 2 * engine.ppc_launch(10 ** 7, 128, 16)["lds_bytes"] <= 160 * 1024  # two blocks per CU
    for d, S, pat in ((129, 16, "d = 129"), (1025, 16, "d = 1025"), (100, 0, "S = 0")):
        with pytest.raises(StarkHipError, match=pat) as e:
            engine.ppc_launch(100, d, S)
        assert e.value.code == -1


def test_ppc_pools_partitions():
    """engine.ppc on made-up arrays: sums add, extrema combine, the sd comes from the pooled sums."""
    from stark_amd import engine
    rng = np.random.default_rng(5)
    ys = [rng.poisson(3.0, n).astype(float) for n in (40, 25)]
    reps = [rng.poisson(3.0, (6, n)).astype(float) for n in (40, 25)]
    f = lambda v: [v.sum(), (v * v).sum(), v.max(), v.min(), (v == 0).sum()]
    obs = np.array([f(v) + [v.size, 0, 0] for v in ys])
    stats = np.array([[f(r) + [1.0 + s, 2.0, 0] for s, r in enumerate(rp)] for rp in reps])
    out = engine.ppc(stats, obs)
    ally, allr = np.concatenate(ys), np.concatenate(reps, axis=1)
    assert out["n"] == 65 and out["n_non_finite"] == 0
    assert abs(out["sd"]["obs"] - ally.std(ddof=1)) <= 1e-12
    assert np.allclose(out["sd"]["rep"], allr.std(axis=1, ddof=1), rtol=0, atol=1e-12)
    assert np.array_equal(out["max"]["rep"], allr.max(axis=1)) and out["min"]["obs"] == ally.min()
    assert out["mean"]["p"] == np.mean(allr.mean(axis=1) >= ally.mean())
    assert np.array_equal(out["chi2"]["rep"], 2.0 * (1.0 + np.arange(6))) and out["chi2"]["p"] == 0.0 + np.mean(
        2.0 * (1.0 + np.arange(6)) >= 4.0)
    ref = R.pool(stats, obs)
    for k in ref:
        assert np.array_equal(ref[k]["rep"], out[k]["rep"]) and ref[k]["p"] == out[k]["p"], k


def test_driver_refuses_before_any_device_work():
    """Stark.ppc: ValueError for more than 128 covariates and for 8 schools, worded like bootstrap's."""
    from stark_amd import stark
    from stark_amd.rdd import LocalContext, LocalRDD
    import os
    from conftest import ROOT
    st = stark.Stark(LocalContext(), LocalRDD([[(1.0,) * 130 + (1,)] * 4]),
                     lambda part: {"N": len(part), "K": 130, "x": np.array(part)[:, :130], "y": np.array(part)[:, 130].astype(int)})
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "logistic.stan"))
    with pytest.raises(ValueError, match="at most 128 covariates"):
        st.ppc(np.zeros((132, 8)))
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "schools.stan"))
    with pytest.raises(ValueError, match="8 schools"):
        st.ppc(np.zeros((11, 8)))
