"""Laplace fits on the analytic Hessian (engine.laplace), the combine with the caller's weights
(stk_consensus_weighted) and concensusWeight(weights="laplace"), on the GPU.

References: tools.laplace.laplace (Newton on the central-difference Hessian of the library's own
gradient; its error in the sds is <= 8.2e-6 at these shapes) and tools.laplace.consensus_fixed_weights
(numpy).  Figures are printed as MAXERR lines.
"""
import os
import socket

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_hessian import make_data

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. engine.laplace on one shard
@pytest.mark.parametrize("n,d", [(333, 5), (1000, 128), (4096, 100)])
@pytest.mark.parametrize("family", ("logistic", "poisson", "linear"))
def test_laplace_from_zero_matches_the_difference_newton(ctx, family, n, d):
    from stark_amd import engine
    from tools import laplace as L
    _, X, y, _ = make_data(family, n, d)
    m = engine.Model(ctx, family, [{"x": X, "y": y}])
    try:
        mode, cov, info = engine.laplace(m, q0=None)
        sd = np.sqrt(np.diag(cov))
        print(f"MAXERR laplace_info[{family}-{n}-{d}] hessians={info['hessians']} kinds={info['kinds']} "
              f"halvings={info['halvings']}")
        if family == "linear":
            assert info["kinds"][0] == "block" and info["kinds"][-1] == "newton"
        else:
            assert set(info["kinds"]) == {"newton"} and sum(info["halvings"]) <= 1
        m2, c2, _ = L.laplace(m, [0], mode, sd)
        sd2 = np.sqrt(np.diag(c2))
        dm, dsd = float(np.abs((m2 - mode) / sd).max()), float(np.abs(sd2 / sd - 1).max())
        print(f"MAXERR laplace_vs_difference[{family}-{n}-{d}] mode_in_sd={dm:.3e} sd_ratio={dsd:.3e}")
        assert dm < 1e-4 and dsd < 1e-4
        if family == "linear":
            Xt = np.concatenate([np.ones((n, 1)), X], axis=1)
            ols, *_ = np.linalg.lstsq(Xt, y, rcond=None)
            r = y - Xt @ ols
            e1 = float(np.abs(mode[:-1] - ols).max() / np.abs(ols).max())
            e2 = float(abs(np.exp(2 * mode[-1]) / (r @ r / (n - 1)) - 1))
            print(f"MAXERR laplace_linear_closed_form[{n}-{d}] theta={e1:.3e} sigma2={e2:.3e}")
            assert e1 < 1e-9 and e2 < 1e-12
    finally:
        m.close()


# ---------------------------------------------------------------- 2. several shards, reduce=
def _four_shards():
    _, X, y, _ = make_data("logistic", 1200, 10, seed=77)
    return X, y, [{"x": X[k * 300:(k + 1) * 300], "y": y[k * 300:(k + 1) * 300]} for k in range(4)]


def _rank_worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from stark_amd import engine
        _, _, shards = _four_shards()
        m = engine.Model(engine.default_context(0), "logistic", shards[2 * rank:2 * rank + 2])

        def reduce(v):
            t = torch.from_numpy(v)
            dist.all_reduce(t)

        mode, cov, info = engine.laplace(m, reduce=reduce)
        q.put((rank, mode, cov, info["hessians"]))
        m.close()
    finally:
        dist.destroy_process_group()


def test_laplace_over_shards_and_ranks(ctx):
    """4 shards = the one shard of their concatenated rows (modes within 1e-9 sd); 2 ranks of 2 shards
    each, summed by a gloo all-reduce, reach that mode too, with the same bits on both ranks."""
    import torch.multiprocessing as mp
    from stark_amd import engine
    X, y, shards = _four_shards()
    m4 = engine.Model(ctx, "logistic", shards)
    m1 = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        mode4, cov4, _ = engine.laplace(m4)
        mode1, cov1, _ = engine.laplace(m1)
        sd = np.sqrt(np.diag(cov1))
        e = float(np.abs((mode4 - mode1) / sd).max())
        print(f"MAXERR laplace_4_shards_vs_concatenated mode_in_sd={e:.3e}")
        assert e < 1e-9
        np.testing.assert_allclose(cov4, cov1, rtol=1e-9, atol=1e-12 * np.abs(cov1).max())
        sub, _, _ = engine.laplace(m4, shards=[1, 3])              # an explicit subset: per-shard calls
        assert np.abs((sub - mode1) / sd).max() > 1e-3
    finally:
        m4.close()
        m1.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    s_ = socket.socket()
    s_.bind(("127.0.0.1", 0))
    port = s_.getsockname()[1]
    s_.close()
    procs = [mpc.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    assert float(np.abs((res[0][1] - mode1) / sd).max()) < 1e-9


# ---------------------------------------------------------------- 3. stk_consensus_weighted
def _wishart_case(P, ns, S=200, seed=0):
    rng = np.random.default_rng(1000 * P + ns + seed)
    W = []
    for _ in range(ns):
        A = rng.normal(size=(P, 4 * P))
        W.append(A @ A.T / (4 * P))
    assert np.linalg.cond(sum(W)) <= 100
    draws = [rng.normal(size=(P, S)) + rng.normal(size=(P, 1)) for _ in range(ns)]
    return draws, W


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("ns", (2, 3, 8))
@pytest.mark.parametrize("P", (11, 53, 102, 131))
def test_consensus_weighted_matches_numpy(ctx, P, ns, device):
    import torch
    from stark_amd import engine
    from tools import laplace as L
    draws, W = _wishart_case(P, ns)
    ref = L.consensus_fixed_weights(draws, W)
    arg = torch.as_tensor(np.stack(draws)).cuda() if device else draws
    out, used = engine.consensus_weighted(arg, W, ctx)
    out = out.cpu().numpy() if device else out
    err = float(np.abs(out - ref).max() / np.abs(ref).max())
    print(f"MAXERR consensus_weighted[P{P}-{ns}-{'device' if device else 'host'}] {err:.3e}")
    assert used.all() and err < 1e-12


def test_consensus_weighted_nan_draws_and_nan_weights(ctx):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    from tools import laplace as L
    draws, W = _wishart_case(11, 3, seed=5)
    bad = [d.copy() for d in draws]
    bad[1][4, 17] = np.nan
    out, used = engine.consensus_weighted(bad, W, ctx)
    ref = L.consensus_fixed_weights([draws[0], draws[2]], [W[0], W[2]])
    assert list(used) == [True, False, True]
    assert np.abs(out - ref).max() < 1e-12 * np.abs(ref).max()
    Wn = [w.copy() for w in W]
    Wn[2][3, 3] = np.nan
    with pytest.raises(StarkHipError, match="shard 2") as e:
        engine.consensus_weighted(draws, Wn, ctx)
    assert e.value.code == -1
    out, used = engine.consensus_weighted([draws[0], draws[1], bad[1]], Wn, ctx)   # NaN weights of a NaN shard: left out
    assert list(used) == [True, True, False]


@pytest.mark.parametrize("device", (False, True))
def test_consensus_with_weights_gives_lp_its_own_block(ctx, device):
    import torch
    from stark_amd import engine
    from tools import laplace as L
    draws, W = _wishart_case(12, 3, seed=9)                      # 11 parameter rows + lp__
    for s, d in enumerate(draws):
        d[-1] = 50.0 * s + 3.0 * d[-1]                           # every shard's lp__ at its own offset
    Wp = [w[:-1, :-1] for w in W]
    out, used = engine.consensus(torch.as_tensor(np.stack(draws)).cuda() if device else draws, ctx, weights=Wp)
    out = out.cpu().numpy() if device else out
    ref = L.consensus_fixed_weights([d[:-1] for d in draws], Wp)
    sep, _ = engine.consensus(draws, ctx, separate_lp=True)
    assert used.all()
    assert np.abs(out[:-1] - ref).max() < 1e-12 * np.abs(ref).max()
    np.testing.assert_allclose(out[-1], sep[-1], rtol=1e-12)


# ---------------------------------------------------------------- 4. end to end
PROGRAM = os.path.join(ROOT, "stark_amd", "models", "logistic.stan")


def _stark_logistic(rows, k, nparts):
    from stark_amd import stark
    from stark_amd.rdd import LocalContext

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": k, "x": a[:, :k], "y": a[:, k].astype(np.int64)}

    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize(rows, nparts), prep)
    st.setStanModel(file=PROGRAM)
    assert st.family == "logistic"
    return st, prep


def test_laplace_weights_end_to_end(ctx):
    """Logistic d = 50, 8 shards x 20,000 rows, 16 chains, 200 warmup + 100 draws, through the driver.
    On the same draws the combined means lie closer to the full-data Laplace mode with the per-shard
    Laplace weights than with the sampled weights (separate_lp=True, the parent's accurate path), and
    within the batch MCSE bar of tests/test_gpu_consensus.py."""
    from stark_amd import engine
    from stark_amd import rdd as _rdd
    d, S, n_s, C, nw, ns = 50, 8, 20_000, 16, 200, 100
    rng = np.random.default_rng(2024)
    X = rng.uniform(-1.7, 1.7, (S * n_s, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    y = (rng.uniform(size=S * n_s) < 1 / (1 + np.exp(-(0.3 + X @ beta)))).astype(np.int64)
    rows = [tuple(r) for r in np.column_stack([X, y])]
    st, prep = _stark_logistic(rows, d, S)
    out = st.concensusWeight(weights="laplace", chains=C, iter=nw + ns, warmup=nw, permuted=False, seed=31)
    assert out.shape == (d + 2, C * ns) and np.isfinite(out).all()
    assert st.last_run.info["errors"] == 0
    draws = st.last_run.draws
    shards = [prep(list(p)) for p in _rdd.partitions_of(st.rdd)]
    m = engine.Model(ctx, "logistic", [{"x": s["x"], "y": s["y"]} for s in shards])
    try:
        W = []
        for s in range(S):
            _, cov, _ = engine.laplace(m, [s], q0=draws[s][:d + 1].mean(axis=1))
            W.append(np.linalg.inv(cov))
        comb, used = engine.consensus(draws, ctx, weights=W)
        assert used.all()
        np.testing.assert_allclose(out, comb, rtol=1e-12, atol=0)
        mode, cov, _ = engine.laplace(m)                          # the full-data posterior: the sum of the shards
        sd = np.sqrt(np.diag(cov))
        samp, _ = engine.consensus(draws, ctx, separate_lp=True)
        z2_lap = float(np.mean(((comb[:d + 1].mean(1) - mode) / sd) ** 2))
        z2_smp = float(np.mean(((samp[:d + 1].mean(1) - mode) / sd) ** 2))
        groups, cg, gm = 4, C // 4, []
        for g in range(groups):                                   # batch MCSE: groups of chains, the weights held fixed
            sel = [np.ascontiguousarray(x[:, g * cg * ns:(g + 1) * cg * ns]) for x in draws]
            c, _ = engine.consensus(sel, ctx, weights=W)
            gm.append(c[:d + 1].mean(1))
        rel = float(np.sqrt(np.mean(np.var(np.array(gm), axis=0, ddof=1) / groups / sd ** 2)))
        z2_mcse = float(np.mean(((comb[:d + 1].mean(1) - mode) / (rel * sd)) ** 2))
        print(f"MAXERR end_to_end mean_z2_laplace_weights={z2_lap:.4e} mean_z2_sampled_weights={z2_smp:.4e} "
              f"batch_mcse_rel={rel:.4e} mean_z2_in_mcse={z2_mcse:.4e}")
        assert z2_lap < z2_smp
        assert z2_mcse < 2.5
    finally:
        m.close()


def test_laplace_weights_refuse_schools_before_sampling(monkeypatch):
    from stark_amd import stark
    from stark_amd.rdd import LocalContext
    sc = LocalContext()
    school = list(zip([28, 8, -3, 7, -1, 1, 18, 12], [15, 10, 16, 11, 9, 11, 10, 18]))
    st = stark.Stark(sc, sc.parallelize(school, 2),
                     lambda p: {"J": len(p), "y": [v[0] for v in p], "sigma": [v[1] for v in p]})
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "schools.stan"))

    def boom(*a, **k):
        raise AssertionError("sampled")

    monkeypatch.setattr(st, "_run_distributed", boom)
    with pytest.raises(ValueError, match="schools"):
        st.concensusWeight(weights="laplace", iter=200)
    with pytest.raises(ValueError, match="weights"):
        st.concensusWeight(weights="exact", iter=200)


def test_sample_weights_are_the_default_path(ctx):
    """weights="sample" is today's call, bit for bit; pars= selects the rows of the Laplace weights too."""
    rng = np.random.default_rng(4)
    X = rng.uniform(-1.7, 1.7, (1200, 4))
    y = (rng.uniform(size=1200) < 1 / (1 + np.exp(-(0.2 + X @ np.array([0.5, -0.4, 0.3, 0.1]))))).astype(np.int64)
    st, _ = _stark_logistic([tuple(r) for r in np.column_stack([X, y])], 4, 4)
    a = st.concensusWeight(chains=4, iter=300, seed=5)
    b = st.concensusWeight(chains=4, iter=300, seed=5, weights="sample")
    assert np.array_equal(a, b)
    a = st.concensusWeight(chains=4, iter=300, seed=5, separate_lp=True)
    b = st.concensusWeight(chains=4, iter=300, seed=5, separate_lp=True, weights="sample")
    assert np.array_equal(a, b)
    lap = st.concensusWeight(chains=4, iter=300, seed=5, weights="laplace")
    assert lap.shape == a.shape and np.isfinite(lap).all()
    assert np.all(np.abs(lap[:5].mean(1) - a[:5].mean(1)) < 0.1)       # the same posterior, loosely
    sel = st.concensusWeight(chains=4, iter=300, seed=5, weights="laplace", pars=["beta"])
    assert sel.shape == (5, a.shape[1])                                  # beta[4] + lp__
    assert np.all(np.abs(sel[:4].mean(1) - a[1:5].mean(1)) < 0.1)


def test_linear_laplace_weights_are_in_the_constrained_space(ctx):
    """Linear family through the driver: the draw rows hold sigma = e^u, so the weights are the inverse
    of J (-H)^-1 J with J = diag(1, .., 1, sigma_hat) -- restated here from engine.laplace."""
    from stark_amd import engine, stark
    from stark_amd import rdd as _rdd
    from stark_amd.rdd import LocalContext
    rng = np.random.default_rng(6)
    k = 3
    X = rng.uniform(-1.7, 1.7, (2000, k))
    y = 0.4 + X @ np.array([0.5, -0.3, 0.2]) + 0.6 * rng.normal(size=2000)

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": k, "x": a[:, :k], "y": a[:, k]}

    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize([tuple(r) for r in np.column_stack([X, y])], 4), prep)
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "linear.stan"))
    assert st.family == "linear"
    out = st.concensusWeight(weights="laplace", chains=4, iter=400, permuted=False, seed=8)
    draws = st.last_run.draws
    shards = [prep(list(p)) for p in _rdd.partitions_of(st.rdd)]
    m = engine.Model(ctx, "linear", [{"x": s["x"], "y": s["y"]} for s in shards])
    if st.priors:
        m.set_prior(**st.priors)
    try:
        W = []
        for s in range(4):
            q0 = draws[s][:k + 2].mean(axis=1)
            q0[-1] = np.log(q0[-1])
            mode, cov, _ = engine.laplace(m, [s], q0=q0)
            J = np.diag(np.concatenate([np.ones(k + 1), [np.exp(mode[-1])]]))
            W.append(np.linalg.inv(J @ cov @ J))
        ref, _ = engine.consensus(draws, ctx, weights=W)
    finally:
        m.close()
    np.testing.assert_allclose(out, ref, rtol=1e-10, atol=0)
    Xt = np.concatenate([np.ones((2000, 1)), X], axis=1)
    ols, *_ = np.linalg.lstsq(Xt, y, rcond=None)
    assert np.all(np.abs(out[:k + 1].mean(1) - ols) < 0.05)
    assert abs(out[k + 1].mean() - 0.6) < 0.05
