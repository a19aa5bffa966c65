"""Any chains= per shard for the regression families: the C chains of a shard run as the contiguous
batches of engine.chain_batches(C, d), each batch one grouped sweep launch per shard group plus its
own k_sweep_reduce.  A chain's lp, gradient and draws depend only on its data, its RNG stream and the
size of the batch it sits in -- pinned here bit for bit against the single-batch runs, and against
the CPU oracle at the bars of test_gpu_sweep_shards.py."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_sweep_shards import GATED_ROWS, ROWS, _check_against_oracle, _grouped_case

pytestmark = pytest.mark.gpu


def _single_launch_before(B, d):
    """Batch sizes that log_density_grad_shards (the single-launch hook) takes at d."""
    return B in (1, 2, 4, 8, 64) or (B == 16 and d <= 128)


def _batches(C, d):
    from stark_amd import engine
    plan = engine.chain_batches(C, d)
    c0 = np.concatenate([[0], np.cumsum(plan)])
    return [(int(c0[i]), int(b)) for i, b in enumerate(plan)]


def _pmap(fn, items):
    """fn over items on 8 threads, in order (the oracle's C calls release the GIL)."""
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(fn, items))


# ---------------------------------------------------------------- 1. lp / grad through the plan
LPGRAD = [(100, 3), (50, 5), (100, 17), (100, 32), (100, 63), (100, 70), (100, 130), (129, 24), (200, 16), (300, 40)]


def _lpgrad_case(ctx, orc, family, d, C, tag, **prior):
    from stark_amd import engine
    okw = {f"prior_{k}": v for k, v in prior.items()}
    shards, oms, q = _grouped_case(orc, family, d, C, **okw)
    m = engine.Model(ctx, family, shards)
    if prior:
        m.set_prior(**prior)
    try:
        lp, g = m.log_density_grad_chains(q)
        assert lp.shape == (len(ROWS), C) and np.isfinite(lp).all() and np.isfinite(g).all()
        _check_against_oracle(oms, q, lp, g, f"{tag}[{family}-{d}-{C}] plan={engine.chain_batches(C, d)}")
        for c0, B in _batches(C, d):
            if not _single_launch_before(B, d):
                continue
            lp1, g1 = m.log_density_grad_shards(q[:, c0:c0 + B])
            np.testing.assert_array_equal(lp[:, c0:c0 + B], lp1, err_msg=f"batch {c0}+{B}")
            np.testing.assert_array_equal(g[:, c0:c0 + B], g1, err_msg=f"batch {c0}+{B}")
    finally:
        m.close()


@pytest.mark.parametrize("d,C", LPGRAD)
@pytest.mark.parametrize("family", ["logistic", "linear"])
def test_lpgrad_through_the_plan_matches_oracle(ctx, orc, family, d, C):
    """Six shards in five equal-n groups at C points each through the batches of a sampling run: vs the
    oracle, and every batch whose size was a single launch before equal, bit for bit, to that launch
    on the batch's own points."""
    _lpgrad_case(ctx, orc, family, d, C, "chains")


def test_lpgrad_through_the_plan_with_priors(ctx, orc):
    _lpgrad_case(ctx, orc, "logistic", 100, 3, "chains_prior", alpha=2.5, beta=0.3)


# ---------------------------------------------------------------- 2. sampler chains = the single-batch runs
def _one_shard(orc, family, d, n=600):
    rng = np.random.default_rng(1000 * d + n)
    X = rng.uniform(-1.7, 1.7, (n, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    if family == "logistic":
        y = (rng.uniform(size=n) < 1 / (1 + np.exp(-(0.2 + X @ beta)))).astype(np.int32)
    else:
        y = 0.3 + X @ beta + rng.normal(size=n)
    return {"x": X, "y": y}


def _run(m, chains, ids, nw=30, ns=20):
    s = m.sampler(num_warmup=nw, num_samples=ns, chains=chains, seed=21, shard_ids=ids)
    try:
        s.run()
        dr, st = s.draws(0)
        eps, im = s.adaptation()
        assert s.info()["errors"] == 0
        return dr.reshape(dr.shape[0], chains, ns), st.reshape(chains, ns, -1), eps, im
    finally:
        s.close()


@pytest.mark.parametrize("family,d,C", [("logistic", 100, 17), ("linear", 100, 17), ("logistic", 100, 3),
                                        ("linear", 100, 3), ("logistic", 200, 24), ("linear", 200, 24)])
def test_sampler_chains_equal_single_batch_runs(ctx, orc, family, d, C):
    """An adaptive run at a split count: the chains of batch (c0, B) give the draws, stats, step sizes
    and metric of a chains=B run with shard_ids=[c0 / B] (the same RNG streams c0 .. c0 + B - 1),
    bit for bit."""
    from stark_amd import engine
    m = engine.Model(ctx, family, [_one_shard(orc, family, d)])
    try:
        dr, st, eps, im = _run(m, C, [0])
        assert np.isfinite(dr).all()
        batches = _batches(C, d)
        assert len(batches) > 1
        for c0, B in batches:
            assert c0 % B == 0
            dr1, st1, eps1, im1 = _run(m, B, [c0 // B])
            np.testing.assert_array_equal(dr[:, c0:c0 + B], dr1, err_msg=f"draws of batch {c0}+{B}")
            np.testing.assert_array_equal(st[c0:c0 + B], st1, err_msg=f"stats of batch {c0}+{B}")
            np.testing.assert_array_equal(eps[c0:c0 + B], eps1)
            np.testing.assert_array_equal(im[c0:c0 + B], im1)
    finally:
        m.close()


# ---------------------------------------------------------------- 3. transitions with idle shards
def _gated_shards(orc, family, d, C):
    """The data recipe of test_gpu_sweep_shards.py::test_transition_gated_shards_match_oracle."""
    rng = np.random.default_rng(1000 * d + C)
    N = sum(GATED_ROWS)
    off = np.concatenate([[0], np.cumsum(GATED_ROWS)])
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    X = rng.uniform(-1.7, 1.7, (N, d))
    if family == "logistic":
        y = (rng.uniform(size=N) < 1 / (1 + np.exp(-(0.2 + X @ beta)))).astype(np.int32)
        fam, D = orc.FAM_LOGREG, d + 1
    else:
        y = 0.3 + X @ beta + rng.normal(size=N)
        fam, D = orc.FAM_LINREG, d + 2
    shards = [{"x": X[off[s]: off[s + 1]], "y": y[off[s]: off[s + 1]]} for s in range(3)]
    return shards, fam, D


def _gated_transition(ctx, orc, family, d, C, eps, tag, need_idle=True):
    from stark_amd import engine
    shards, fam, D = _gated_shards(orc, family, d, C)
    q0 = np.random.default_rng(5).normal(0, 0.1, (C, D))
    kw = dict(seed=7, iteration=11, eps=eps, max_depth=4)
    oms = [orc.Model(fam, X=sh["x"], y=sh["y"]) for sh in shards]
    flat = _pmap(lambda sc: oms[sc[0]].transition(q0[sc[1]], gid=sc[0] * C + sc[1], **kw),
                 [(s, c) for s in range(3) for c in range(C)])
    want = [flat[s * C:(s + 1) * C] for s in range(3)]
    longest = [max(int(w[2][3]) for w in ws) for ws in want]
    if need_idle:
        assert len(set(longest)) > 1, longest                   # (i) some shard idles while another sweeps
    divergent = sum(int(w[2][4]) for ws in want for w in ws)
    if divergent == 0:                                          # (ii) the chains moved
        moved = sum(bool(np.any(w[0] != q0[c])) for ws in want for c, w in enumerate(ws))
        assert 4 * moved >= 3 * 3 * C, moved
    else:
        assert {4, 5, 6} & {int(w[2][3]) for ws in want for w in ws}
    m = engine.Model(ctx, family, shards)
    try:
        got = [m.transition(s, q0, **kw) for s in range(3)]
    finally:
        m.close()
    eq = max(float((np.abs(got[s][0][c] - want[s][c][0]) / (1e-10 + 1e-8 * np.abs(want[s][c][0]))).max())
             for s in range(3) for c in range(C))
    elp = max(abs(got[s][1][c] - want[s][c][1]) / max(1.0, abs(want[s][c][1])) for s in range(3) for c in range(C))
    print(f"MAXERR {tag}[{family}-{d}-{C}-{eps}] plan={engine.chain_batches(C, d)} longest={longest} "
          f"divergent={divergent} q_over_bar={eq:.3e} lp_rel={elp:.3e}")
    for s in range(3):
        q, lp, st = got[s]
        for c in range(C):
            oq, olp, ost, _ = want[s][c]
            np.testing.assert_allclose(q[c], oq, rtol=1e-8, atol=1e-10, err_msg=f"shard {s} chain {c}")
            assert abs(lp[c] - olp) <= 1e-9 * max(1, abs(olp)), (s, c, lp[c], olp)
            assert st[c, 2] == ost[2] and st[c, 3] == ost[3] and st[c, 4] == ost[4], (s, c, st[c], ost)
            np.testing.assert_allclose(st[c, [0, 5]], ost[[0, 5]], rtol=1e-9, atol=1e-12)
    return divergent


GATED = ([("logistic", 100, 3, 0.05), ("logistic", 50, 5, 0.05), ("logistic", 100, 17, 0.1), ("logistic", 100, 32, 0.05),
          ("logistic", 129, 16, 0.05), ("logistic", 200, 16, 0.1)]
         + [("linear", d, C, 0.02) for d, C in ((100, 3), (50, 5), (100, 17), (129, 16), (100, 70))])
GATED_DIVERGENT = [("linear", 100, 32, 0.05), ("linear", 200, 16, 0.05)]


@pytest.mark.parametrize("family,d,C,eps", GATED)
def test_transition_split_counts_gated_shards_match_oracle(ctx, orc, family, d, C, eps):
    """One fixed-step transition of three shards whose trees end at different steps, at split chain
    counts: every batch's sweep and reduce must skip a finished shard.  Every chain vs the oracle's twin."""
    _gated_transition(ctx, orc, family, d, C, eps, "gated_chains")


@pytest.mark.parametrize("family,d,C,eps", GATED_DIVERGENT)
def test_transition_split_counts_divergent_exits_match_oracle(ctx, orc, family, d, C, eps):
    assert _gated_transition(ctx, orc, family, d, C, eps, "gated_chains_div") > 0


# ---------------------------------------------------------------- 4. dense_e
def test_transition_dense_metric_at_three_chains(ctx, orc):
    """One transition under a full D x D inverse metric at C = 3 (batches 2 + 1), d = 13, vs the
    oracle's dense twin at the bars of test_gpu_dense_oracle.py."""
    from stark_amd import engine
    from test_gpu_dense_oracle import _check_rows, _general_metric, _regression_rows
    d, C, n, eps = 13, 3, 400, 0.2
    (shard,), (om,) = _regression_rows(orc, "logistic", d, [n], 1000 * d + C)
    D = d + 1
    q0 = np.random.default_rng(5).normal(0, 0.1, (C, D))
    Minv = _general_metric(D, n)
    kw = dict(seed=41, inv_metric=Minv, factor=orc.cholesky(Minv), max_depth=6)
    want = [om.transition(q0[c], gid=c, iteration=6, eps=eps, **kw) for c in range(C)]
    assert any(bool(np.any(w[0] != q0[c])) for c, w in enumerate(want))
    m = engine.Model(ctx, "logistic", [shard])
    try:
        q, lp, st = m.transition(0, q0, seed=41, iteration=6, eps=eps, inv_metric=Minv, max_depth=6)
    finally:
        m.close()
    _check_rows(orc, f"dense_chains[logistic-{d}-{C}]", [((eps, c), q[c], lp[c], st[c], want[c][0], want[c][1], want[c][2])
                                                        for c in range(C)])


# ---------------------------------------------------------------- 5. checkpoint
def test_checkpoint_of_a_split_count(ctx, orc):
    """chains=17 at d = 100 saved mid-warmup by one sampler and resumed by another: bit-identical to the
    unsplit run.  A chains=16 blob is refused by the chains=17 sampler."""
    from stark_amd import engine
    m = engine.Model(ctx, "logistic", [_one_shard(orc, "logistic", 100)])
    cfg = dict(num_warmup=30, num_samples=20, chains=17, seed=21, shard_ids=[0])
    a = m.sampler(**cfg)
    b = m.sampler(**cfg)
    c = m.sampler(**cfg)
    e = m.sampler(**{**cfg, "chains": 16})
    try:
        a.run()
        b.run(17, max_steps=150)                 # mid-warmup, mid-trajectory
        assert int(b.iterations().min()) < 30
        c.load_state(b.save_state())
        c.run()
        for x, y in zip(a.draws(0), c.draws(0)):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(a.adaptation(), c.adaptation()):
            np.testing.assert_array_equal(x, y)
        assert a.info()["grad_evals"] == c.info()["grad_evals"]
        e.run(5)
        with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
            c.load_state(e.save_state())
    finally:
        for x in (a, b, c, e):
            x.close()
        m.close()


# ---------------------------------------------------------------- 6. the driver
def test_driver_three_chains(ctx, orc):
    """Stark.concensusWeight(chains=3) on a two-partition linear regression: P x S with S = 3 x the
    post-warmup draws, and the consensus mean within the batch MCSE of the closed-form posterior
    mean (estimator and bars of test_gpu_consensus.py, one chain per batch group)."""
    from stark_amd import stark
    from stark_amd.rdd import LocalContext
    from test_gpu_consensus import _batch_mcse_rel
    d, n_s, C, ns = 5, 400, 3, 200
    X = orc.gen_x(43, 0, 2 * n_s, d)
    y = orc.gen_y_linear(43, 0, X, 0.3, orc.gen_beta(43, d))
    rows = [(tuple(X[i]), float(y[i])) for i in range(2 * n_s)]
    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize(rows, 2), lambda data: {"N": len(data), "K": d, "x": [r[0] for r in data],
                                                                "y": [r[1] for r in data]})
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "linear.stan"))
    out = st.concensusWeight(chains=C, iter=2 * ns, seed=12, separate_lp=True, permuted=False)
    assert out.shape == (d + 3, C * ns) and np.isfinite(out).all()       # alpha, beta[5], sigma, lp__
    assert st.last_run.info["errors"] == 0
    mean, cov = orc.linreg_exact_moments(X, y)
    sd = np.sqrt(np.diag(cov))
    rel = _batch_mcse_rel(st.last_run.draws, C, ns, ctx, sd, groups=3)
    z = (out[:d + 1].mean(1) - mean) / (rel * sd)
    print(f"MAXERR driver_chains3 mean_z2={np.mean(z ** 2):.3f} max|z|={np.abs(z).max():.3f} rel_mcse={rel:.4f}")
    assert np.mean(z ** 2) < 2.5, (np.mean(z ** 2), rel)
    assert np.abs(z).max() < 4.5, (np.abs(z).max(), rel)


# ---------------------------------------------------------------- 7. refusals that remain
def test_refusals_that_remain(ctx):
    from stark_amd import engine
    rng = np.random.default_rng(3)
    m = engine.Model(ctx, "logistic", [{"x": rng.uniform(-1, 1, (40, 7)), "y": (rng.uniform(size=40) < 0.5).astype(np.int32)}])
    try:
        with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
            m.sampler(num_warmup=0, num_samples=1, chains=0)
    finally:
        m.close()
    big = engine.Model(ctx, "logistic", [{"x": rng.uniform(-1, 1, (40, 1024)), "y": (rng.uniform(size=40) < 0.5).astype(np.int32)}])
    try:
        with pytest.raises(engine.StarkHipError, match=r"too large \(max 1024\)"):
            big.sampler(num_warmup=0, num_samples=1, chains=3)
    finally:
        big.close()
