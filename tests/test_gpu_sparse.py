"""Sparse (CSR) design matrices: a second storage for the six regression families (stk_model_create_sparse,
k_sweep_sp).  The sparse sweeps against the references the dense sweeps use, evaluated on the densified matrix,
at the project's 1e-10 bars; against the dense model of the same matrix on the GPU; bit-reproducible; the sampler
replayed by the oracle; checkpoints; the driver; and the entry points that refuse a sparse model by name.

STARK_SPARSE_ERRORS_OUT=<file>: the parity tests' largest errors, in units of the bars, are written there as JSON
(profiles/r30a_sparse_errors.json is such a run)."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_sweep_shards import _check_against_oracle, _rel

pytestmark = pytest.mark.gpu

import scipy.sparse as sp  # noqa: E402

FAMILIES = ["linear", "logistic", "poisson", "neg_binomial", "student_t", "gamma"]
WIDTHS = [1, 2, 16, 129, 512, 513, 1024]
PATTERNS = ["empty", "onehot", "mixed"]
ROWS = [1, 77, 1483]        # one model of three shards: three launch groups, G = 1 chunk each
POINTS = 31                 # 16 + 8 + 4 + 2 + 1 where 16 is a batch size (d <= 512), else 8 + 8 + 8 + 4 + 2 + 1
NU = 4.0
RTOL = 1e-10

_ERRORS = {}


@pytest.fixture(scope="module", autouse=True)
def _write_errors():
    yield
    out = os.environ.get("STARK_SPARSE_ERRORS_OUT")
    if out and _ERRORS:
        with open(out, "w") as f:
            json.dump({"bars": "lp: |err| / max(|lp|, 1) over 1e-10; grad: |err| / max(|g_j|, 1e-3 (max|g| + 1)) over 1e-10",
                       "cases": _ERRORS}, f, indent=1, sort_keys=True)


def _matrix(pattern, n, d, rng):
    """A scipy CSR matrix of n x d.  empty: no entry (K = 0).  onehot: every row has 1 .. min(8, d) ones.
    mixed: values in U(-1.7, 1.7), about a quarter of the rows empty, the others 1 .. min(12, d) entries, and
    row n // 2 fully dense (K = d)."""
    if pattern == "empty":
        return sp.csr_matrix((n, d))
    rows, cols, vals = [], [], []
    for r in range(n):
        if pattern == "onehot":
            k = int(rng.integers(1, min(8, d) + 1))
            v = np.ones(k)
        elif r == n // 2:
            k = d
            v = rng.uniform(-1.7, 1.7, k) / np.sqrt(d)
        elif rng.uniform() < 0.25:
            continue
        else:
            k = int(rng.integers(1, min(12, d) + 1))
            v = rng.uniform(-1.7, 1.7, k)
        c = np.sort(rng.choice(d, k, replace=False))
        rows += [r] * k
        cols += list(c)
        vals += list(v)
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, d))


def _response(family, eta, rng):
    n = eta.shape[0]
    if family == "logistic":
        return (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.int32)
    if family == "poisson":
        return rng.poisson(np.exp(np.clip(eta, -20, 6))).astype(np.int32)
    if family == "neg_binomial":
        mu = np.exp(np.clip(eta, -20, 6))
        return rng.poisson(mu * rng.gamma(3.0, 1 / 3.0, n)).astype(np.int32)
    if family == "student_t":
        return eta + 0.7 * rng.standard_t(NU, n)
    if family == "gamma":
        return np.exp(eta) * rng.gamma(5.0, 1 / 5.0, n)
    return eta + rng.normal(size=n)


def _case(family, d, pattern, rows=ROWS, points=POINTS, seed=0):
    """Sparse shards, their densified twins and `points` points per shard."""
    rng = np.random.default_rng(100003 * d + 17 * FAMILIES.index(family) + PATTERNS.index(pattern) + seed)
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    sparse, dense = [], []
    for n in rows:
        X = _matrix(pattern, n, d, rng)
        Xd = np.asarray(X.todense(), np.float64)
        y = _response(family, 0.3 + Xd @ beta, rng)
        sparse.append({"x": X, "y": y})
        dense.append({"x": Xd, "y": y})
    D = d + (1 if family in ("logistic", "poisson") else 2)
    q = rng.normal(0, 0.2, (len(rows), points, D))
    return sparse, dense, q


def _model(engine, ctx, family, shards):
    return engine.Model(ctx, family, shards, **({"nu": NU} if family == "student_t" else {}))


def _reference(orc, family, dense, q):
    """lp [nshards][C] and grad [nshards][C][D] of the family's reference on the densified rows (longdouble where the
    reference is numpy), or the oracle's models for linear and logistic."""
    if family in ("linear", "logistic"):
        fam = orc.FAM_LINREG if family == "linear" else orc.FAM_LOGREG
        return [orc.Model(fam, X=sh["x"], y=sh["y"]) for sh in dense]
    if family == "poisson":
        from test_gpu_poisson import ref_lpgrad
        return [ref_lpgrad(sh["x"], sh["y"], q[s]) for s, sh in enumerate(dense)]
    if family == "neg_binomial":
        import negbin_ref as R
        return [R.ref_lpgrad(sh["x"], sh["y"], q[s]) for s, sh in enumerate(dense)]
    if family == "student_t":
        import student_ref as R
        return [R.ref_lpgrad(sh["x"], sh["y"], q[s], NU) for s, sh in enumerate(dense)]
    import gamma_ref as R
    return [R.ref_lpgrad(sh["x"], sh["y"], q[s]) for s, sh in enumerate(dense)]


def _bars(lp, g, olp, og):
    """The largest lp and gradient errors of one shard's points in units of the 1e-10 bars (check_bars's own)."""
    wl = wg = 0.0
    for c in range(len(olp)):
        o = np.float64(olp[c])
        ogc = np.asarray(og[c], np.float64)
        wl = max(wl, float(abs(lp[c] - o) / max(abs(o), 1.0)) / RTOL)
        bar = RTOL * np.maximum(np.abs(ogc), (np.abs(ogc).max() + 1.0) * 1e-3)
        wg = max(wg, float((np.abs(g[c] - ogc) / bar).max()))
    return wl, wg


def _check(family, tag, ref, q, lp, g):
    """The project's bars, exactly as _check_against_oracle (linear, logistic) and check_bars (the others) apply
    them; the largest errors are printed first, in units of the bars."""
    from test_gpu_poisson import check_bars
    if family in ("linear", "logistic"):
        wl = wg = 0.0
        for s, om in enumerate(ref):
            for c in range(q.shape[1]):
                olp, og = om.lpgrad(q[s, c])
                wl = max(wl, float(_rel(lp[s, c], olp)) / RTOL)
                bar = RTOL * np.maximum(np.abs(og), 1e-3 * (np.abs(og).max() + 1.0))      # _check_against_oracle's own
                wg = max(wg, float((np.abs(g[s, c] - og) / bar).max()))
        print(f"MAXERR {tag} lp_over_bar={wl:.3e} grad_over_bar={wg:.3e}")
        _ERRORS.setdefault(tag, {}).update(lp_over_bar=wl, grad_over_bar=wg)
        _check_against_oracle(ref, q, lp, g, tag)
        return
    worst = [_bars(lp[s], g[s], *ref[s]) for s in range(len(ref))]
    wl, wg = max(w[0] for w in worst), max(w[1] for w in worst)
    print(f"MAXERR {tag} lp_over_bar={wl:.3e} grad_over_bar={wg:.3e}")
    _ERRORS.setdefault(tag, {}).update(lp_over_bar=wl, grad_over_bar=wg)
    for s in range(len(ref)):
        check_bars(lp[s], g[s], ref[s][0], ref[s][1], where=(tag, s))


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("family", FAMILIES)
def test_sparse_lpgrad_matches_the_dense_references(ctx, orc, family, d, pattern):
    """31 points per shard through the sparse batch table of d (16 + 8 + 4 + 2 + 1 where 16 is a batch size) against
    the family's reference on the densified matrix, and against the dense model of the same matrix on the GPU, at
    the same bars (not bitwise: the summation order differs)."""
    from stark_amd import engine
    from test_gpu_poisson import check_bars
    sparse, dense, q = _case(family, d, pattern)
    plan = engine.chain_batches(POINTS, d, sparse=True)
    assert plan == ([16, 8, 4, 2, 1] if d <= 512 else [8, 8, 8, 4, 2, 1])
    ms = _model(engine, ctx, family, sparse)
    md = _model(engine, ctx, family, dense)
    try:
        assert ms.sparse and not md.sparse
        for s, sh in enumerate(sparse):
            info = ms.sparse_info(s)
            K = int(np.diff(sh["x"].indptr).max()) if sh["x"].nnz else 0
            assert info == {"K": K, "nnz": int(sh["x"].nnz), "bytes": 12 * K * ROWS[s]}, info   # the layout's bytes
            if pattern == "mixed" and ROWS[s] > 1:
                assert K == d
            if pattern == "empty":
                assert K == 0
        assert "x" not in ms.device_arrays(0) and "x" in md.device_arrays(0)
        lp, g = ms.log_density_grad_chains(q)
        lpd, gd = md.log_density_grad_chains(q)
    finally:
        ms.close()
        md.close()
    assert np.isfinite(lp).all() and np.isfinite(g).all()
    tag = f"sparse[{family}-{d}-{pattern}]"
    _check(family, tag, _reference(orc, family, dense, q), q, lp, g)
    worst = [_bars(lp[s], g[s], lpd[s], gd[s]) for s in range(len(ROWS))]
    wl, wg = max(w[0] for w in worst), max(w[1] for w in worst)
    print(f"MAXERR {tag} vs_dense lp_over_bar={wl:.3e} grad_over_bar={wg:.3e}")
    _ERRORS.setdefault(tag, {}).update(vs_dense_lp_over_bar=wl, vs_dense_grad_over_bar=wg)
    for s in range(len(ROWS)):
        check_bars(lp[s], g[s], lpd[s], gd[s], where=(tag, "dense model", s))


def test_sparse_priors_and_scalar_priors(ctx):
    """set_prior (normal priors, and the gamma family's shape prior) on a sparse model: the reduce is the dense one."""
    from stark_amd import engine
    import gamma_ref as R
    from test_gpu_poisson import check_bars
    sparse, dense, q = _case("gamma", 16, "mixed", rows=[300], points=5)
    m = _model(engine, ctx, "gamma", sparse)
    try:
        m.set_prior(alpha=2.0, beta=0.5, shape=(2.0, 0.5))
        lp, g = m.log_density_grad_chains(q)
    finally:
        m.close()
    check_bars(lp[0], g[0], *R.ref_lpgrad(dense[0]["x"], dense[0]["y"], q[0], shape_prior=(2.0, 0.5), prior=(2.0, 0.5)),
               where="sparse priors")


# ---------------------------------------------------------------- 2. reproducibility
REPRO = [("logistic", 16, "onehot"), ("linear", 129, "mixed"), ("neg_binomial", 513, "mixed"), ("poisson", 512, "onehot"),
         ("student_t", 2, "mixed"), ("gamma", 1024, "mixed")]


@pytest.mark.parametrize("family,d,pattern", REPRO)
def test_sparse_bits_do_not_depend_on_the_launch(ctx, family, d, pattern):
    """The same call twice; every shard alone in a model of its own against the grouped launches (two shards of
    equal n share one); every batch of the plan against its single launch (log_density_grad_shards); one point per
    call through log_density_grad: equal bits every time."""
    from stark_amd import engine
    rows = [700, 77, 77, 2500]                # groups of 1, 2 and 1 shards; 2500 rows: two chunks
    sparse, _, q = _case(family, d, pattern, rows=rows, points=POINTS, seed=5)
    m = _model(engine, ctx, family, sparse)
    try:
        lp, g = m.log_density_grad_chains(q)
        lp2, g2 = m.log_density_grad_chains(q)
        np.testing.assert_array_equal(lp, lp2)
        np.testing.assert_array_equal(g, g2)
        plan = engine.chain_batches(POINTS, d, sparse=True)
        c0 = 0
        for B in plan:
            lp1, g1 = m.log_density_grad_shards(q[:, c0:c0 + B])
            np.testing.assert_array_equal(lp[:, c0:c0 + B], lp1, err_msg=f"batch {c0}+{B}")
            np.testing.assert_array_equal(g[:, c0:c0 + B], g1, err_msg=f"batch {c0}+{B}")
            c0 += B
        lp3, g3 = m.log_density_grad(3, q[3, -1:])            # the last batch is one chain
        np.testing.assert_array_equal(lp[3, -1:], lp3)
        np.testing.assert_array_equal(g[3, -1:], g3)
    finally:
        m.close()
    for s in range(len(rows)):
        one = _model(engine, ctx, family, [sparse[s]])
        try:
            lps, gs = one.log_density_grad_chains(q[s:s + 1])
        finally:
            one.close()
        np.testing.assert_array_equal(lp[s:s + 1], lps, err_msg=f"shard {s} alone")
        np.testing.assert_array_equal(g[s:s + 1], gs, err_msg=f"shard {s} alone")


def test_sparse_storage_does_not_change_the_bits(ctx):
    """A shard whose tiles are staged in LDS (K = 8) and the same rows in a shard whose longest row is d (one
    extra row, K = d = 400: its entries are read from global memory) give the same lp and gradient bits for the
    shared rows' part -- checked through a shard that differs only by a row of explicit zeros."""
    from stark_amd import engine
    rng = np.random.default_rng(11)
    n, d = 500, 400
    X = _matrix("onehot", n, d, rng)
    y = (rng.uniform(size=n + 1) < 0.5).astype(np.int32)
    wide = sp.vstack([X, sp.csr_matrix((np.zeros(d), (np.zeros(d, int), np.arange(d))), shape=(1, d))]).tocsr()
    narrow = sp.vstack([X, sp.csr_matrix((1, d))]).tocsr()
    assert wide.nnz == X.nnz + d                                   # explicit zeros are kept
    q = rng.normal(0, 0.2, (1, 16, d + 1))
    a = engine.Model(ctx, "logistic", [{"x": narrow, "y": y}])
    b = engine.Model(ctx, "logistic", [{"x": wide, "y": y}])
    try:
        assert a.sparse_info(0)["K"] == 8 and b.sparse_info(0)["K"] == d
        assert engine.sparse_launch(n + 1, d, 8, 16)["staged"] == 1 and engine.sparse_launch(n + 1, d, d, 16)["staged"] == 0
        la, ga = a.log_density_grad_chains(q)
        lb, gb = b.log_density_grad_chains(q)
    finally:
        a.close()
        b.close()
    np.testing.assert_array_equal(la, lb)
    np.testing.assert_array_equal(ga, gb)


# ---------------------------------------------------------------- 3. the sampler
def _transition_rows(orc, family, d, C, n=400):
    rng = np.random.default_rng(1000 * d + C)
    X = _matrix("mixed", n, d, rng)
    Xd = np.asarray(X.todense(), np.float64)
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    y = _response(family, 0.2 + Xd @ beta, rng)
    fam, D = (orc.FAM_LOGREG, d + 1) if family == "logistic" else (orc.FAM_LINREG, d + 2)
    return {"x": X, "y": y}, orc.Model(fam, X=Xd, y=y), D


@pytest.mark.parametrize("family,d,C,eps", [("logistic", 13, 3, 0.05), ("logistic", 40, 17, 0.05), ("linear", 13, 17, 0.02),
                                            ("linear", 40, 3, 0.02)])
def test_sparse_transition_diag_e_matches_oracle(ctx, orc, family, d, C, eps):
    """A few fixed-step transitions of a sparse shard at 3 (2 + 1) and 17 (16 + 1) chains, replayed by the oracle on
    the densified rows: treedepth, n_leapfrog and divergent equal, q and lp at the bars of test_gpu_chain_batches.py."""
    from stark_amd import engine
    shard, om, D = _transition_rows(orc, family, d, C)
    q0 = np.random.default_rng(5).normal(0, 0.1, (C, D))
    m = engine.Model(ctx, family, [shard])
    try:
        for it in (11, 12):
            kw = dict(seed=7, iteration=it, eps=eps, max_depth=4)
            q, lp, st = m.transition(0, q0, **kw)
            for c in range(C):
                oq, olp, ost, _ = om.transition(q0[c], gid=c, **kw)
                np.testing.assert_allclose(q[c], oq, rtol=1e-8, atol=1e-10, err_msg=f"iteration {it} chain {c}")
                assert abs(lp[c] - olp) <= 1e-9 * max(1, abs(olp)), (it, c, lp[c], olp)
                assert st[c, 2] == ost[2] and st[c, 3] == ost[3] and st[c, 4] == ost[4], (it, c, st[c], ost)
                np.testing.assert_allclose(st[c, [0, 5]], ost[[0, 5]], rtol=1e-9, atol=1e-12)
            assert any(bool(np.any(q[c] != q0[c])) for c in range(C))
    finally:
        m.close()


@pytest.mark.parametrize("C", [3, 17])
def test_sparse_transition_dense_e_matches_oracle(ctx, orc, C):
    """One transition under a full D x D inverse metric on a sparse shard vs the oracle's dense-metric twin, with the
    helpers and bars of test_gpu_dense_oracle.py."""
    from stark_amd import engine
    from test_gpu_dense_oracle import _check_rows, _general_metric
    d, n, eps = 13, 400, 0.2
    shard, om, D = _transition_rows(orc, "logistic", d, C, n)
    q0 = np.random.default_rng(5).normal(0, 0.1, (C, D))
    Minv = _general_metric(D, n)
    kw = dict(seed=41, inv_metric=Minv, factor=orc.cholesky(Minv), max_depth=6)
    want = [om.transition(q0[c], gid=c, iteration=6, eps=eps, **kw) for c in range(C)]
    m = engine.Model(ctx, "logistic", [shard])
    try:
        q, lp, st = m.transition(0, q0, seed=41, iteration=6, eps=eps, inv_metric=Minv, max_depth=6)
    finally:
        m.close()
    _check_rows(orc, f"sparse_dense_e[logistic-{d}-{C}]", [((eps, c), q[c], lp[c], st[c], want[c][0], want[c][1], want[c][2])
                                                         for c in range(C)])


@pytest.mark.parametrize("metric", ["diag_e", "dense_e", "unit_e"])
@pytest.mark.parametrize("criterion", [0, 1])
def test_sparse_sampler_runs_every_metric_and_criterion(ctx, metric, criterion):
    """A short adaptive run of a sparse poisson model at 5 chains: finite draws, no stopped chain; the same run twice
    gives the same bits."""
    from stark_amd import engine
    sparse, _, _ = _case("poisson", 16, "onehot", rows=[400, 300])
    m = engine.Model(ctx, "poisson", sparse)
    try:
        cfg = dict(num_warmup=30, num_samples=20, chains=5, seed=3, metric=metric, nuts_criterion=criterion)
        a = m.sample(**cfg)
        b = m.sample(**cfg)
    finally:
        m.close()
    assert a.info["errors"] == 0
    for x, y in zip(a.draws, b.draws):
        assert np.isfinite(x).all()
        np.testing.assert_array_equal(x, y)


def test_sparse_checkpoint_resumes_bit_identically_and_is_bound_to_its_storage(ctx):
    """chains = 17 on a sparse logistic shard saved mid-warmup by one sampler and resumed by another: the draws of the
    unsplit run.  A blob saved against the DENSE model of the same matrix is refused as saved against other data."""
    from stark_amd import engine
    sparse, dense, _ = _case("logistic", 40, "onehot", rows=[600])
    m = engine.Model(ctx, "logistic", sparse)
    md = engine.Model(ctx, "logistic", dense)
    cfg = dict(num_warmup=30, num_samples=20, chains=17, seed=21, shard_ids=[0])
    a, b, c, e = m.sampler(**cfg), m.sampler(**cfg), m.sampler(**cfg), md.sampler(**cfg)
    try:
        assert m.fingerprint(0) != md.fingerprint(0)
        assert m.fingerprint(0) == engine.shard_fingerprint("logistic", sparse[0])
        a.run()
        b.run(17, max_steps=150)
        assert int(b.iterations().min()) < 30
        c.load_state(b.save_state())
        c.run()
        for x, y in zip(a.draws(0), c.draws(0)):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(a.adaptation(), c.adaptation()):
            np.testing.assert_array_equal(x, y)
        e.run(5)
        with pytest.raises(engine.StarkHipError, match="other data"):
            c.load_state(e.save_state())
    finally:
        for x in (a, b, c, e):
            x.close()
        m.close()
        md.close()


# ---------------------------------------------------------------- 4. the driver
def test_sparse_partitions_through_the_driver(ctx):
    """Two partitions of 2,000 rows with 40 one-hot columns, logistic, handed over as scipy matrices: the consensus
    posterior means within four combined MCSE of the dense-path run on the densified rows.  The semiparametric
    combiner and distribute run on the same partitions."""
    from stark_amd import stark
    from stark_amd.rdd import LocalContext
    from test_gpu_consensus import _batch_mcse_rel
    d, n_s, C, ns = 40, 2000, 8, 100
    rng = np.random.default_rng(77)
    col = rng.integers(0, d, 2 * n_s)
    beta = rng.normal(0, 0.7, d)
    y = (rng.uniform(size=2 * n_s) < 1 / (1 + np.exp(-(0.2 + beta[col])))).astype(int)
    rows = [(int(col[i]), int(y[i])) for i in range(2 * n_s)]

    def prep(as_sparse):
        def cb(data):
            c = np.array([r[0] for r in data])
            X = sp.csr_matrix((np.ones(len(data)), (np.arange(len(data)), c)), shape=(len(data), d))
            return {"N": len(data), "K": d, "x": X if as_sparse else np.asarray(X.todense()), "y": [r[1] for r in data]}
        return cb

    out, runs = {}, {}
    for as_sparse in (True, False):
        sc = LocalContext()
        st = stark.Stark(sc, sc.parallelize(rows, 2), prep(as_sparse))
        st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "logistic_prior.stan"))
        out[as_sparse] = st.concensusWeight(chains=C, iter=2 * ns, seed=12, permuted=False)
        runs[as_sparse] = st.last_run
        assert out[as_sparse].shape == (d + 2, C * ns) and np.isfinite(out[as_sparse]).all()
        assert st.last_run.info["errors"] == 0
        if as_sparse:
            semi = st.concensusWeight(chains=2, iter=100, seed=12, combiner="semiparametric")
            assert semi.shape[0] == d + 2 and np.isfinite(semi).all()
            dist_out = st.distribute(n=2, chains=2, iter=60, seed=12)
            assert np.isfinite(np.asarray(dist_out)).all()
            for what, call in (("waic", lambda: st.waic(out[True])), ("loo", lambda: st.loo(out[True])),
                               ("ppc", lambda: st.ppc(out[True])), ("bootstrap", lambda: st.bootstrap(n=16)),
                               ("weights", lambda: st.concensusWeight(chains=2, iter=60, seed=12, weights="laplace")),
                               ("method", lambda: st.concensusWeight(chains=2, iter=60, seed=12, method="laplace"))):
                with pytest.raises(ValueError, match="sparse"):
                    call()
    sd = out[False][:d + 1].std(1)
    rel = np.hypot(_batch_mcse_rel(runs[True].draws, C, ns, ctx, sd, groups=4), _batch_mcse_rel(runs[False].draws, C, ns, ctx, sd, groups=4))
    z = (out[True][:d + 1].mean(1) - out[False][:d + 1].mean(1)) / (rel * sd)
    print(f"MAXERR sparse_driver max|z|={np.abs(z).max():.3f} combined_rel_mcse={rel:.4f}")
    assert np.abs(z).max() < 4.0, (np.abs(z).max(), rel)


# ---------------------------------------------------------------- 5. refusals
def test_every_other_entry_point_refuses_a_sparse_model_by_name(ctx):
    """The analysis sweeps and full-data mode return STK_E_ARG with a message that says the model is sparse, before
    any launch; the model still samples afterwards."""
    from stark_amd import engine
    sparse, _, q = _case("logistic", 16, "onehot", rows=[300], points=4)
    m = engine.Model(ctx, "logistic", sparse)
    draws = q[0]
    try:
        calls = {
            "hessian": lambda: m.hessian(0, draws[0]),
            "log_predictive": lambda: m.log_predictive(draws),
            "loo": lambda: m.loo(draws),
            "log_density": lambda: m.log_density(draws),
            "bootstrap": lambda: m.log_density_grad_boot(draws),
            "posterior_predict": lambda: m.posterior_predict(draws),
        }
        for name, call in calls.items():
            with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG.*sparse") as ei:
                call()
            assert ei.value.code == -1, name
        s = m.sampler(num_warmup=5, num_samples=5, chains=2, seed=1)
        try:
            with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG.*sparse"):
                s.set_allreduce(lambda ptr, count, stream: 0)
        finally:
            s.close()
        res = m.sample(num_warmup=20, num_samples=10, chains=3, seed=2)
        assert res.info["errors"] == 0 and all(np.isfinite(dr).all() for dr in res.draws)
    finally:
        m.close()


def test_sparse_creation_refusals_name_shard_and_row(ctx):
    """Through engine.Model (the C ABI on the device's context): an index equal to d in shard 1, a NaN value; a
    model of mixed storage."""
    from stark_amd import engine
    y = np.array([0, 1, 1], np.int32)
    good = {"x_csr": ([0, 1, 1, 2], [0, 3], [1.0, 2.0]), "d": 4, "y": y}
    with pytest.raises(engine.StarkHipError, match=r"shard 1: row 2: index 4 is outside \[0, 4\)"):
        engine.Model(ctx, "logistic", [good, {"x_csr": ([0, 1, 1, 2], [0, 4], [1.0, 2.0]), "d": 4, "y": y}])
    with pytest.raises(engine.StarkHipError, match=r"shard 0: row 0: .*not finite"):
        engine.Model(ctx, "logistic", [{"x_csr": ([0, 1, 1, 2], [0, 3], [np.nan, 2.0]), "d": 4, "y": y}])
    with pytest.raises(ValueError, match="all sparse or all dense"):
        engine.Model(ctx, "logistic", [good, {"x": np.zeros((3, 4)), "y": y}])
    with pytest.raises(ValueError, match="y must be 0 or 1"):                 # the y checks are the dense path's
        engine.Model(ctx, "logistic", [dict(good, y=np.array([0, 2, 1]))])


def test_device_resident_csr_arrays_are_checked_and_give_the_host_model(ctx):
    """stk_model_create_sparse on indptr, indices and values that lie in device memory (torch tensors): the same
    fingerprint, lp and gradient as the model of the host arrays; a bad index, unsorted indices, a decreasing indptr
    and a NaN in device memory are refused with the shard and the row, before anything is launched."""
    import ctypes
    import torch
    from stark_amd import _lib, engine
    sparse, _, q = _case("logistic", 16, "mixed", rows=[300], points=4)
    indptr, indices, values, d = engine.canonical_csr(sparse[0])
    y = np.ascontiguousarray(sparse[0]["y"], np.int32)

    def create(ip, ix, vv):
        t = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (ip, ix, vv)]
        torch.cuda.synchronize()
        sh = _lib.ShardSparse(len(ip) - 1, d, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), None, y.ctypes.data)
        h = ctypes.c_void_p()
        rc = _lib.load().stk_model_create_sparse(ctx._h, _lib.STK_LOGREG, ctypes.byref(sh), 1, ctypes.byref(h))
        return rc, h, _lib.load().stk_last_error().decode()

    rc, h, _ = create(indptr, indices, values)
    assert rc == 0
    host = engine.Model(ctx, "logistic", sparse)
    dev = engine.Model.__new__(engine.Model)                      # takes the handle over, as Model.synthetic does
    dev._nshards = 1
    engine.Model.__init__(dev, ctx, "logistic", None, _handle=h)
    try:
        dev.sparse = True
        assert dev.fingerprint(0) == host.fingerprint(0) and dev.sparse_info(0) == host.sparse_info(0)
        for a, b in zip(dev.log_density_grad_chains(q), host.log_density_grad_chains(q)):
            np.testing.assert_array_equal(a, b)
    finally:
        dev.close()
        host.close()
    row = int(np.flatnonzero(np.diff(indptr) >= 2)[0])
    e0 = int(indptr[row])
    bad_index, unsorted, nan = indices.copy(), indices.copy(), values.copy()
    bad_index[e0] = d
    unsorted[e0], unsorted[e0 + 1] = indices[e0 + 1], indices[e0]
    nan[e0] = np.nan
    down = indptr.copy()
    down[row + 1] = indptr[row] - 1 if indptr[row] > 0 else -1
    for what, args, msg in (("index", (indptr, bad_index, values), rf"shard 0: row {row}: index {d} is outside \[0, {d}\)"),
                            ("unsorted", (indptr, unsorted, values), rf"shard 0: row {row}: indices must be strictly increasing"),
                            ("nan", (indptr, indices, nan), rf"shard 0: row {row}: .*not finite"),
                            ("indptr", (down, indices, values), rf"shard 0: row {row}: indptr decreases")):
        import re
        rc, _, err = create(*args)
        assert rc == -1 and re.search(msg, err), (what, rc, err)
