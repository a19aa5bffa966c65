"""The categorical family (softmax regression, K = ncat classes) on the GPU: k_sweep_cat's lp / gradient against the
longdouble reference tests/categorical_ref.py (the density of include/stark_hip.h, STK_CATEGORICAL) over the envelope's
shapes, K = 2 against the oracle's logistic density, relabelled classes, extreme coefficients, priors, chain batches and
grouped launches bit for bit, the oracle's logistic NUTS replaying K = 2 transitions, sampling against an exact grid
posterior, determinism and checkpoints, the metrics and U-turn criteria, the Stark driver, and the family's refusals.

Bars: check_bars of tests/test_gpu_gamma.py (the project's 1e-10 density bars), restated here.

Inputs.  X, alpha and beta are dyadic (X multiples of 2^-6 in [-1.7, 1.7], the coefficients multiples of 2^-10), as
tests/test_gpu_gamma.py builds them: every product x_ij beta_gj and every partial sum of eta is exact in fp64 whatever
the order of the sum, so eta reaches the residual without rounding error, on the device as in the reference.
"""
import os

import numpy as np
import pytest

import categorical_ref as R

pytestmark = pytest.mark.gpu

FAM = "categorical"
RTOL = 1e-10


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


def dyadic(v, bits):
    return np.round(np.asarray(v) * 2.0 ** bits) / 2.0 ** bits


def make_data(n, d, ncat, seed=None, classes="all"):
    """X ~ U(-1.7, 1.7) and coefficients ~ N(0, 1 / sqrt(d)), dyadic; y drawn from the softmax of the data's own
    coefficients.  classes: "all"; "missing" (class 2 never occurs: its rows become class 1); "reference" (every row
    class ncat); "first" (every row class 1)."""
    rng = np.random.default_rng(100000 * ncat + 1000 * n + d if seed is None else seed)
    G = ncat - 1
    X = dyadic(rng.uniform(-1.7, 1.7, (n, d)), 6)
    q0 = dyadic(np.concatenate([rng.normal(0, 0.5, G), rng.normal(0, 1 / np.sqrt(d), G * d)]), 10)
    eta = R.eta(X, q0[None, :], ncat)[:, 0, :].astype(np.float64)
    p = np.exp(eta - eta.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    y = 1 + (rng.uniform(size=(n, 1)) > np.cumsum(p, axis=1)[:, :-1]).sum(1)
    if classes == "missing":
        y[y == 2] = 1
    elif classes == "reference":
        y[:] = ncat
    elif classes == "first":
        y[:] = 1
    return rng, X, y.astype(np.int32), q0


def points(rng, q0, C, sd=0.2):
    """C points: point 0 the data's own coefficients, the others within N(0, sd) of them, dyadic."""
    q = dyadic(q0[None, :] + rng.normal(0, sd, (C, q0.size)), 10)
    q[0] = q0
    return q


def lpgrad(ctx, X, y, ncat, q, prior=None):
    """lp (C,) and gradient (C, D) of one shard at the rows of q through the chain batches of a run at chains = C."""
    from stark_amd import engine
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}], ncat=ncat)
    try:
        if prior is not None:
            m.set_prior(alpha=prior[0], beta=prior[1])
        lp, g = m.log_density_grad_chains(q[None])
    finally:
        m.close()
    return lp[0], g[0]


# ---------------------------------------------------------------- 1. lp / gradient over the envelope
# (K, d, n, C): every K at its envelope corner; d at 1, 3, 4, 5, the tile edges 15 / 16 / 17, 31 / 32 / 33, 64, 100, 127,
# 128; n at the sub-tile (15, 16, 17), chunk-granule (63, 64, 65) and multi-chunk (257, 4097: 9 chunks) edges; C = 1, 3,
# 16 (one launch), 17 (16 + 1), 35 (16 + 16 + 3).
CASES = [
    (2, 1, 1, 1), (2, 16, 17, 16), (2, 100, 257, 3), (2, 128, 4097, 16), (2, 256, 65, 17), (2, 33, 63, 35), (2, 129, 64, 3),
    (3, 3, 15, 1), (3, 5, 16, 3), (3, 17, 64, 16), (3, 64, 257, 17), (3, 127, 65, 16), (3, 128, 4097, 16), (3, 100, 63, 35),
    (3, 31, 1, 3),
    (4, 4, 17, 3), (4, 15, 65, 16), (4, 33, 257, 16), (4, 80, 64, 17), (4, 32, 4097, 3),
    (5, 1, 63, 16), (5, 16, 16, 1), (5, 17, 257, 35), (5, 64, 4097, 16), (5, 33, 15, 3), (5, 48, 65, 16),
    (9, 3, 17, 16), (9, 15, 64, 3), (9, 16, 257, 17), (9, 31, 63, 16), (9, 32, 4097, 16), (9, 5, 1, 1),
    (17, 1, 16, 3), (17, 4, 65, 16), (17, 15, 257, 35), (17, 16, 4097, 16), (17, 5, 15, 1), (17, 16, 64, 17),
]
SPECIAL = [(3, 5, 65, 16, "missing"), (5, 17, 64, 3, "reference"), (9, 16, 63, 16, "first"), (17, 16, 257, 17, "missing"),
           (2, 100, 64, 16, "reference")]


@pytest.mark.parametrize("ncat,d,n,C", CASES)
def test_categorical_lpgrad(ctx, ncat, d, n, C):
    from stark_amd import engine
    rng, X, y, q0 = make_data(n, d, ncat)
    q = points(rng, q0, C)
    k = max(1, n // 3)
    m = engine.Model(ctx, FAM, [{"x": X[:k], "y": y[:k], "ncat": ncat}, {"x": X, "y": y, "ncat": ncat}])   # ncat from the data
    try:
        D = (ncat - 1) * (d + 1)
        assert m.ncat == ncat and m.D == [D, D] and m.P == [D + 1, D + 1] and m.n_rows == [k, n]
        assert engine.chain_batches(C, d, ncat=ncat) == [16] * (C // 16) + ([C % 16] if C % 16 else [])
        lp, g = m.log_density_grad_chains(np.stack([q, q]))
    finally:
        m.close()
    olp, og = R.ref_lpgrad(X, y, q, ncat)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g))
    wl, wg = check_bars(lp[1], g[1], olp, og, (ncat, d, n, C))
    olp0, og0 = R.ref_lpgrad(X[:k], y[:k], q, ncat)
    check_bars(lp[0], g[0], olp0, og0, (ncat, d, k, C, "shard 0"))
    print(f"MAXERR categorical[{ncat}-{d}-{n}-{C}] lp={wl:.3e} grad={wg:.3e}")


@pytest.mark.parametrize("ncat,d,n,C,classes", SPECIAL)
def test_categorical_lpgrad_degenerate_classes(ctx, ncat, d, n, C, classes):
    """A class that never occurs, every row the reference class, every row class 1."""
    rng, X, y, q0 = make_data(n, d, ncat, classes=classes)
    assert {"missing": 2 not in y, "reference": np.all(y == ncat), "first": np.all(y == 1)}[classes]
    q = points(rng, q0, C)
    lp, g = lpgrad(ctx, X, y, ncat, q)
    olp, og = R.ref_lpgrad(X, y, q, ncat)
    wl, wg = check_bars(lp, g, olp, og, (ncat, d, n, C, classes))
    print(f"MAXERR categorical[{classes}-{ncat}-{d}-{n}-{C}] lp={wl:.3e} grad={wg:.3e}")


# ---------------------------------------------------------------- 2. K = 2 is the logistic model
@pytest.mark.parametrize("d,n,C", [(5, 257, 3), (100, 4097, 16), (256, 65, 17)])
def test_categorical_two_classes_is_the_oracles_logistic(ctx, orc, d, n, C):
    rng, X, y, q0 = make_data(n, d, 2)
    q = points(rng, q0, C)
    lp, g = lpgrad(ctx, X, y, 2, q)
    om = orc.Model(orc.FAM_LOGREG, X=X, y=(y == 1).astype(np.int32))
    olp, og = map(np.array, zip(*[om.lpgrad(q[c]) for c in range(C)]))
    wl, wg = check_bars(lp, g, olp, og, ("logistic", d, n, C))
    print(f"MAXERR categorical[logistic-{d}-{n}-{C}] lp={wl:.3e} grad={wg:.3e}")


# ---------------------------------------------------------------- 3. relabelling
@pytest.mark.parametrize("ncat,d,n,C,g1,g2", [(3, 17, 65, 3, 1, 2), (5, 33, 257, 16, 2, 4), (9, 16, 64, 17, 1, 8), (17, 16, 63, 16, 5, 16)])
def test_categorical_relabelling(ctx, ncat, d, n, C, g1, g2):
    """Two non-reference classes swapped in y and their (alpha, beta) blocks in q: the same lp, the block-swapped
    gradient.  A mis-indexed class tile fails this."""
    rng, X, y, q0 = make_data(n, d, ncat)
    q = points(rng, q0, C)
    lp, g = lpgrad(ctx, X, y, ncat, q)
    q2, y2 = R.swap_classes(q, y, ncat, d, g1, g2)
    lp2, g2_ = lpgrad(ctx, X, y2, ncat, q2)
    gback, _ = R.swap_classes(g2_, y, ncat, d, g1, g2)
    check_bars(lp2, gback, lp.astype(np.longdouble), g.astype(np.longdouble), ("relabel", ncat, d, n, C))
    olp, og = R.ref_lpgrad(X, y, q, ncat)
    check_bars(lp2, gback, olp, og, ("relabel-ref", ncat, d, n, C))


# ---------------------------------------------------------------- 4. extreme eta
@pytest.mark.parametrize("scale", [30.0, 1e3, 1e150])
@pytest.mark.parametrize("ncat,d,n,C", [(3, 100, 257, 16), (5, 17, 300, 3), (17, 16, 65, 17), (2, 129, 64, 16)])
def test_categorical_lpgrad_extreme_eta(ctx, scale, ncat, d, n, C):
    """The first half of the points scaled by 30, 1e3, 1e150: every eta stays finite, so every point must be finite
    and within the bars (the maximum is subtracted before the exponentials)."""
    rng, X, y, q0 = make_data(n, d, ncat, seed=int(scale) % 1000 + n + ncat)
    q = points(rng, q0, C)
    q[: (C + 1) // 2] *= scale
    with np.errstate(over="ignore"):
        assert np.all(np.isfinite(R.eta(X, q, ncat).astype(np.float64)))
    lp, g = lpgrad(ctx, X, y, ncat, q)
    olp, og = R.ref_lpgrad(X, y, q, ncat)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(g)), (scale, lp)
    wl, wg = check_bars(lp, g, olp, og, (scale, ncat, d, n, C))
    print(f"MAXERR categorical[scale{scale:g}-{ncat}-{d}-{n}-{C}] lp={wl:.3e} grad={wg:.3e}")


@pytest.mark.parametrize("ncat,d,n,C", [(3, 100, 257, 16), (9, 16, 65, 3), (17, 5, 64, 17)])
def test_categorical_nan_and_inf(ctx, ncat, d, n, C):
    """A NaN coefficient gives a NaN lp at that point; an infinite one (eta = +-inf or NaN) never a finite lp and never
    +inf; the other points keep their bits."""
    rng, X, y, q0 = make_data(n, d, ncat)
    q = points(rng, q0, C)
    lp0, g0 = lpgrad(ctx, X, y, ncat, q)
    G = ncat - 1
    qn = q.copy()
    qn[0, 0] = np.nan                         # alpha_1
    qn[1, G + (G - 1) * d] = np.nan           # the last class's first beta
    qn[2, G - 1] = np.inf                     # alpha_G = +inf
    if C > 3:
        qn[3, 0] = -np.inf                    # alpha_1 = -inf: class 1 has probability 0
        qn[4, G] = 1e308                      # beta_1[0] x overflows for |x| > 1.8 never; 1e308 * 1.7 = inf
        qn[4, G + d - 1] = 1e308
    lp, g = lpgrad(ctx, X, y, ncat, qn)
    bad = ~np.isfinite(qn).all(1) | (np.abs(qn) > 1e300).any(1)
    assert np.all(np.isnan(lp[:2])) and not np.any(np.isfinite(g[:2]).all(1))
    assert not np.any(np.isfinite(lp[bad])) and not np.any(lp == np.inf), lp[bad]
    assert np.array_equal(lp[~bad], lp0[~bad]) and np.array_equal(g[~bad], g0[~bad])


# ---------------------------------------------------------------- 5. priors
@pytest.mark.parametrize("ncat,d,n,C", [(3, 100, 257, 16), (5, 17, 65, 3), (17, 16, 64, 17)])
def test_categorical_priors(ctx, ncat, d, n, C):
    rng, X, y, q0 = make_data(n, d, ncat)
    q = points(rng, q0, C)
    lp0, g0 = lpgrad(ctx, X, y, ncat, q)
    for flat in ((None, None), (0.0, 0.0), (float("inf"), 0.0)):
        lp, g = lpgrad(ctx, X, y, ncat, q, prior=flat)
        assert np.array_equal(lp, lp0) and np.array_equal(g, g0)
    for prior in ((2.5, 0.5), (0.0, 1.5), (10.0, 0.0)):
        lp, g = lpgrad(ctx, X, y, ncat, q, prior=prior)
        olp, og = R.ref_lpgrad(X, y, q, ncat, prior=prior)
        check_bars(lp, g, olp, og, ("prior", prior, ncat, d, n, C))
        assert not np.array_equal(lp, lp0)


# ---------------------------------------------------------------- 6. bits
@pytest.mark.parametrize("ncat,d,n", [(3, 100, 4097), (9, 32, 257), (17, 16, 65), (2, 256, 300)])
def test_categorical_bits_do_not_depend_on_the_launch(ctx, ncat, d, n):
    """Every chain of C = 35 (16 + 16 + 3) equals its value as a single launch of one chain, as one of 16 and in another
    column; shards of equal n grouped in one launch equal their separate launches; two runs are identical."""
    from stark_amd import engine
    rng, X, y, q0 = make_data(n, d, ncat)
    q = points(rng, q0, 35)
    y2 = np.roll(y, 7)
    three = [{"x": X, "y": y}, {"x": X, "y": y2}, {"x": X[: n // 2 + 1], "y": y[: n // 2 + 1]}]   # shards 0, 1 share a launch
    m = engine.Model(ctx, FAM, three, ncat=ncat)
    one = [engine.Model(ctx, FAM, [sh], ncat=ncat) for sh in three]
    try:
        lp, g = m.log_density_grad_chains(np.stack([q, q, q]))
        lpb, gb = m.log_density_grad_chains(np.stack([q, q, q]))
        assert np.array_equal(lp, lpb) and np.array_equal(g, gb)
        for s in range(3):
            lps, gs = one[s].log_density_grad_chains(q[None])
            assert np.array_equal(lps[0], lp[s]) and np.array_equal(gs[0], g[s]), s
        for c in (0, 5, 15, 16, 31, 32, 34):
            lp1, g1 = one[0].log_density_grad(0, q[c:c + 1])                 # alone: column 0 of a launch of 1
            assert np.array_equal(lp1[0], lp[0, c]) and np.array_equal(g1[0], g[0, c]), c
        lp16, g16 = one[0].log_density_grad(0, q[19:35])                     # other columns, another batch
        assert np.array_equal(lp16, lp[0, 19:35]) and np.array_equal(g16, g[0, 19:35])
        lps3, gs3 = m.log_density_grad_shards(np.stack([q[:3], q[:3], q[:3]]))
        assert np.array_equal(lps3, lp[:, :3]) and np.array_equal(gs3, g[:, :3])
    finally:
        m.close()
        for x in one:
            x.close()


# ---------------------------------------------------------------- 7. transitions: the oracle's logistic NUTS at K = 2
def _transition_rows(orc, d, C, n=400):
    rng, X, y, q0 = make_data(n, d, 2, seed=1000 * d + C)
    return X, y, orc.Model(orc.FAM_LOGREG, X=X, y=(y == 1).astype(np.int32))


@pytest.mark.parametrize("d,C,eps", [(13, 3, 0.05), (40, 17, 0.05)])
def test_categorical_transition_diag_e_matches_oracle(ctx, orc, d, C, eps):
    """test_sparse_transition_diag_e_matches_oracle's check and bars: a few fixed-step transitions at 3 and 17 (16 + 1)
    chains replayed by the oracle's logistic model on y' = 1[y = 1]."""
    from stark_amd import engine
    X, y, om = _transition_rows(orc, d, C)
    q0 = np.random.default_rng(5).normal(0, 0.1, (C, d + 1))
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}], ncat=2)
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
def test_categorical_transition_dense_e_matches_oracle(ctx, orc, C):
    """test_sparse_transition_dense_e_matches_oracle's check: one transition under a full D x D inverse metric, with
    the helpers and bars of test_gpu_dense_oracle.py."""
    from stark_amd import engine
    from test_gpu_dense_oracle import _check_rows, _general_metric
    d, n, eps = 13, 400, 0.2
    X, y, om = _transition_rows(orc, d, C, n)
    D = d + 1
    q0 = np.random.default_rng(5).normal(0, 0.1, (C, D))
    Minv = _general_metric(D, n)
    kw = dict(seed=41, inv_metric=Minv, factor=orc.cholesky(Minv), max_depth=6)
    want = [om.transition(q0[c], gid=c, iteration=6, eps=eps, **kw) for c in range(C)]
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}], ncat=2)
    try:
        q, lp, st = m.transition(0, q0, seed=41, iteration=6, eps=eps, inv_metric=Minv, max_depth=6)
    finally:
        m.close()
    _check_rows(orc, f"categorical_dense_e[{d}-{C}]", [((eps, c), q[c], lp[c], st[c], want[c][0], want[c][1], want[c][2])
                                                      for c in range(C)])


# ---------------------------------------------------------------- 8. sampling against an exact posterior
def grid_data():
    """n = 60, d = 1, K = 3: y from the softmax of alpha = (0.4, -0.3), beta = (0.9, -0.6)."""
    rng = np.random.default_rng(2030)
    x = rng.uniform(-1.7, 1.7, 60)
    eta = np.stack([0.4 + 0.9 * x, -0.3 - 0.6 * x, np.zeros(60)], axis=1)
    p = np.exp(eta)
    p /= p.sum(1, keepdims=True)
    y = 1 + (rng.uniform(size=(60, 1)) > np.cumsum(p, axis=1)[:, :-1]).sum(1)
    return x, y.astype(np.int32)


def grid_posterior_of(x, y, npts=49, half=8.0):
    """The flat-prior posterior of q = (alpha_1, alpha_2, beta_1, beta_2) on a npts^4 tensor grid over +-`half` Laplace
    standard deviations around the mode, from the reference's formulas in fp64: eta_1 depends on (alpha_1, beta_1)
    alone and eta_2 on (alpha_2, beta_2) alone.  Returns (means, variances, the same of the every-other-point subgrid,
    the mass on the grid's faces, the axes)."""
    X = x[:, None]
    q = np.zeros((1, 4))
    for _ in range(50):                                   # Newton on the reference's gradient, Hessian by its formula
        e = R.eta(X, q, 3)[:, 0, :].astype(np.float64)
        p = np.exp(e - e.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        z = np.stack([np.ones_like(x), x], axis=1)        # (n, 2)
        H = np.zeros((4, 4))
        for g1 in range(2):
            for g2 in range(2):
                w = p[:, g1] * ((g1 == g2) - p[:, g2])
                blk = -(z * w[:, None]).T @ z             # rows (alpha, beta) of class g1 against class g2
                for a in range(2):
                    for b in range(2):
                        H[2 * a + g1, 2 * b + g2] = blk[a, b]
        g = R.ref_lpgrad(X, y, q, 3)[1][0].astype(np.float64)
        step = np.linalg.solve(H, g)
        q = q - step[None, :]
        if np.abs(step).max() < 1e-13:
            break
    sd = np.sqrt(np.diag(np.linalg.inv(-H)))
    ax = [q[0, j] + sd[j] * np.linspace(-half, half, npts) for j in range(4)]
    E1 = np.exp(ax[0][:, None, None] + ax[2][None, :, None] * x[None, None, :])     # (a1, b1, n)
    E2 = np.exp(ax[1][:, None, None] + ax[3][None, :, None] * x[None, None, :])     # (a2, b2, n)
    lp = np.zeros((npts, npts, npts, npts))                                          # axes a1, b1, a2, b2
    for i in range(len(x)):
        lp -= np.log1p(E1[:, :, i][:, :, None, None] + E2[:, :, i][None, None, :, :])
    n1, n2 = float((y == 1).sum()), float((y == 2).sum())
    s1, s2 = float(x[y == 1].sum()), float(x[y == 2].sum())
    lp += (n1 * ax[0][:, None] + s1 * ax[2][None, :])[:, :, None, None] + (n2 * ax[1][:, None] + s2 * ax[3][None, :])[None, None, :, :]
    lp = np.ascontiguousarray(lp.transpose(0, 2, 1, 3))                              # axes in q's order: a1, a2, b1, b2
    qq = np.array([[ax[0][24], ax[1][24], ax[2][24], ax[3][24]], [ax[0][3], ax[1][40], ax[2][10], ax[3][47]]])
    olp = R.ref_lpgrad(X, y, qq, 3)[0].astype(np.float64)
    assert np.allclose([lp[24, 24, 24, 24], lp[3, 40, 10, 47]], olp, rtol=1e-12)     # the grid is the reference's density

    def moments(lp, axes):
        w = np.exp(lp - lp.max())
        w /= w.sum()
        face = sum(np.take(w, i, axis=k).sum() for k in range(4) for i in (0, -1))
        out = []
        for k, gax in enumerate(axes):
            wm = w.sum(tuple(i for i in range(4) if i != k))
            mu = (wm * gax).sum()
            out.append((mu, (wm * (gax - mu) ** 2).sum()))
        return np.array(out), face

    fine, face = moments(lp, ax)
    coarse, _ = moments(lp[::2, ::2, ::2, ::2], [a[::2] for a in ax])
    return fine, coarse, face, ax


@pytest.fixture(scope="module")
def grid_posterior():
    """Accepted only if the half-resolution subgrid agrees to 1e-6 relative on all eight moments and the mass on the
    faces is below 1e-8."""
    x, y = grid_data()
    fine, coarse, face, _ = grid_posterior_of(x, y)
    assert face < 1e-8, face
    assert np.all(np.abs(coarse - fine) <= 1e-6 * np.abs(fine)), (coarse, fine)
    return x, y, fine[:, 0].copy(), fine[:, 1].copy()


@pytest.mark.parametrize("metric", ["diag_e", "dense_e"])
@pytest.mark.parametrize("chains", [16, 3])
def test_categorical_sampling_exact(ctx, grid_posterior, chains, metric):
    """test_gamma_sampling_exact's criterion for the four coefficients: four-sigma bars from the run's own effective
    sizes, |mean - exact| <= 4 sd / sqrt(n_eff) and |var / exact - 1| <= 4 sqrt(2 / n_eff2), n_eff2 the n_eff of the
    centred squares; no divergences; the lp__ row is the reference density at the drawn point."""
    from stark_amd import diagnostics, engine
    x, y, mean, var = grid_posterior
    X = x[:, None].copy()
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}], ncat=3)
    try:
        res = m.sample(num_warmup=300, num_samples=1000, chains=chains, seed=3100 + chains, metric=metric)
    finally:
        m.close()
    assert res.info["divergent"] == 0 and res.info["errors"] == 0, res.info
    dr = res.draws[0]
    assert dr.shape == (5, chains * 1000) and np.isfinite(dr).all()
    for p in range(4):
        ch = dr[p].reshape(chains, 1000)
        ne = diagnostics.ess(ch)
        sq = (ch - mean[p]) ** 2
        ne2 = diagnostics.ess(sq)
        em = abs(ch.mean() - mean[p]) / (np.sqrt(var[p]) / np.sqrt(ne))
        ev = abs(sq.mean() / var[p] - 1.0) / np.sqrt(2.0 / ne2)
        print(f"chains={chains} {metric} par {p}: n_eff {ne:.0f} mean z {em:.2f}; n_eff2 {ne2:.0f} var z {ev:.2f}")
        assert em <= 4.0, (p, ch.mean(), mean[p], ne)
        assert ev <= 4.0, (p, sq.mean(), var[p], ne2)
    olp = R.ref_lpgrad(X, y, np.ascontiguousarray(dr[:4].T), 3)[0].astype(np.float64)
    assert np.all(np.abs(dr[4] - olp) <= RTOL * np.maximum(np.abs(olp), 1.0))


# ---------------------------------------------------------------- 9. determinism, checkpoints, metrics
@pytest.fixture(scope="module")
def small_rows():
    """1000 rows, d = 5, K = 3."""
    _rng, X, y, _q0 = make_data(1000, 5, 3, seed=79)
    return X, y


def test_categorical_deterministic_and_resumable(ctx, small_rows):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    X, y = small_rows
    cfg = dict(num_warmup=60, num_samples=60, chains=17, seed=31)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}], ncat=3)                                       # K = 3, d = 5: D = 12
    y4 = np.where(np.arange(1000) % 7 == 0, 4, y).astype(np.int32)
    m4 = engine.Model(ctx, FAM, [{"x": np.ascontiguousarray(X[:, :3]), "y": y4}], ncat=4)        # K = 4, d = 3: D = 12
    try:
        assert m.D == m4.D == [12]
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
        s3 = m4.sampler(**cfg)                      # the same D and the same sampler: the classes are part of the geometry
        before = s3.iterations().copy()
        with pytest.raises(StarkHipError) as e:
            s3.load_state(blob)
        assert e.value.code == -1
        assert np.array_equal(s3.iterations(), before)
        s3.close()
    finally:
        m.close()
        m4.close()


@pytest.mark.parametrize("metric", ["unit_e", "dense_e", "diag_e"])
@pytest.mark.parametrize("criterion", ["stan2.19", "stan2.23"])
def test_categorical_metrics_and_criteria_run(ctx, small_rows, metric, criterion):
    from stark_amd import engine
    X, y = small_rows
    m = engine.Model(ctx, FAM, [{"x": X[:500], "y": y[:500]}], ncat=3)
    try:
        res = m.sample(num_warmup=100, num_samples=50, chains=2, seed=8, metric=metric, nuts_criterion=criterion)
        assert res.info["errors"] == 0 and res.draws[0].shape == (13, 100) and np.isfinite(res.draws[0]).all()
        olp = R.ref_lpgrad(X[:500], y[:500], np.ascontiguousarray(res.draws[0][:12].T), 3)[0].astype(np.float64)
        assert np.all(np.abs(res.draws[0][12] - olp) <= RTOL * np.maximum(np.abs(olp), 1.0))
    finally:
        m.close()


# ---------------------------------------------------------------- 10. the driver
def test_categorical_through_the_driver(ctx):
    """The committed program on 4 partitions of 2,000 rows (no class separable), consensus combine: every coefficient
    within four posterior standard deviations of the generating value; the rows the driver's pars= selection returns."""
    from stark_amd import engine, frontend, stark
    from stark_amd.rdd import LocalContext
    rng = np.random.default_rng(11)
    d, ncat, n = 2, 3, 2000
    truth = np.array([0.5, -0.4, 0.8, -0.5, -0.6, 0.3])          # alpha_1, alpha_2, beta_1[0..2), beta_2[0..2)
    X = rng.uniform(-1.7, 1.7, (n, d))
    eta = R.eta(X, truth[None, :], ncat)[:, 0, :].astype(np.float64)
    p = np.exp(eta)
    p /= p.sum(1, keepdims=True)
    y = 1 + (rng.uniform(size=(n, 1)) > np.cumsum(p, axis=1)[:, :-1]).sum(1)
    rows = [tuple(float(v) for v in X[i]) + (int(y[i]),) for i in range(n)]

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": d, "ncat": ncat, "x": a[:, :d], "y": a[:, d].astype(np.int64)}

    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize(rows, 4), prep)
    st.setStanModel(file=os.path.join(os.path.dirname(frontend.__file__), "models", "categorical.stan"))
    assert st.family == FAM and st.priors == {}
    out = st.concensusWeight(chains=4, iter=600, separate_lp=True, permuted=False, seed=21)
    assert out.shape == (7, 4 * 300)                                # alpha[1..2], beta[1..4], lp__
    assert len(st.last_run.draws) == 4 and st.last_run.info["errors"] == 0
    ref, used = engine.consensus(st.last_run.draws, separate_lp=True)
    assert used.all() and np.array_equal(out, ref)
    est, sd = out[:6].mean(1), out[:6].std(1)
    print(f"categorical consensus {est} sd {sd}")
    assert np.all(np.abs(est - truth) <= 4 * sd), (est, truth, sd)
    assert np.all(sd < 0.3)
    # the driver's own pars= selection: the rows it hands back per key are alpha (S, G), beta (S, G d), lp__ last
    kw = dict(chains=2, iter=200, seed=22, permuted=False)
    full = st.concensusWeight(**kw)
    only_a, only_b = st.concensusWeight(pars=["alpha"], **kw), st.concensusWeight(pars=["beta"], **kw)
    assert full.shape == (7, 200) and only_a.shape == (3, 200) and only_b.shape == (5, 200)
    sel = [st._sample_partitions([prep(rows[:500])], pars=p_, **kw)[0] for p_ in (None, ["alpha"], ["beta"])]
    assert np.array_equal(sel[1], sel[0][[0, 1, 6]]) and np.array_equal(sel[2], sel[0][[2, 3, 4, 5, 6]])
    assert sel[1][:2].T.shape == (200, 2) and sel[2][:4].T.shape == (200, 4)         # alpha (S, G), beta (S, G d)
    for call in (lambda: st.concensusWeight(chains=2, iter=100, seed=1, weights="laplace"),
                 lambda: st.concensusWeight(chains=2, iter=100, seed=1, method="laplace"),
                 lambda: st.waic(out), lambda: st.loo(out), lambda: st.ppc(out), lambda: st.bootstrap(n=4)):
        with pytest.raises(ValueError, match=FAM):
            call()

    def prep_bad(part):
        dd = prep(part)
        dd["y"] = np.where(np.arange(len(part)) == 2, 4, dd["y"])
        return dd

    bad = stark.Stark(sc, sc.parallelize(rows, 4), prep_bad)
    bad.setStanModel(family=FAM)
    with pytest.raises(ValueError, match=r"y\[2\]"):
        bad.concensusWeight(chains=2, iter=100, seed=1)


# ---------------------------------------------------------------- 11. the refusals
def test_categorical_refusals(ctx, small_rows):
    """Each refusal is STK_E_ARG (or ValueError) with a message that names the family or the shape, before anything is
    launched; a valid sweep afterwards still runs."""
    import ctypes
    from stark_amd import _lib, engine
    from stark_amd._lib import StarkHipError
    lib = _lib.load()
    X, y = small_rows
    X, y = X[:100], y[:100]

    def refused(call, *words):
        with pytest.raises(StarkHipError) as e:
            call()
        assert e.value.code == -1 and all(w in str(e.value) for w in words), str(e.value)

    refused(lambda: engine.Model.synthetic(ctx, FAM, 1, 1000, 10), FAM)
    refused(lambda: engine.Model(ctx, FAM, [{"x_csr": ([0, 1, 1, 2], [0, 3], [1.0, 2.0]), "d": 4, "y": [1, 2, 1]}], ncat=2), FAM)
    # outside the envelope: K and d named, by value, before any launch
    refused(lambda: engine.Model(ctx, FAM, [{"x": np.zeros((4, 17)), "y": [1, 2, 17, 3]}], ncat=17), "K = 17", "d = 17")
    refused(lambda: engine.Model(ctx, FAM, [{"x": np.zeros((4, 5)), "y": [1, 2, 18, 3]}], ncat=18), "K = 18", "d = 5")
    refused(lambda: engine.Model(ctx, FAM, [{"x": np.zeros((4, 129)), "y": [1, 2, 3, 3]}], ncat=3), "K = 3", "d = 129")
    # a class outside [1, K]: the first one, with its shard and row
    for v in (0, 4, -1):
        yb = y.copy()
        yb[37] = v
        yb[60] = 9
        refused(lambda: engine.Model(ctx, FAM, [{"x": X, "y": y}, {"x": X, "y": yb}], ncat=3), "shard 1", "y_int[37]", f"= {v}")
    # a model without its classes: every density and sampler call says so; the classes are set once
    arr = (_lib.Shard * 1)()
    xx, yy = np.ascontiguousarray(X), np.ascontiguousarray(y, np.int32)
    arr[0] = _lib.Shard(100, 5, xx.ctypes.data, None, yy.ctypes.data, None)
    h = ctypes.c_void_p()
    assert lib.stk_model_create(ctx._h, _lib.STK_CATEGORICAL, arr, 1, ctypes.byref(h)) == 0
    try:
        q = np.zeros((2, 12))
        lp, g = np.zeros(2), np.zeros((2, 12))
        for rc in (lib.stk_log_density_grad(h, 0, q.ctypes.data, 2, lp.ctypes.data, g.ctypes.data),
                   lib.stk_log_density_grad_chains(h, q.ctypes.data, 2, lp.ctypes.data, g.ctypes.data),
                   lib.stk_log_density_grad_shards(h, q.ctypes.data, 2, lp.ctypes.data, g.ctypes.data)):
            assert rc == -1 and "stk_model_set_categories" in lib.stk_last_error().decode()
        cfg = engine.make_config(num_warmup=5, num_samples=5, chains=2, seed=1)
        sh = ctypes.c_void_p()
        assert lib.stk_sampler_create(h, ctypes.byref(cfg), ctypes.byref(sh)) == -1
        assert "stk_model_set_categories" in lib.stk_last_error().decode()
        assert lib.stk_model_set_categories(h, 1) == -1 and "K = 1" in lib.stk_last_error().decode()
        assert lib.stk_model_set_categories(h, 2) == -1 and "y_int" in lib.stk_last_error().decode()   # the data hold class 3
        assert lib.stk_model_set_categories(h, 3) == 0
        assert lib.stk_model_set_categories(h, 3) == -1 and "once" in lib.stk_last_error().decode()
        assert lib.stk_log_density_grad(h, 0, q.ctypes.data, 2, lp.ctypes.data, g.ctypes.data) == 0
    finally:
        lib.stk_model_destroy(h)
    m = engine.Model(ctx, FAM, [{"x": X, "y": y}], ncat=3)
    lg = engine.Model(ctx, "logistic", [{"x": X, "y": (y == 1).astype(np.int32)}])
    try:
        assert lib.stk_model_set_categories(lg._h, 3) == -1 and "logistic" in lib.stk_last_error().decode()
        s = m.sampler(num_warmup=10, num_samples=10, chains=2, seed=1)
        refused(lambda: s.set_allreduce(lambda ptr, count, stream: None), FAM)
        s.close()
        q = np.zeros((16, 12))
        for call in (lambda: m.hessian(0, q[0]), lambda: m.log_predictive(q), lambda: m.loo(q),
                     lambda: m.log_density(q, 0), lambda: m.log_density_grad_boot(q, 0, seed=1),
                     lambda: m.posterior_predict(q, seed=1)):
            refused(call, FAM)
        refused(lambda: engine.yrep_host(FAM, 1, 0, 0, 0, np.zeros((4, 2))), FAM)
        refused(lambda: m.log_density_grad_shards(np.zeros((1, 17, 12))), "17")
        lp, g = m.log_density_grad(0, q)                      # a valid sweep afterwards still runs
        olp, og = R.ref_lpgrad(X, y, q, 3)
        check_bars(lp, g, olp, og, "after the refusals")
        data = m.copy_data(0)                                 # y as given
        assert np.array_equal(data["y"], y) and np.array_equal(data["x"], X)
        assert m.fingerprint(0) == engine.shard_fingerprint(FAM, {"x": X, "y": y})
    finally:
        m.close()
        lg.close()
