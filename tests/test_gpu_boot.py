"""The weighted bootstrap sweep (stk_log_density_grad_boot, boot.hip), engine.bootstrap and Stark.bootstrap
against numpy restatements (tests/boot_ref.py).

The density of replicate b at q_b, with eta_i = alpha + x_i . beta and the twin's weights w_ib
(engine.boot_weights, checked against Philox in tests/test_host_boot.py):
    lp_b   = sum_i w_ib ll_i + prior + Jacobian         ll_i, prior, Jacobian: tests/test_gpu_logdens.py's
    grad_b = its gradient                               (linear: sum w ll = -wsum u - sum w z^2 / 2)
    wsum_b = sum_i w_ib
restated in np.longdouble.  Bars: lp within 1e-10 of sum w |ll| plus the absolute prior and Jacobian terms;
the gradient within 1e-10 of sum_i w_i |x_ij| |resid_i| per coordinate (plus the absolute prior term; for u the
absolute terms sum w z^2 + wsum + 1); the poisson wsum exact, the exponential one within 1e-12 relative.
Every case prints its largest error in units of its bar as a MAXERR line.
"""
import warnings

import numpy as np
import pytest

import boot_ref as br

pytestmark = pytest.mark.gpu

BAR = 1e-10
FAMILIES = br.FAMILIES
NS = (1, 15, 16, 17, 63, 64, 65, 257, 1030)
DS = (1, 3, 4, 5, 16, 17, 100, 128)
RS = (1, 15, 16, 17, 33)
KINDS = ("poisson", "exponential")
PRIOR = (2.5, 1.5)                   # sds of alpha and beta
L = np.longdouble


def points(truth, R, seed):
    return truth[None, :] + np.random.default_rng(seed).normal(0, 0.1, (R, truth.size))


def errors(lp, g, ws, ref, kind):
    """The largest errors of lp, grad and wsum in units of their bars against ref = br.weighted(...)."""
    rlp, rg, rws, slp, sg = ref
    with np.errstate(invalid="ignore", divide="ignore"):      # a scale of 0 (every weight 0): exact
        el = np.abs(lp.astype(L) - rlp) / (BAR * slp)
        eg = np.abs(g.astype(L) - rg) / (BAR * sg)
    e_lp = float(np.where(slp > 0, el, np.where(lp == rlp, 0, np.inf)).max())
    e_g = float(np.where(sg > 0, eg, np.where(g == rg, 0, np.inf)).max())
    if kind == "poisson":
        e_ws = 0.0 if np.array_equal(ws, rws.astype(np.float64)) else np.inf
    else:
        e_ws = float((np.abs(ws.astype(L) - rws) / (1e-12 * rws)).max())      # Exp(1) weights are > 0
    return e_lp, e_g, e_ws


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("family", FAMILIES)
def test_density_gradient_and_wsum_match_the_restatement(ctx, family, d):
    """Every n of NS (one model each, the first n rows; row 515 is all zero) x both kinds x priors off and on
    at R = 33 against the restatement, and every smaller R of RS against the first R rows of that, bit for bit."""
    from stark_amd import engine
    X, y, truth = br.make_data(family, max(NS), d, 7000 + 10 * d + FAMILIES.index(family))
    Q = points(truth, max(RS), d)
    worst = {"lp": 0.0, "grad": 0.0, "wsum": 0.0}
    for n in NS:
        m = engine.Model(ctx, family, [{"x": np.ascontiguousarray(X[:n]), "y": np.ascontiguousarray(y[:n])}])
        try:
            for prior in (None, PRIOR):
                m.set_prior(*(prior or (None, None)))
                for kind in KINDS:
                    W = engine.boot_weights(11, 0, 0, n, 0, max(RS), kind)
                    ref = br.weighted(family, X[:n], y[:n], Q, W, prior)
                    lp, g, ws = m.log_density_grad_boot(Q, 0, seed=11, kind=kind)
                    assert lp.shape == (33,) and g.shape == (33, truth.size) and ws.shape == (33,)
                    assert np.isfinite(lp).all() and np.isfinite(g).all()
                    e_lp, e_g, e_ws = errors(lp, g, ws, ref, kind)
                    for k, v in (("lp", e_lp), ("grad", e_g), ("wsum", e_ws)):
                        worst[k] = max(worst[k], v)
                    assert e_lp <= 1.0 and e_g <= 1.0 and e_ws <= 1.0, (family, n, d, prior, kind, e_lp, e_g, e_ws)
                    for R in RS[:-1]:
                        lp2, g2, ws2 = m.log_density_grad_boot(Q[:R], 0, seed=11, kind=kind)
                        assert np.array_equal(lp2, lp[:R]) and np.array_equal(g2, g[:R]) and np.array_equal(ws2, ws[:R])
        finally:
            m.close()
    print(f"MAXERR boot {family} d={d}: lp {worst['lp']:.3g} grad {worst['grad']:.3g} wsum {worst['wsum']:.3g} bars")


def test_device_weights_are_the_twins(ctx):
    """wsum of the n-row prefix shard minus wsum of the (n - 1)-row prefix, n = 1 .. 80, 16 poisson replicates:
    the twin's w_{n-1,b} exactly -- across the 16- and 64-row boundaries and the padding select."""
    from stark_amd import engine
    X, y, truth = br.make_data("logistic", 80, 3, 1)
    Q = points(truth, 16, 2)
    twin = engine.boot_weights(77, 5, 0, 80, 16, 16, "poisson")
    prev = np.zeros(16)
    for n in range(1, 81):
        m = engine.Model(ctx, "logistic", [{"x": np.ascontiguousarray(X[:n]), "y": np.ascontiguousarray(y[:n])}])
        try:
            _, _, ws = m.log_density_grad_boot(Q, 0, rep0=16, seed=77, streams=[5], kind="poisson")
        finally:
            m.close()
        assert np.array_equal(ws - prev, twin[n - 1]), (n, ws - prev, twin[n - 1])
        prev = ws
    print("MAXERR boot device weights: 0 bars")


@pytest.mark.parametrize("family", FAMILIES)
def test_bit_level_contracts(ctx, family):
    from stark_amd import engine
    d = 17
    X, y, truth = br.make_data(family, 257 + 65 + 1030, d, 31)
    cuts = (0, 257, 322, 1352)
    shards = [{"x": np.ascontiguousarray(X[a:b]), "y": np.ascontiguousarray(y[a:b])} for a, b in zip(cuts, cuts[1:])]
    Q = points(truth, 33, 4)
    m = engine.Model(ctx, family, shards)
    try:
        for kind in KINDS:
            lp, g, ws = m.log_density_grad_boot(Q, None, seed=9, kind=kind)
            assert lp.shape == (3, 33) and g.shape == (3, 33, truth.size) and ws.shape == (3, 33)
            for s in range(3):       # the grouped launch is the single-shard calls; NULL streams the local index
                one = m.log_density_grad_boot(Q, s, seed=9, kind=kind, streams=[s])
                assert all(np.array_equal(a, b[s]) for a, b in zip(one, (lp, g, ws))), (kind, s)
            again = m.log_density_grad_boot(Q, None, seed=9, kind=kind, streams=[0, 1, 2])
            assert all(np.array_equal(a, b) for a, b in zip(again, (lp, g, ws)))
            # replicate 16 alone, among other companions, and R = 17 as 16 + 1
            alone = m.log_density_grad_boot(Q[16:17], 1, rep0=16, seed=9, kind=kind)
            assert all(np.array_equal(a[0], b[1][16]) for a, b in zip(alone, (lp, g, ws)))
            Q2 = points(truth, 33, 5)
            Q2[16] = Q[16]
            other = m.log_density_grad_boot(Q2, 1, seed=9, kind=kind)
            assert all(np.array_equal(a[16], b[1][16]) for a, b in zip(other, (lp, g, ws)))
            assert not np.array_equal(other[0][15], lp[1][15])
            r17 = m.log_density_grad_boot(Q[:17], 1, seed=9, kind=kind)
            r16 = m.log_density_grad_boot(Q[:16], 1, seed=9, kind=kind)
            for a, b, c in zip(r17, r16, alone):
                assert np.array_equal(a[:16], b) and np.array_equal(a[16], c[0])
            # streams change the weights
            moved = m.log_density_grad_boot(Q, None, seed=9, kind=kind, streams=[0, 7, 2])
            assert np.array_equal(moved[0][0], lp[0]) and np.array_equal(moved[0][2], lp[2])
            assert not np.array_equal(moved[2][1], ws[1]) and not np.array_equal(moved[0][1], lp[1])
            # a NaN point: its own lp is not finite, nobody else moves
            Q3 = Q.copy()
            Q3[20, 2] = np.nan
            lp3, g3, ws3 = m.log_density_grad_boot(Q3, None, seed=9, kind=kind)
            keep = np.arange(33) != 20
            assert not np.isfinite(lp3[:, 20]).any()
            assert np.array_equal(lp3[:, keep], lp[:, keep]) and np.array_equal(g3[:, keep], g[:, keep])
            assert np.array_equal(ws3, ws)
    finally:
        m.close()
    print(f"MAXERR boot contracts {family}: 0 bars")


def test_refusals_name_the_value(ctx):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    m = engine.Model(ctx, "schools", [{"y": [28.0, 8.0, -3.0], "sigma": [15.0, 10.0, 16.0]}])
    try:
        with pytest.raises(StarkHipError, match="schools"):
            m.log_density_grad_boot(np.zeros((1, m.D[0])), 0)
    finally:
        m.close()
    rng = np.random.default_rng(0)
    m = engine.Model(ctx, "logistic", [{"x": rng.normal(size=(20, 129)), "y": rng.integers(0, 2, 20)}])
    try:
        with pytest.raises(StarkHipError, match="d = 129"):
            m.log_density_grad_boot(np.zeros((1, 130)), 0)
    finally:
        m.close()
    m = engine.Model(ctx, "logistic", [{"x": rng.normal(size=(20, 3)), "y": rng.integers(0, 2, 20)}])
    try:
        q = np.zeros((1, 4))
        with pytest.raises(StarkHipError, match="kind = 2"):
            m.log_density_grad_boot(q, 0, kind=2)
        with pytest.raises(StarkHipError, match="R = 0"):
            m.log_density_grad_boot(np.zeros((0, 4)), 0)
        with pytest.raises(StarkHipError, match="rep0 = 8"):
            m.log_density_grad_boot(q, 0, rep0=8)
        with pytest.raises(StarkHipError, match="4097"):
            m.log_density_grad_boot(np.zeros((17, 4)), 0, rep0=4080)
        with pytest.raises(StarkHipError, match=f"stream = {2 ** 20}"):
            m.log_density_grad_boot(q, 0, streams=[2 ** 20])
        lp, _, _ = m.log_density_grad_boot(np.zeros((16, 4)), 0, rep0=4080)       # the last tile is fine
        assert np.isfinite(lp).all()
    finally:
        m.close()


@pytest.mark.parametrize("n,d", ((1030, 16), (257, 3)))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_bootstrap_end_to_end(ctx, family, kind, n, d):
    """B = 20 (a full tile and a tail), one shard and the same rows split over two: every replicate converges
    within 1e-7 sd of the host Newton solve on the twin's weights."""
    from stark_amd import engine
    X, y, truth = br.make_data(family, n, d, 900 + n + d)
    cut = n // 3
    for cuts in ((0, n), (0, cut, n)):
        shards = [{"x": np.ascontiguousarray(X[a:b]), "y": np.ascontiguousarray(y[a:b])} for a, b in zip(cuts, cuts[1:])]
        m = engine.Model(ctx, family, shards)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                res = engine.bootstrap(m, 20, kind=kind, seed=13)
        finally:
            m.close()
        assert res["converged"].all() and res["estimates"].shape == (20, truth.size)
        ref = br.newton_replicates(family, shards, range(len(shards)), 20, kind, 13, res["mode"])
        sd = np.sqrt(np.diag(res["cov"]))
        err = float((np.abs(res["estimates"] - ref) / sd).max())
        print(f"MAXERR bootstrap {family} {kind} n={n} d={d} shards={len(shards)}: {err / 1e-7:.3g} bars, "
              f"iterations {res['iterations'].min()}..{res['iterations'].max()}")
        assert err <= 1e-7


def test_replicate_variance_matches_the_laplace_variance(ctx):
    """Logistic, n = 4100, d = 5, B = 256 exponential replicates at a fixed seed: every parameter's replicate
    variance over its Laplace variance lies in [0.5, 1.5] -- the variance estimator's relative sd is
    sqrt(2 / 255) = 0.09, so five of them.  (The host Newton solve on the twin's weights gives 0.86 .. 1.28
    at this seed.)"""
    from stark_amd import engine
    X, y, truth = br.make_data("logistic", 4100, 5, 44)
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        res = engine.bootstrap(m, 256, kind="exponential", seed=2024)
    finally:
        m.close()
    assert res["converged"].all()
    ratio = res["estimates"].var(axis=0, ddof=1) / np.diag(res["cov"])
    print(f"MAXERR bootstrap variance ratio: {ratio.min():.3f} .. {ratio.max():.3f} "
          f"({max(abs(ratio - 1).max() / 0.5, 0):.3g} bars)")
    assert np.all((ratio >= 0.5) & (ratio <= 1.5)), ratio


def _driver(rows, parts, K=5, family="logistic"):
    import os
    from conftest import ROOT
    from stark_amd import stark
    from stark_amd.rdd import LocalContext, LocalRDD

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": K, "x": a[:, :K], "y": a[:, K].astype(np.int64)}

    cuts = np.concatenate([[0], np.cumsum(parts)])
    rdd = LocalRDD([rows[cuts[i]:cuts[i + 1]] for i in range(len(parts))])
    st = stark.Stark(LocalContext(), rdd, prep)
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", f"{family}.stan"))
    return st


def test_driver_bootstrap(ctx):
    """Stark.bootstrap over two logistic partitions, n = 32 replicates: P x 32, pars= selects rows, and the
    matrix is engine.bootstrap over the two shards after the constraining transform (logistic: none)."""
    from stark_amd import engine
    parts, d = (150, 107), 5
    X, y, _ = br.make_data("logistic", sum(parts), d, 77)
    rows = [tuple(X[i]) + (int(y[i]),) for i in range(sum(parts))]
    st = _driver(rows, parts)
    out = st.bootstrap(n=32, weights="poisson", seed=5)
    assert out.shape == (d + 2, 32) and np.isfinite(out).all()
    assert st.bootstrap_diagnostics["converged"].all() and st.bootstrap_diagnostics["wsum"].shape == (32,)
    shards = [{"x": np.ascontiguousarray(X[:150]), "y": y[:150]}, {"x": np.ascontiguousarray(X[150:]), "y": y[150:]}]
    m = engine.Model(ctx, "logistic", shards)
    try:
        res = engine.bootstrap(m, 32, kind="poisson", seed=5)
    finally:
        m.close()
    assert np.array_equal(out[:-1], res["estimates"].T) and np.array_equal(out[-1], res["lp"])
    sel = st.bootstrap(n=32, weights="poisson", seed=5, pars=["alpha"])
    assert sel.shape == (2, 32) and np.array_equal(sel, out[[0, -1]])
    with pytest.raises(ValueError, match="weights"):
        st.bootstrap(n=4, weights="gamma")


def test_driver_bootstrap_refusals():
    """8 schools and K = 129 raise ValueError before a model is built (no device is touched: no ctx)."""
    import os
    from conftest import ROOT
    from stark_amd import stark
    from stark_amd.rdd import LocalContext, LocalRDD
    st = stark.Stark(LocalContext(), LocalRDD([[(28.0, 15.0), (8.0, 10.0)]]),
                     lambda part: {"J": len(part), "y": [r[0] for r in part], "sigma": [r[1] for r in part]})
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "schools.stan"))
    with pytest.raises(ValueError, match="schools"):
        st.bootstrap(n=4)
    rows = [tuple(np.zeros(129)) + (i % 2,) for i in range(8)]
    st = _driver(rows, (4, 4), K=129)
    with pytest.raises(ValueError, match="K = 129"):
        st.bootstrap(n=4)
