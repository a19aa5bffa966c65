"""Pin the CPU oracle before trusting it (CPU only).

* Philox4x32-10 against Random123's published known-answer vectors.
* The numpy combine restatement against fixtures produced by the REFERENCE's own
  consensus_avg / driver solve (tests/golden/make_golden.py imports stark/stark.py).
* Densities against central finite differences; the NUTS twin against exact posterior
  moments (8 schools by quadrature, flat-prior linear regression in closed form).
"""
import numpy as np
import pytest

from stark_amd.stark import _extract_to_matrix


KAT = [  # Random123 kat_vectors, philox4x32_10
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_kat(orc, ctr, key, want):
    assert tuple(orc.philox(ctr, key)) == want


@pytest.mark.parametrize("P", [11, 53, 102])
def test_combine_restatement_matches_reference(golden, orc, P):
    g = golden("combine_ref.npz")
    f1, f2 = g[f"P{P}_f1"], g[f"P{P}_f2"]
    red = orc.consensus_avg_ref(f1, f2)
    np.testing.assert_allclose(red[0], g[f"P{P}_sumW"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(red[1], g[f"P{P}_sumWtheta"], rtol=1e-10, atol=1e-12 * np.abs(red[1]).max())
    final = orc.consensus_combine_ref([f1, f2])
    np.testing.assert_allclose(final, g[f"P{P}_final"], rtol=1e-9, atol=1e-12 * np.abs(final).max())


def test_combine_lp_row_leak(orc):
    """The reference's joint combine (lp__ inside inv(cov), stark/stark.py:49-56) on Gaussian
    shards whose lp__ rows sit 300 lp-sds apart: the parameter means move by several posterior
    sds; combining the parameter rows alone (the separate_lp block) does not."""
    rng = np.random.default_rng(11)
    P, n, S = 21, 1000, 8
    A = rng.normal(size=(P, P)) / np.sqrt(P)
    L = np.linalg.cholesky(8 * (A @ A.T + 0.5 * np.eye(P)))
    mus = [L @ rng.normal(size=P) for _ in range(S)]
    draws = []
    for s in range(S):
        w = rng.normal(size=(P, n))
        lp = -0.5 * (w ** 2).sum(0) + 300 * np.sqrt(P / 2) * rng.normal()
        draws.append(np.vstack([mus[s][:, None] + L @ w, lp]))
    full = np.mean(mus, axis=0)
    z2 = lambda c: float((((c.mean(1) - full) / c.std(1)) ** 2).mean())
    assert z2(orc.consensus_combine_ref(draws)[:-1]) > 5.0
    assert z2(orc.consensus_combine_ref([d[:-1] for d in draws])) < 0.2


def test_combine_nan_guard_reference(golden, orc):
    g = golden("combine_ref.npz")
    out = orc.consensus_avg_ref(g["nan_f1"], g["nan_f2"])
    np.testing.assert_array_equal(out, g["nan_out"])
    np.testing.assert_array_equal(out, g["nan_f2"])


def test_concat_reference(golden):
    from stark_amd.stark import concatenate_samples
    g = golden("concat_ref.npz")
    np.testing.assert_array_equal(concatenate_samples(g["a"], g["b"]), g["out"])


def test_extract_to_matrix_reference(golden):
    """stark/stark.py:49-56 contract (key order, (S,1) reshape, transpose) vs the reference's
    own closure output on the same fake fit."""
    import collections
    g = golden("driver_ref.npz")
    # rebuild partition 0's fake fit at iter=600 from the fixture and compare layouts
    od = collections.OrderedDict((k, g[f"w600_part0_{k}"]) for k in ("mu", "tau", "eta", "theta", "lp__"))
    m = _extract_to_matrix(od)
    assert m.shape == (11, 300)
    np.testing.assert_array_equal(m[0], od["mu"])
    np.testing.assert_array_equal(m[2:6], od["eta"].T)
    np.testing.assert_array_equal(m[-1], od["lp__"])
    assert g["part0"].shape == (11, 1000)


@pytest.mark.parametrize("family", ["schools", "logistic", "linear"])
def test_oracle_density_fd(orc, family):
    rng = np.random.default_rng(3)
    if family == "schools":
        m = orc.Model(orc.FAM_SCHOOLS, y=orc.SCHOOLS_Y, sigma=orc.SCHOOLS_SIGMA)
    else:
        X = rng.uniform(-1.7, 1.7, (300, 5))
        beta = rng.normal(0, 0.5, 5)
        if family == "logistic":
            y = (rng.uniform(size=300) < 1 / (1 + np.exp(-X @ beta))).astype(np.int32)
            m = orc.Model(orc.FAM_LOGREG, X=X, y=y)
        else:
            y = X @ beta + rng.normal(size=300)
            m = orc.Model(orc.FAM_LINREG, X=X, y=y)
    q = rng.normal(0, 0.3, m.D)
    lp, g = m.lpgrad(q)
    h = 1e-6
    fd = np.array([(m.lpgrad(q + h * e)[0] - m.lpgrad(q - h * e)[0]) / (2 * h) for e in np.eye(m.D)])
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-6 * max(1.0, np.abs(g).max()))


def _ld_schools(y, sigma, q):
    """stark_amd/models/schools.stan in long double: non-centred, tau = exp(u) with Jacobian + u.
    Returns (lp, grad, sum |terms| of lp, sum |terms| of every gradient component)."""
    L = np.longdouble
    y, sigma, q = y.astype(L), sigma.astype(L), q.astype(L)
    mu, u, eta = q[0], q[1], q[2:]
    tau = np.exp(u)
    z = (y - (mu + tau * eta)) / sigma
    r = z / sigma
    lp = (-eta * eta / 2 - z * z / 2).sum() + u
    g = np.concatenate([[r.sum(), tau * (r * eta).sum() + 1], -eta + tau * r])
    alp = (eta * eta / 2).sum() + (z * z / 2).sum() + abs(u)
    ag = np.concatenate([[np.abs(r).sum(), (tau * np.abs(r * eta)).sum() + 1], np.abs(eta) + tau * np.abs(r)])
    return lp, g, alp, ag


def _ld_logistic(X, y, q):
    """stark_amd/models/logistic.stan in long double with Stan 2.19's bernoulli_logit cut-offs:
    with t = (2y - 1) eta, the term is -exp(-t) above 20, t below -20, -log1p(exp(-t)) between."""
    L = np.longdouble
    X, q = X.astype(L), q.astype(L)
    sgn = (2 * y - 1).astype(L)
    t = sgn * (q[0] + X @ q[1:])
    e = np.exp(-t)
    lt = np.where(t > 20, -e, np.where(t < -20, t, -np.log1p(e)))
    de = sgn * np.where(t > 20, e, np.where(t < -20, L(1), e / (e + 1)))
    lp = lt.sum()
    g = np.concatenate([[de.sum()], X.T @ de])
    ag = np.concatenate([[np.abs(de).sum()], np.abs(X).T @ np.abs(de)])
    return lp, g, np.abs(lt).sum(), ag


def _ld_linear(X, y, q):
    """stark_amd/models/linear.stan in long double: sigma = exp(u), lp = -ss/2 - N u + u."""
    L = np.longdouble
    X, y, q = X.astype(L), y.astype(L), q.astype(L)
    n, d = X.shape
    u = q[d + 1]
    inv_s = np.exp(-u)
    z = (y - (q[0] + X @ q[1:d + 1])) * inv_s
    ss = (z * z).sum()
    dm = z * inv_s
    lp = -ss / 2 - n * u + u
    g = np.concatenate([[dm.sum()], X.T @ dm, [-L(n) + ss + 1]])
    ag = np.concatenate([[np.abs(dm).sum()], np.abs(X).T @ np.abs(dm), [L(n) + ss + 1]])
    return lp, g, ss / 2 + n * abs(u) + abs(u), ag


@pytest.mark.parametrize("family", ["schools", "logistic", "linear"])
def test_oracle_density_matches_extended_precision(orc, family):
    """The oracle's three densities and gradients against their restatement in long double (64-bit
    mantissa).  The bar is derived: a sequential fp64 sum of n terms errs by at most
    n 2^-53 sum |term_i| to first order, and every term carries a few roundings of its own (the
    d-term dot product of eta, exp, log1p, the products): |oracle - ld| <= 4 (n + d) 2^-53 sum
    |terms|, the sums of absolute terms taken in long double per lp and per gradient component.
    On the same inputs that bound is to lie below 1e-11 max(|value|, 1), so the GPU tests' 1e-10
    bar against the oracle has a factor 10 of room above the oracle's own error.

    A worst-case bound relative to the value says something only where the sum does not cancel
    (sum |terms| / |value| is what it scales with; the GPU tests floor their gradient bar for
    the same reason), so the regression points are chosen away from the mode: see the comments
    at the inputs.

    Measured (x86-64): the oracle's error is at most 0.10 of the bound (schools) and 3.0e-3 of it
    (regressions), i.e. at most 3.6e-4 of 1e-11 max(|value|, 1) everywhere.  The bound is at most
    0.091 of 1e-11 max(|value|, 1) for every lp, 0.022 for the schools gradient, 0.10 for the
    logistic gradient and 0.72 for the linear one."""
    if np.finfo(np.longdouble).eps >= 2.0 ** -53:
        pytest.skip("np.longdouble is no wider than fp64 on this platform")
    rng = np.random.default_rng(8)
    cases = []          # (name, oracle model, n + d, long-double restatement, q)
    if family == "schools":
        for J, y, sigma in ((8, orc.SCHOOLS_Y, orc.SCHOOLS_SIGMA), (70, rng.normal(0, 10, 70), rng.uniform(5, 20, 70))):
            om = orc.Model(orc.FAM_SCHOOLS, y=y, sigma=sigma)
            for k in range(3):
                cases.append((f"J={J} q{k}", om, J, lambda q, y=y, sigma=sigma: _ld_schools(y, sigma, q),
                              rng.normal(0, 1, om.D)))
    else:
        # linear: every coefficient 0.3 away from the generating one, so that no gradient component is
        # the cancelling sum it is near the mode (there sum |terms| exceeds |value| without limit)
        n, d = 2000, 40
        X = rng.uniform(-1.7, 1.7, (n, d))
        beta = rng.normal(0, 1 / np.sqrt(d), d)
        away = beta + 0.3 * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
        if family == "logistic":
            # The residual y - p saturates, so over centred columns no point keeps all 41 gradient
            # components from cancelling (sum |x_ij de_i| stays >= 29 |sum x_ij de_i| for some j at
            # n = 2000, d = 40, and the worst-case bound, linear in n, then exceeds 1e-11 |g_j|).
            # Non-negative columns and an intercept that is too high make every component a sum of
            # mostly one sign: the bound is about the arithmetic, not about cancellation.
            X = np.abs(X)
            eta = X @ beta
            eta[: n // 50] *= 80.0
            y = (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.int32)
            om = orc.Model(orc.FAM_LOGREG, X=X, y=y)
            # the first point keeps every row between the cut-offs; the second puts the y = 1 rows
            # above +20 and the y = 0 rows below -20
            qs = [("alpha+3", np.concatenate([[3.0], beta])), ("alpha+100, 40 beta", np.concatenate([[100.0], 40 * beta]))]
            t = (2 * y - 1) * (3.0 + X @ beta)
            assert np.all(np.abs(t) < 20)
            t = (2 * y - 1) * (100.0 + X @ (40 * beta))
            assert (t > 20).sum() > 100 and (t < -20).sum() > 100
            cases += [(name, om, n + d, lambda q: _ld_logistic(X, y, q), q) for name, q in qs]
        else:
            y = 0.3 + X @ beta + rng.normal(size=n)
            om = orc.Model(orc.FAM_LINREG, X=X, y=y)
            for u in (-6.0, 0.0, 6.0):
                cases.append((f"log sigma={u}", om, n + d, lambda q: _ld_linear(X, y, q),
                              np.concatenate([[0.8], away, [u]])))
    res = []
    for name, om, nd, ld, q in cases:
        lp, g = om.lpgrad(q)
        rlp, rg, alp, ag = ld(q)
        got = np.concatenate([[lp], g]).astype(np.longdouble)
        ref = np.concatenate([[rlp], rg])
        bound = 4 * nd * np.longdouble(2.0) ** -53 * np.concatenate([[alp], ag])
        room = 1e-11 * np.maximum(np.abs(ref), 1)
        res.append((name, np.abs(got - ref), bound, room))
        print(f"{family} {name}: max err/bound = {float((res[-1][1] / bound).max()):.3g}, "
              f"err/(1e-11 max(|v|, 1)) = {float((res[-1][1] / room).max()):.3g}, "
              f"bound/(1e-11 max(|v|, 1)) = lp {float(bound[0] / room[0]):.3g}, grad {float((bound[1:] / room[1:]).max()):.3g}")
    for name, err, bound, room in res:
        assert np.all(err <= bound), (name, float((err / bound).max()))
    for name, err, bound, room in res:
        assert np.all(bound < room), (name, float((bound / room).max()), int(np.argmax(bound / room)))


def test_oracle_generator_shapes(orc):
    X = orc.gen_x(7, 0, 50, 9)
    assert X.shape == (50, 9) and np.all(np.abs(X) < np.sqrt(3))
    assert abs(X.var() - 1.0) < 0.2
    b = orc.gen_beta(7, 9)
    y, margin = orc.gen_y_logistic(7, 0, X, 0.0, b)
    assert set(np.unique(y)) <= {0, 1} and np.all(margin >= 0)
    # sharding invariance: rows carry their global index
    np.testing.assert_array_equal(orc.gen_x(7, 20, 10, 9), X[20:30])


def test_oracle_nuts_schools_exact_moments(orc):
    m = orc.Model(orc.FAM_SCHOOLS, y=orc.SCHOOLS_Y, sigma=orc.SCHOOLS_SIGMA)
    em, ev = orc.schools_exact_moments(orc.SCHOOLS_Y, orc.SCHOOLS_SIGMA)
    runs = [m.run_chain(num_warmup=1000, num_samples=5000, seed=11, gid=c) for c in range(8)]
    Q = np.concatenate([r["q"][1000:] for r in runs])
    from stark_amd.diagnostics import ess
    for k in range(m.D):
        x = np.stack([r["q"][1000:, k] for r in runs])
        mcse = x.std() / np.sqrt(ess(x))
        assert abs(Q[:, k].mean() - em[k]) < 5 * mcse + 1e-3, (k, Q[:, k].mean(), em[k], mcse)
    # variances of eta within 10%
    np.testing.assert_allclose(Q[:, 2:].var(0), ev[2:], rtol=0.1)


def test_oracle_nuts_linreg_closed_form(orc):
    rng = np.random.default_rng(5)
    X = rng.uniform(-1.7, 1.7, (200, 3))
    y = 0.5 + X @ np.array([1.0, -0.5, 0.25]) + rng.normal(size=200)
    m = orc.Model(orc.FAM_LINREG, X=X, y=y)
    mean, cov = orc.linreg_exact_moments(X, y)
    runs = [m.run_chain(num_warmup=500, num_samples=2000, seed=3, gid=c) for c in range(4)]
    Q = np.concatenate([r["q"][500:, :4] for r in runs])
    sd = np.sqrt(np.diag(cov))
    assert np.all(np.abs(Q.mean(0) - mean) < 0.1 * sd + 4 * sd / np.sqrt(len(Q) / 3))
    np.testing.assert_allclose(Q.std(0), sd, rtol=0.08)


def test_oracle_transition_deterministic(orc):
    m = orc.Model(orc.FAM_SCHOOLS, y=orc.SCHOOLS_Y, sigma=orc.SCHOOLS_SIGMA)
    q0 = np.linspace(-0.5, 0.5, m.D)
    a = m.transition(q0, seed=5, gid=3, iteration=7, eps=0.3)
    b = m.transition(q0, seed=5, gid=3, iteration=7, eps=0.3)
    np.testing.assert_array_equal(a[0], b[0])
    assert a[2][3] == 2 ** a[2][2] - 1 or a[2][4] == 1 or a[2][2] >= 0


def test_residual_v3_emulation_accuracy():
    """The design of k_sweepe's logistic residual v3 (tables, polynomial degrees, Stan's +-20
    cutoffs by clamping, one Newton step on a 2^-24 reciprocal seed), emulated in numpy by
    tools/residual_v3_accuracy.py, against Stan's bernoulli_logit term in long double: lt within
    4e-15 absolute and dv within 1e-15 relative away from the cutoff bands, exactly Stan's (t, 1)
    below -20, NaN kept.  (The GPU kernel is checked against the oracle in test_gpu_kernels.py.)"""
    import numpy as np
    from tools import residual_v3_accuracy as R
    t = np.concatenate([np.random.default_rng(3).uniform(-25, 25, 100_000), np.linspace(-21, -19, 2001)])
    lt, dv = R.resid3(t)
    lr, dr = R.stan(t)
    inner = np.abs(t) < 20
    assert np.abs(lt - lr.astype(np.float64))[inner].max() < 4e-15
    assert (np.abs(dv - dr.astype(np.float64)) / dr.astype(np.float64))[inner].max() < 1e-15
    low = t < -20
    assert np.array_equal(lt[low], t[low]) and np.all(dv[low] == 1.0)
    assert np.isnan(R.resid3(np.array([np.nan]))[0][0])


def test_residual_v4_emulation_accuracy():
    """The design of k_sweep16's logistic residual v4 (sweep16.hip: logit_resid4 -- 1024-entry exp
    table, fitted degree-3 polynomial, ln2/1024 rounded once, Stan's lower cutoff by a -1100 ldexp
    exponent, and the log terms summed as log1p of a per-lane running product flushed every 256
    elements), emulated in numpy by tools/residual_v3_accuracy.py, against Stan's bernoulli_logit
    term in long double: the lp sum of 2e5 uniform t in [-25, 25] and of a stretch where every e is
    below eps (t > 37: the product must still add them) within 1e-14 relative, dv within 4e-15
    relative away from the cutoff bands, exactly 1 below -20, a NaN kept in the sum."""
    import numpy as np
    from tools import residual_v3_accuracy as R
    rng = np.random.default_rng(4)
    for t in (rng.uniform(-25, 25, 200_000), rng.uniform(37, 45, 50_000), rng.uniform(-0.5, 3, 70_001)):
        lp, dv = R.resid4(t)
        lr, dr = R.stan(t)
        ref = float(lr.sum())
        assert abs(lp - ref) <= 1e-14 * abs(ref), (lp, ref)
        inner = np.abs(t) < 20
        if inner.any():
            assert (np.abs(dv - dr.astype(np.float64)) / dr.astype(np.float64))[inner].max() < 4e-15
    t = np.linspace(-30, -20.000001, 999)
    lp, dv = R.resid4(t)
    assert np.all(dv == 1.0) and abs(lp - float(t.sum())) <= 1e-15 * abs(float(t.sum()))   # lt = t exactly
    assert np.isnan(R.resid4(np.array([0.5, np.nan, -3.0]))[0])


def test_nuts_table_math_emulation_accuracy():
    """The fused NUTS kernel's table-driven exp / log1p (nuts.hip exp_mt, log1p01_mt), emulated in
    numpy by tools/nuts_math_accuracy.py: within 3 ulp of long-double references over the ranges
    the state machine feeds them, with exp's special values (0, inf, NaN) kept."""
    import numpy as np
    from tools import nuts_math_accuracy as M
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-40, 0, 100_000), rng.uniform(-700, 700, 100_000)])
    assert M.ulps(M.exp_mt(x), np.exp(x.astype(np.longdouble))).max() < 3
    e = np.concatenate([rng.uniform(0, 1, 100_000), 10.0 ** rng.uniform(-300, 0, 50_000), [0.0, 1.0]])
    assert M.ulps(M.log1p01_mt(e), np.log1p(e.astype(np.longdouble))).max() < 3
    sp = M.exp_mt(np.array([-np.inf, np.inf, np.nan, -1000.0, 1000.0]))
    assert sp[0] == 0 and sp[1] == np.inf and np.isnan(sp[2]) and sp[3] == 0 and sp[4] == np.inf


# ================================================================ the oracle's dense metric (dense_e)
def _dense_data(orc, family, n, d, seed, xscale=1.0):
    rng = np.random.default_rng(seed)
    X = xscale * rng.uniform(-1.7, 1.7, (n, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d) / xscale
    if family == "logistic":
        y = (rng.uniform(size=n) < 1 / (1 + np.exp(-(0.2 + X @ beta)))).astype(np.int32)
        return X, y, orc.FAM_LOGREG, d + 1
    return X, 0.3 + X @ beta + rng.normal(size=n), orc.FAM_LINREG, d + 2


def _rows_over_bars(rows):
    """rows: (where, got (q, lp, stats), want (q, lp, stats)).  Asserts the replay bars of
    tests/test_gpu_dense_metric.py's _check_rows on every row."""
    for where, (q, lp, st), (oq, olp, ost) in rows:
        assert st[2] == ost[2] and st[3] == ost[3] and st[4] == ost[4], (where, st, ost)
        np.testing.assert_allclose(q, oq, rtol=1e-8, atol=1e-10, err_msg=str(where))
        assert abs(lp - olp) <= 1e-9 * max(1.0, abs(olp)), (where, lp, olp)
        np.testing.assert_allclose(st[[0, 5]], ost[[0, 5]], rtol=1e-9, atol=1e-12, err_msg=str(where))


def test_oracle_cholesky_is_a_factor(orc):
    rng = np.random.default_rng(2)
    for D in (1, 2, 7, 40):
        G = rng.normal(size=(D, D))
        A = G @ G.T / D + 0.5 * np.eye(D)
        A = np.tril(A) + np.tril(A, -1).T
        L = orc.cholesky(A)
        assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0)
        np.testing.assert_allclose(L @ L.T, A, rtol=0, atol=1e-14 * np.abs(A).max() * D)
        np.testing.assert_allclose(L, np.linalg.cholesky(A), rtol=1e-12, atol=1e-15)
    bad = np.eye(3)
    bad[0, 1] = bad[1, 0] = 2.0
    with pytest.raises(ValueError, match="positive definite"):
        orc.cholesky(bad)


@pytest.mark.parametrize("family", ["schools", "logistic", "linear"])
def test_oracle_dense_with_a_diagonal_matrix_is_the_diagonal_oracle(orc, family):
    """M^-1 = diag(v): dense and diagonal transitions differ only in the order of the sums (the dense
    loops add exact zeros and divide by sqrt(v) where the diagonal path divides by sqrt(v) too)."""
    rng = np.random.default_rng(8)
    if family == "schools":
        m = orc.Model(orc.FAM_SCHOOLS, y=orc.SCHOOLS_Y, sigma=orc.SCHOOLS_SIGMA)
        eps_list = (0.1, 0.3)
    else:
        X, y, fam, _ = _dense_data(orc, family, 200, 7, 3)
        m = orc.Model(fam, X=X, y=y)
        eps_list = (0.02, 0.06)
    v = rng.uniform(0.5, 2.0, m.D)
    if family == "linear":
        v[0] /= 200
        v[-1] /= 400
    depths = set()
    for eps in eps_list:
        for c in range(6):
            q0 = rng.normal(0, 0.1, m.D)
            kw = dict(seed=13, gid=c, iteration=3, eps=eps, max_depth=6)
            a = m.transition(q0, inv_metric=np.diag(v), **kw)
            b = m.transition(q0, inv_metric=v, **kw)
            np.testing.assert_array_equal(a[2][1:5], b[2][1:5])
            np.testing.assert_allclose(a[0], b[0], rtol=1e-12, atol=0)
            assert abs(a[1] - b[1]) <= 1e-12 * abs(b[1])
            np.testing.assert_allclose(a[2][[0, 5]], b[2][[0, 5]], rtol=1e-12, atol=0)
            assert a[3] == b[3]
            depths.add(int(a[2][2]))
    assert max(depths) >= 3, depths


@pytest.mark.parametrize("family", ["logistic", "linear"])
def test_oracle_block_dense_metric_is_the_diagonal_oracle_on_reparametrised_data(orc, family):
    """blockdiag(a, L L^T[, s]) on (X, q) vs the diagonal oracle on (X L, q'), d = 9, max_depth 6."""
    d, n, chains = 9, 300, 16
    lin = family == "linear"
    X, y, fam, D = _dense_data(orc, family, n, d, 100 * d + int(lin), xscale=0.07 if lin else 1.0)
    rng = np.random.default_rng(7 * d + int(lin))
    Lb = np.tril(rng.normal(0, 0.3 / np.sqrt(d), (d, d)), -1) + np.diag(rng.uniform(0.5, 1.5, d))
    a, s = rng.uniform(0.5, 2.0, 2)
    if lin:
        a, s = a / n, s / (2 * n)
    Minv = np.zeros((D, D))
    Minv[0, 0] = a
    B = Lb @ Lb.T
    Minv[1:d + 1, 1:d + 1] = np.tril(B) + np.tril(B, -1).T
    im = np.ones(D)
    im[0] = a
    if lin:
        Minv[-1, -1] = im[-1] = s
    q0p = rng.normal(0, 0.1, (chains, D))
    to_q = lambda qp: np.concatenate([qp[:1], Lb @ qp[1:d + 1], qp[d + 1:]])   # noqa: E731
    om, omr = orc.Model(fam, X=X, y=y), orc.Model(fam, X=np.ascontiguousarray(X @ Lb), y=y)
    rows, depths = [], set()
    for eps in (0.02, 0.05, 0.1, 0.3):
        for c in range(chains):
            kw = dict(seed=31, gid=c, iteration=4, eps=eps, max_depth=6)
            oq, olp, ost, _ = omr.transition(q0p[c], inv_metric=im, **kw)
            q, lp, st, _ = om.transition(to_q(q0p[c]), inv_metric=Minv, **kw)
            rows.append(((eps, c), (q, lp, st), (to_q(oq), olp, ost)))
            depths.add(int(ost[2]))
    assert max(depths) >= 4, depths
    _rows_over_bars(rows)


@pytest.mark.parametrize("D", [11, 202])
def test_oracle_general_dense_metric_one_leaf(orc, D):
    """A random SPD M^-1 with alpha-beta and log sigma cross terms at max_depth 1: the draw is q0 or
    one of the two one-leapfrog candidates of p = L^-T u, in numpy (the arithmetic of
    test_gpu_dense_metric.py's test_general_dense_metric_one_leaf)."""
    d, n, seed, it = D - 2, 300, 19, 0
    X, y, fam, _ = _dense_data(orc, "linear", n, d, 5 * D)
    rng = np.random.default_rng(D)
    G = rng.normal(size=(D, D))
    Minv = (G @ G.T / D + 0.5 * np.eye(D)) / n
    Minv = np.tril(Minv) + np.tril(Minv, -1).T
    assert abs(Minv[0, 1]) > 0 and abs(Minv[-1, 1]) > 0 and abs(Minv[-1, 0]) > 0
    L = np.linalg.cholesky(Minv)
    om = orc.Model(fam, X=X, y=y)
    eps = 0.35 if D == 11 else 0.1
    ols, _ = orc.linreg_exact_moments(X, y)
    rss = float(((y - np.hstack([np.ones((n, 1)), X]) @ ols) ** 2).sum())
    q0 = np.concatenate([ols, [0.5 * np.log(rss / n)]]) + np.random.default_rng(3).normal(0, 0.02, (16, D))
    moved = 0
    for c in range(16):
        q, lp, st, ng = om.transition(q0[c], seed=seed, gid=c, iteration=it, eps=eps, inv_metric=Minv, max_depth=1)
        u = np.array([orc.lib().orc_normal(seed, c, it, 0, e, orc.TAG_MOM) for e in range(D)])
        p = np.linalg.solve(L.T, u)
        lp0, g0 = om.lpgrad(q0[c])
        H0 = -lp0 + 0.5 * p @ Minv @ p
        cands = []
        for sgn in (1.0, -1.0):
            ph = p + 0.5 * sgn * eps * g0
            q1 = q0[c] + sgn * eps * (Minv @ ph)
            lp1, g1 = om.lpgrad(q1)
            p1 = ph + 0.5 * sgn * eps * g1
            H1 = -lp1 + 0.5 * p1 @ Minv @ p1
            cands.append((q1, 1.0 if H0 - H1 > 0 else float(np.exp(H0 - H1)), lp1))
        assert st[2] == 1 and st[3] == 1 and ng == 2, st
        if np.array_equal(q, q0[c]):
            err = min(abs(st[0] - a) for _, a, _ in cands)
        else:
            moved += 1
            q1, acc, lp1 = cands[int(np.argmin([np.abs(q - c1).max() for c1, _, _ in cands]))]
            np.testing.assert_allclose(q, q1, rtol=1e-8, atol=1e-10, err_msg=str(c))
            assert abs(lp - lp1) <= 1e-9 * max(1.0, abs(lp1)), (lp, lp1)
            err = abs(st[0] - acc)
        assert err <= 1e-9, (c, st[0], [a for _, a, _ in cands])
    assert moved > 8, moved


def _correlated_linear(n=400, d=12, rho=0.9, seed=5):
    """The data of tests/test_gpu_dense_metric.py's dense_e tests."""
    rng = np.random.default_rng(seed)
    X = np.sqrt(rho) * rng.normal(size=(n, 1)) + np.sqrt(1 - rho) * rng.normal(size=(n, d))
    beta = rng.normal(0, 1, d)
    return X, 0.3 + X @ beta + rng.normal(size=n)


def test_oracle_dense_run_adapts_by_the_formula_and_samples_the_posterior(orc):
    """run_chain(metric="dense_e") on the correlated linear data: the final matrix is Stan's
    covar_adaptation formula on the run's own last window (num_warmup 300: draws 150..249), the
    closed-form moments hold within 5 MCSE and the trees are at most a third of diag_e's."""
    from stark_amd.diagnostics import ess
    X, y = _correlated_linear()
    mean, _ = orc.linreg_exact_moments(X, y)
    om = orc.Model(orc.FAM_LINREG, X=X, y=y)
    chains, nw, ns = 8, 300, 300
    dense = [om.run_chain(num_warmup=nw, num_samples=ns, seed=5, gid=c, metric="dense_e") for c in range(chains)]
    diag = [om.run_chain(num_warmup=nw, num_samples=ns, seed=5, gid=c) for c in range(chains)]
    for c, r in enumerate(dense):
        assert r["inv_metric"].shape == (14, 14)
        w = r["q"][150:250]
        n = len(w)
        cov = np.cov(w.T, ddof=1)
        want = (n / (n + 5.0)) * cov + 1e-3 * (5.0 / (n + 5.0)) * np.eye(14)
        sc = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
        assert np.all(np.abs(r["inv_metric"] - want) <= 1e-12 * sc), (c, (np.abs(r["inv_metric"] - want) / sc).max())
        np.testing.assert_array_equal(r["inv_metric"], r["inv_metric"].T)
    z = []
    for k in range(13):
        x = np.stack([r["q"][nw:, k] for r in dense])
        z.append((x.mean() - mean[k]) / (x.std(ddof=1) / np.sqrt(ess(x))))
    assert np.all(np.abs(z) < 5), z
    lf_dense = np.mean([r["stats"][nw:, 3].mean() for r in dense])
    lf_diag = np.mean([r["stats"][nw:, 3].mean() for r in diag])
    assert lf_dense <= lf_diag / 3.0, (lf_dense, lf_diag)


def test_oracle_metric_selector(orc):
    """unit_e keeps the unit metric and adapts the step; diag_e is the default; a dense initial
    matrix that is not positive definite is the step-size-error code."""
    X, y, fam, D = _dense_data(orc, "logistic", 300, 4, 6)
    om = orc.Model(fam, X=X, y=y)
    kw = dict(num_warmup=150, num_samples=10, seed=4, gid=1)
    u = om.run_chain(metric="unit_e", **kw)
    np.testing.assert_array_equal(u["inv_metric"], np.ones(D))
    assert u["stepsize"] != 1.0 and u["stepsize"] > 0
    a, b = om.run_chain(**kw), om.run_chain(metric="diag_e", **kw)
    np.testing.assert_array_equal(a["q"], b["q"])
    assert np.any(a["inv_metric"] != 1.0)
    # a diagonal initial matrix: the init buffer (75 transitions under the initial metric) is diag_e's
    v = np.linspace(0.5, 1.5, D)
    e = om.run_chain(metric="dense_e", inv_metric=np.diag(v), **kw)
    assert e["inv_metric"].shape == (D, D) and np.abs(e["inv_metric"] - np.diag(np.diag(e["inv_metric"]))).max() > 0
    bad = np.eye(D)
    bad[0, 1] = bad[1, 0] = 2.0
    with pytest.raises(RuntimeError, match="positive definite"):
        om.run_chain(metric="dense_e", inv_metric=bad, **kw)
    with pytest.raises(ValueError, match="shape"):
        om.run_chain(metric="dense_e", inv_metric=np.eye(D + 1), **kw)


def test_oracle_self_replay_reports_flips_and_errors(orc):
    """On a proper posterior the oracle replays itself far inside the bars; on linearly separable
    logistic data (flat priors: the chains run off) it does not, and the helper says so."""
    X, y, fam, D = _dense_data(orc, "logistic", 400, 9, 77)
    om = orc.Model(fam, X=X, y=y)
    rng = np.random.default_rng(1)
    G = rng.normal(size=(D, D))
    Minv = (G @ G.T / D + 0.5 * np.eye(D)) / 400
    Minv = np.tril(Minv) + np.tril(Minv, -1).T
    starts = [(rng.normal(0, 0.1, D), c, 2, 0.2) for c in range(8)]
    flips, worst = orc.self_replay(om, starts, seed=9, inv_metric=Minv, factor=orc.cholesky(Minv), max_depth=6)
    assert flips == 0 and worst <= 1e-2, (flips, worst)
    flips0, worst0 = orc.self_replay(om, starts, seed=9, inv_metric=Minv, max_depth=6, rel=0.0)
    assert flips0 == 0 and worst0 == 0.0                 # the same start: the same bits, factored per call or once
    far = [(q * 1e3, c, it, eps) for q, c, it, eps in starts]
    _, worst_far = orc.self_replay(om, far, seed=9, inv_metric=Minv, max_depth=6, rel=1e-6)
    assert worst_far > 1.0, worst_far
