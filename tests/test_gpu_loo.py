"""The PSIS-LOO sweep (stk_loo, loo.hip) against a numpy restatement of the definitions in np.longdouble,
for the three regression families.

ll_is is the normalised pointwise log likelihood of tests/test_gpu_predictive.py (restated here).  For
one row with S draws (include/stark_hip.h):
    lr = -ll, shifted by its maximum; M = ceil(min(0.2 S, 3 sqrt S)); M < 5 or a constant tail: khat = +inf
    and no smoothing; else the M largest lr are the tail t, cut the largest value outside it,
    x = exp(t) - exp(cut), the Zhang-Stephens fit with the loo package's prior gives (khat, sigma), and a
    finite khat replaces t_j by log(sigma expm1(-khat log1p(-p_j)) / khat + exp(cut)), p_j = (j - 0.5) / M;
    lw = min(lr, 0) - logsumexp; elpd_loo = logsumexp(ll + lw); lppd = logsumexp(ll) - log S;
    p_loo = lppd - elpd_loo.  A non-finite ll: elpd_loo, p_loo and khat NaN, lppd what IEEE gives.
    totals    n, sum lppd, sum p_loo, sum elpd_loo, sum elpd_loo^2, #(khat > 0.5), #(khat > 0.7),
              #(rows with a non-finite elpd_loo, lppd or p_loo, or a NaN khat)
The bars: with scale_i = max(1, max_s |ll_is|), elpd_loo, lppd and p_loo within 1e-10 scale_i (the project's
density bar), every total within 1e-10 max(1, sum_i |term_i|).  khat has no derived bar: every case
measures the float64 run of this restatement against the longdouble one and takes max(1e-10, 1000 x that
error) -- the factor covers the device ll's ~2 ulp feeding a fit whose conditioning varies by row.  The
counts are exact: every case first asserts on the restatement that no khat lies within 1e-6 of 0.5 or 0.7.
Every case prints its largest errors and its khat bar as a MAXERR line (tools/loo_errors.py collects them).
"""
import ctypes
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 1e-10
DBL_MAX = np.finfo(np.float64).max
FAMILIES = ("logistic", "poisson", "linear")
DS = (1, 3, 4, 5, 16, 17, 100, 128)
NS = (1, 15, 16, 17, 33)
SS = (1, 2, 20, 21, 33, 64, 65, 224, 225, 226, 256, 257, 1000, 1023, 1024)   # 256 | 257: 4 | 8 waves per block
KEYS = ("elpd_loo", "khat", "lppd", "p_loo")
L = np.longdouble


def make_data(family, n, d, seed=None):
    """X ~ U(-1.7, 1.7) with one all-zero row (n >= 3); y from the family at a true (alpha, beta[, sigma])."""
    rng = np.random.default_rng(1000 * n + d if seed is None else seed)
    X = rng.uniform(-1.7, 1.7, (n, d))
    if n >= 3:
        X[n // 2] = 0.0
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    eta = 0.3 + X @ beta
    if family == "logistic":
        y = (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.int32)
        truth = np.concatenate([[0.3], beta])
    elif family == "poisson":
        y = rng.poisson(np.exp(eta)).astype(np.int32)
        truth = np.concatenate([[0.3], beta])
    else:
        y = eta + 0.7 * rng.normal(size=n)
        truth = np.concatenate([[0.3], beta, [np.log(0.7)]])
    return rng, X, y, truth


def draws_near(rng, truth, S, sd=0.1):
    return truth[None, :] + rng.normal(0, sd, (S, truth.size))


def ref_ll(family, X, y, Q):
    """ll [n, S] in longdouble; an exp past the largest double is +inf, as in fp64."""
    d = X.shape[1]
    Xl, Ql, yl = X.astype(L), np.asarray(Q).astype(L), np.asarray(y).astype(L)[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        eta = Ql[:, 0][None, :] + Xl @ Ql[:, 1:d + 1].T
        if family == "logistic":
            z = (2 * yl - 1) * eta
            ll = np.minimum(z, 0) - np.log1p(np.exp(-np.abs(z)))
        elif family == "poisson":
            lg = np.array([np.log(np.arange(1, int(v) + 1).astype(L)).sum() if v > 0 else L(0) for v in np.asarray(y)], L)
            g = np.exp(eta)
            g[g > DBL_MAX] = np.inf
            ll = yl * eta - g - lg[:, None]
        else:
            u = Ql[:, -1][None, :]
            r = yl - eta
            ll = -L(0.5) * np.log(2 * L(np.pi)) - u - L(0.5) * r * r * np.exp(-2 * u)
    return ll


def tail_len(S):
    """ceil(min(0.2 S, 3 sqrt S)) in integers (tests/test_host_loo.py: the floating-point formula for S <= 1024)."""
    return min(-(-S // 5), math.isqrt(9 * S - 1) + 1)


def lse(a):
    """logsumexp; -inf entries add 0, every entry -inf gives -inf, a NaN gives NaN."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = a.max()
        if not np.isfinite(m):
            return m if (np.isnan(m) or m < 0) else a.dtype.type(np.inf)
        return m + np.log(np.exp(a - m).sum())


def psis_row(ll, T):
    """(elpd_loo, khat, lppd, p_loo) of one row in the arithmetic T (np.longdouble or np.float64)."""
    ll = ll.astype(T)
    S = ll.size
    nan, inf = T(np.nan), T(np.inf)
    lppd = lse(ll) - np.log(T(S))
    if not np.isfinite(ll).all():
        return nan, nan, lppd, nan
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        lr = -ll
        lr = lr - lr.max()
        order = np.argsort(lr, kind="stable")
        lr, lls = lr[order], ll[order]
        M, khat = tail_len(S), inf
        if M >= 5:
            t, cut = lr[S - M:], lr[S - M - 1]
            if t[-1] - t[0] > 0:
                x = np.exp(t) - np.exp(cut)
                N = M
                Mg = 30 + int(math.isqrt(N))
                xstar = x[int(math.floor(N / 4 + 0.5)) - 1]
                j = np.arange(1, Mg + 1).astype(T)
                theta = 1 / x[-1] + (1 - np.sqrt(Mg / (j - T(0.5)))) / 3 / xstar
                k = np.log1p(-theta[:, None] * x[None, :]).sum(axis=1) / N
                l = N * (np.log(-theta / k) - k - 1)
                w = 1 / np.exp(l[None, :] - l[:, None]).sum(axis=1)
                th = (theta * w).sum()
                k = np.log1p(-th * x).sum() / N
                sigma = -k / th
                khat = (k * N + 5) / (N + 10)
                if np.isfinite(khat):
                    p = (np.arange(1, M + 1).astype(T) - T(0.5)) / M
                    lr = lr.copy()
                    lr[S - M:] = np.log(sigma * np.expm1(-khat * np.log1p(-p)) / khat + np.exp(cut))
        lw = np.minimum(lr, 0)
        lw = lw - lse(lw)
        elpd = lse(lls + lw)
    return elpd, khat, lppd, lppd - elpd


def ref_loo(family, X, y, Q, skip=()):
    """Per-row {elpd_loo, khat, lppd, p_loo, scale} (float64, computed in longdouble), the khat bar of the
    case (max(1e-10, 1000 x the float64 restatement's largest khat error)), the [8] totals and their scales.
    skip: rows whose khat is not compared (their exponentials underflow in float64 and not in longdouble)."""
    ll = ref_ll(family, X, y, Q)
    n, S = ll.shape
    out, out64 = np.empty((n, 4), L), np.empty((n, 4))
    for i in range(n):
        out[i] = psis_row(ll[i], L)
        out64[i] = psis_row(ll[i].astype(np.float64), np.float64)
    keep = np.ones(n, bool)
    keep[list(skip)] = False
    kf = np.isfinite(out[:, 1].astype(np.float64)) & keep
    assert np.array_equal(kf, np.isfinite(out64[:, 1]) & keep)
    kerr = float(np.abs(out64[kf, 1] - out[kf, 1]).max()) if kf.any() else 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        fin = np.where(np.isfinite(ll), np.abs(ll), 0)
        scale = np.maximum(1, fin.max(axis=1)).astype(np.float64)
        e, k, lppd, p = out[:, 0], out[:, 1], out[:, 2], out[:, 3]
        bad = ~(np.isfinite(e) & np.isfinite(lppd) & np.isfinite(p)) | np.isnan(k)
        tot = np.array([n, lppd.sum(), p.sum(), e.sum(), (e * e).sum(), (k > 0.5).sum(), (k > 0.7).sum(), bad.sum()], L)
        tscale = np.array([1, np.abs(lppd).sum(), np.abs(p).sum(), np.abs(e).sum(), (e * e).sum(), 0, 0, 0], L)
    rows = {key: out[:, j].astype(np.float64) for j, key in enumerate(KEYS)}
    rows["scale"] = scale
    # rows where the float64 restatement takes the longdouble one's branches (no underflow changes the tail)
    rows["agree"] = np.isfinite(out64[:, 1]) == np.isfinite(out[:, 1].astype(np.float64))
    # the counts are exact only away from the thresholds
    kk = rows["khat"][np.isfinite(rows["khat"]) & keep]
    assert not np.any(np.abs(kk - 0.5) < 1e-6) and not np.any(np.abs(kk - 0.7) < 1e-6)
    return rows, max(1e-10, 1000 * kerr), tot.astype(np.float64), np.maximum(1, np.where(np.isfinite(tscale), tscale, 0)).astype(np.float64)


def same_class(a, b):
    """Non-finite entries agree exactly (NaN with NaN, each infinity with itself)."""
    a, b = np.asarray(a), np.asarray(b)
    nf = ~np.isfinite(b)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[nf & ~np.isnan(b)], b[nf & ~np.isnan(b)])
                and np.isfinite(a[~nf]).all())


def row_errors(rows, ref, kbar, skip=()):
    """The largest error of elpd_loo / lppd / p_loo in units of their bar, and of khat in units of kbar
    (<= 1 passes); non-finite entries must agree.  skip: rows whose khat is not compared."""
    worst = 0.0
    for key in ("elpd_loo", "lppd", "p_loo"):
        assert same_class(rows[key], ref[key]), key
        f = np.isfinite(ref[key])
        if f.any():
            worst = max(worst, float((np.abs(rows[key][f] - ref[key][f]) / (BAR * ref["scale"][f])).max()))
    keep = np.ones(ref["khat"].size, bool)
    keep[list(skip)] = False
    assert same_class(rows["khat"][keep], ref["khat"][keep]), "khat"
    f = np.isfinite(ref["khat"]) & keep
    kerr = float(np.abs(rows["khat"][f] - ref["khat"][f]).max()) if f.any() else 0.0
    return worst, kerr / kbar, kerr


def total_errors(tot, rtot, tscale):
    assert same_class(tot, rtot)
    assert tot[0] == rtot[0] and tot[5] == rtot[5] and tot[6] == rtot[6] and tot[7] == rtot[7]
    f = np.isfinite(rtot)
    return float((np.abs(tot[f] - rtot[f]) / (BAR * tscale[f])).max())


def check_case(name, tot, rows, ref, kbar, rtot, tscale):
    e_rows, e_k, kerr = row_errors(rows, ref, kbar)
    e_tot = total_errors(tot, rtot, tscale)
    print(f"MAXERR loo[{name}] rows {e_rows:.3e} totals {e_tot:.3e} (units of the 1e-10 bars) khat {kerr:.3e} bar {kbar:.3e}")
    assert e_rows <= 1 and e_tot <= 1 and e_k <= 1, (name, e_rows, e_tot, kerr, kbar)


def multi_chunk_n(d, S):
    """The smallest n of at least 3 chunks whose last 16-row tile is ragged, from the launch info."""
    from stark_amd import engine
    n = 17
    while engine.loo_launch(n, d, S)["G"] < 3 or n % 16 == 0:
        n += 1
    return n


def shapes():
    out = [(37, d, 100) for d in DS]
    out += [(n, 100, 100) for n in NS] + [(None, 100, 100)]
    out += [(33, 17, S) for S in SS]
    return out


@pytest.mark.parametrize("n,d,S", shapes())
@pytest.mark.parametrize("family", FAMILIES)
def test_rows_and_totals_match_the_restatement(ctx, family, n, d, S):
    """Two shards (the first a third of the rows; the second is checked), draws = truth + N(0, 0.1)."""
    from stark_amd import engine
    if n is None:
        n = multi_chunk_n(d, S)
        info = engine.loo_launch(n, d, S)
        assert info["G"] >= 3 and n % info["T"] != 0 and engine.loo_launch(n - 1, d, S)["G"] < 3
    rng, X, y, truth = make_data(family, n, d)
    Q = draws_near(rng, truth, S)
    ref, kbar, rtot, tscale = ref_loo(family, X, y, Q)
    k = max(1, n // 3)
    m = engine.Model(ctx, family, [{"x": X[:k], "y": y[:k]}, {"x": X, "y": y}])
    try:
        tot, rows = m.loo(Q, 1, rows=True)
        if S <= 20:
            assert np.all(rows["khat"] == np.inf) and tot[5] == n and tot[6] == n
        if S == 1:
            assert np.array_equal(rows["elpd_loo"], rows["lppd"]) and np.all(rows["p_loo"] == 0)
            lp = m.log_predictive(Q, 1, rows=True)[1]["lppd"]
            assert np.abs(rows["lppd"] - lp).max() <= BAR * ref["scale"].max()
        assert tot[7] == 0 and np.isfinite(tot).all()
        check_case(f"{family}-{n}-{d}-{S}", tot, rows, ref, kbar, rtot, tscale)
        assert np.array_equal(m.loo(Q, 1), tot)                          # rows = NULL changes no total
    finally:
        m.close()


@functools.lru_cache(maxsize=None)
def _diag_case(family, S, sd, seed):
    rng, X, y, truth = make_data(family, 64, 5, seed=seed)
    Q = draws_near(rng, truth, S, sd=sd)
    return X, y, Q, ref_loo(family, X, y, Q)


@pytest.mark.parametrize("family,S,sd,seed,kind", [("logistic", 100, 0.05, 11, "low"), ("logistic", 100, 0.3, 12, "wide"),
                                                   ("linear", 256, 0.2, 13, "wide")])
def test_both_sides_of_the_diagnostic(ctx, family, S, sd, seed, kind):
    """A low-noise case with every khat below 0.5, and two wide cases with rows above 0.7 (the logistic one
    also has rows below 0.5): the restatement says so first, then the counts must be exact."""
    from stark_amd import engine
    X, y, Q, (ref, kbar, rtot, tscale) = _diag_case(family, S, sd, seed)
    if kind == "low":
        assert np.all(ref["khat"] < 0.5) and rtot[5] == 0
    else:
        assert (ref["khat"] > 0.7).sum() >= 1 and rtot[6] >= 1
        if family == "logistic":
            assert (ref["khat"] < 0.5).sum() >= 1
    m = engine.Model(ctx, family, [{"x": X, "y": y}])
    try:
        tot, rows = m.loo(Q, 0, rows=True)
    finally:
        m.close()
    print(f"khat of the restatement: {np.sort(ref['khat'])[[0, 32, 63]]}, above 0.7: {int(rtot[6])} of 64")
    check_case(f"{family}-{kind}-sd{sd}", tot, rows, ref, kbar, rtot, tscale)


@pytest.mark.parametrize("family", FAMILIES)
def test_identical_draws_are_not_smoothed(ctx, family):
    """All S draws the same point: a constant tail, khat = +inf, elpd_loo_i = lppd_i = ll_i."""
    from stark_amd import engine
    n, d, S = 37, 5, 100
    rng, X, y, truth = make_data(family, n, d)
    Q = np.tile(draws_near(rng, truth, 1), (S, 1))
    ll = ref_ll(family, X, y, Q[:1])[:, 0].astype(np.float64)
    m = engine.Model(ctx, family, [{"x": X, "y": y}])
    try:
        tot, rows = m.loo(Q, 0, rows=True)
    finally:
        m.close()
    sc = BAR * np.maximum(1, np.abs(ll))
    assert np.all(rows["khat"] == np.inf) and tot[5] == n and tot[6] == n and tot[7] == 0
    err = max(float((np.abs(rows[k] - ll) / sc).max()) for k in ("elpd_loo", "lppd"))
    print(f"MAXERR loo[{family}-identical-draws] rows {err:.3e} (units of the 1e-10 bar)")
    assert err <= 1 and np.all(np.abs(rows["p_loo"]) <= sc)
    ref, kbar, rtot, tscale = ref_loo(family, X, y, Q)
    check_case(f"{family}-identical-draws", tot, rows, ref, kbar, rtot, tscale)


def test_logistic_extreme_eta_stays_finite(ctx):
    """Rows with eta = +-40, +-750 and 745 at every draw (the draws differ by N(0, 1e-3)): elpd_loo, lppd and
    p_loo are finite and right.  Their khat is not compared: exp(-|eta|) and the differences between draws
    underflow in float64 and not in longdouble, so the two restatements see different tails."""
    from stark_amd import engine
    n, d, S = 37, 100, 33
    rng, X, y, truth = make_data("logistic", n, d)
    q = rng.normal(0, 0.3, d + 1)
    b = q[1:]
    for row, eta in ((1, 40.0), (2, -40.0), (3, 750.0), (4, -750.0), (20, 745.0)):
        X[row] = (eta - q[0]) * b / (b @ b)
    Q = np.tile(q, (S, 1)) + rng.normal(0, 1e-3, (S, d + 1))
    extreme = (1, 2, 3, 4, 20)
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        tot, rows = m.loo(Q, 0, rows=True)
    finally:
        m.close()
    ref, kbar, rtot, tscale = ref_loo("logistic", X, y, Q, skip=extreme)
    assert all(np.isfinite(rows[k]).all() for k in ("elpd_loo", "lppd", "p_loo")) and np.isfinite(tot[:5]).all()
    e_rows, e_k, kerr = row_errors(rows, ref, kbar, skip=extreme)
    e_tot = float((np.abs(tot[:5] - rtot[:5]) / (BAR * tscale[:5])).max())
    print(f"MAXERR loo[logistic-extreme-eta] rows {e_rows:.3e} totals {e_tot:.3e} khat {kerr:.3e} bar {kbar:.3e}")
    assert e_rows <= 1 and e_k <= 1 and e_tot <= 1 and tot[0] == n


def test_non_finite_draws_are_never_a_finite_wrong_number(ctx):
    """A NaN coordinate in one draw: every row NaN and counted, for the three families.  Poisson: a draw
    whose beta_1 is 800 overflows exp(eta) exactly in the rows with x_1 > (709.78 - alpha) / 800: those rows
    have NaN elpd_loo, p_loo and khat and a finite lppd; the others stay finite, lppd is right in every row,
    and elpd_loo and p_loo are right where the float64 restatement takes the longdouble one's branches.
    (That draw's ll is so low in some rows that exp of the shifted ratios underflows to 0 in float64 and
    not in longdouble: float64 then sees a tail it cannot fit and does not smooth, longdouble smooths.)"""
    from stark_amd import engine
    n, d, S = 40, 5, 33
    for family in FAMILIES:
        rng, X, y, truth = make_data(family, n, d)
        Q = draws_near(rng, truth, S)
        m = engine.Model(ctx, family, [{"x": X, "y": y}])
        try:
            bad = Q.copy()
            bad[3, 1] = np.nan
            tot, rows = m.loo(bad, 0, rows=True)
            assert all(np.isnan(rows[k]).all() for k in KEYS), family
            assert tot[7] == n and tot[0] == n and np.isnan(tot[1:5]).all() and tot[5] == 0 and tot[6] == 0
            ref, _, rtot, _ = ref_loo(family, X, y, bad)
            assert same_class(tot, rtot) and all(same_class(rows[k], ref[k]) for k in KEYS)
            if family == "poisson":
                one = Q.copy()
                one[7, 1] = 800.0
                ll = ref_ll(family, X, y, one)
                hit = ~np.isfinite(ll).all(axis=1)
                assert 0 < hit.sum() < n and not hit[n // 2]             # some rows, never the zero row
                tot, rows = m.loo(one, 0, rows=True)
                ref, kbar, rtot, tscale = ref_loo(family, X, y, one, skip=range(n))
                for k in ("elpd_loo", "p_loo"):
                    assert np.array_equal(np.isnan(rows[k]), hit), k
                assert np.isnan(rows["khat"][hit]).all()
                assert np.isfinite(rows["lppd"]).all() and tot[7] == (hit | np.isnan(rows["khat"])).sum()
                sel = ref["agree"] & ~hit
                assert sel.sum() >= 5
                for k in ("elpd_loo", "p_loo"):
                    assert np.isfinite(rows[k][~hit]).all()
                    rows[k], ref[k] = np.where(sel, rows[k], 0.0), np.where(sel, ref[k], 0.0)
                e_rows, _, _ = row_errors(rows, ref, kbar, skip=range(n))
                print(f"MAXERR loo[poisson-one-overflowing-draw] rows {e_rows:.3e} (units of the 1e-10 bar)")
                assert e_rows <= 1 and same_class(tot[:5], rtot[:5]) and abs(tot[1] - rtot[1]) <= BAR * tscale[1]
                assert tot[5] == (rows["khat"] > 0.5).sum() and tot[6] == (rows["khat"] > 0.7).sum()
                every = Q.copy()
                every[:, 0] = 800.0
                tot, rows = m.loo(every, 0, rows=True)
                assert np.all(rows["lppd"] == -np.inf) and all(np.isnan(rows[k]).all() for k in ("elpd_loo", "khat", "p_loo"))
                assert tot[7] == n and tot[1] == -np.inf
        finally:
            m.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_rows_carry_the_same_bits_anywhere(ctx, family):
    """Rows 0 .. k - 1 of a shard equal the rows of a k-row shard with the same data; shard = -1 over 3
    shards of different n equals the three single calls, rows and totals, in either shard order (a shard
    is shard 0 of one model and shard 2 of the other); two repeats are bit-identical."""
    from stark_amd import engine
    d, S = 17, 100
    parts = []
    for n in (37, multi_chunk_n(d, S), 150):
        rng, X, y, truth = make_data(family, n, d, seed=77 + n)
        parts.append({"x": X, "y": y})
    Q = draws_near(np.random.default_rng(5), truth, S, sd=0.1)
    m = engine.Model(ctx, family, parts)
    m2 = engine.Model(ctx, family, parts[::-1])
    k = 41
    mk = engine.Model(ctx, family, [{"x": parts[2]["x"][:k], "y": parts[2]["y"][:k]}])
    try:
        tot, rows = m.loo(Q, None, rows=True)
        again, rows_again = m.loo(Q, None, rows=True)
        assert np.array_equal(tot, again) and all(np.array_equal(rows[key], rows_again[key]) for key in KEYS)
        tot2, rows2 = m2.loo(Q, None, rows=True)
        assert tot.shape == (3, 8) and rows["khat"].shape == (sum(m.n_rows),)
        assert np.array_equal(tot2, tot[::-1])
        assert np.array_equal(m.loo(Q, None), tot)                       # rows = NULL changes no total
        off = np.concatenate([[0], np.cumsum(m.n_rows)])
        off2 = np.concatenate([[0], np.cumsum(m2.n_rows)])
        for s in range(3):
            t1, r1 = m.loo(Q, s, rows=True)
            assert np.array_equal(t1, tot[s])
            for key in KEYS:
                assert np.array_equal(r1[key], rows[key][off[s]:off[s + 1]])
                assert np.array_equal(r1[key], rows2[key][off2[2 - s]:off2[3 - s]])
        _, rk = mk.loo(Q, 0, rows=True)
        for key in KEYS:
            assert np.array_equal(rk[key], rows[key][off[2]:off[2] + k])
        ref, kbar, rtot, tscale = ref_loo(family, parts[0]["x"], parts[0]["y"], Q)
        check_case(f"{family}-bits-shard0", tot[0], {key: rows[key][:off[1]] for key in KEYS}, ref, kbar, rtot, tscale)
    finally:
        m.close()
        m2.close()
        mk.close()


@pytest.mark.parametrize("n", [17, 65])
def test_no_write_outside_the_outputs(ctx, n):
    """Through ctypes, rows and totals inside larger buffers of a sentinel: nothing outside [n][4] and
    [8] changes."""
    from stark_amd import _lib, engine
    d, S, pad, sentinel = 5, 33, 64, -7.25
    rng, X, y, truth = make_data("logistic", n, d)
    Q = np.ascontiguousarray(draws_near(rng, truth, S))
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        rbuf = np.full(pad + 4 * n + pad, sentinel)
        tbuf = np.full(pad + 8 + pad, sentinel)
        fn = _lib.load().stk_loo
        _lib.check(fn(m._h, 0, Q.ctypes.data, S, ctypes.c_void_p(rbuf.ctypes.data + 8 * pad),
                      ctypes.c_void_p(tbuf.ctypes.data + 8 * pad)))
        for buf, k in ((rbuf, 4 * n), (tbuf, 8)):
            assert np.all(buf[:pad] == sentinel) and np.all(buf[pad + k:] == sentinel)
            assert np.all(buf[pad:pad + k] != sentinel)
        tot, rows = m.loo(Q, 0, rows=True)
        assert np.array_equal(tbuf[pad:pad + 8], tot)
        got = rbuf[pad:pad + 4 * n].reshape(n, 4)
        assert all(np.array_equal(got[:, j], rows[key]) for j, key in enumerate(KEYS))
        # totals alone, rows alone
        tbuf[:] = sentinel
        _lib.check(fn(m._h, 0, Q.ctypes.data, S, None, ctypes.c_void_p(tbuf.ctypes.data + 8 * pad)))
        assert np.array_equal(tbuf[pad:pad + 8], tot) and np.all(tbuf[:pad] == sentinel) and np.all(tbuf[pad + 8:] == sentinel)
        r2 = np.full(4 * n, sentinel)
        _lib.check(fn(m._h, 0, Q.ctypes.data, S, r2.ctypes.data, None))
        assert np.array_equal(r2, rbuf[pad:pad + 4 * n])
    finally:
        m.close()


def test_device_rows_are_written_in_place(ctx):
    """rows as a device tensor: written where it lies, the same bits as the host copy."""
    import torch
    from stark_amd import _lib, engine
    n, d, S = 65, 5, 33
    rng, X, y, truth = make_data("poisson", n, d)
    Q = np.ascontiguousarray(draws_near(rng, truth, S))
    m = engine.Model(ctx, "poisson", [{"x": X, "y": y}])
    try:
        t = torch.full((n + 2, 4), -7.25, dtype=torch.float64, device=f"cuda:{ctx.device}")
        torch.cuda.synchronize()
        tot = np.empty(8)
        _lib.check(_lib.load().stk_loo(m._h, 0, Q.ctypes.data, S, ctypes.c_void_p(t.data_ptr() + 32), tot.ctypes.data))
        host = t.cpu().numpy()
        tot2, rows = m.loo(Q, 0, rows=True)
        assert np.all(host[0] == -7.25) and np.all(host[-1] == -7.25)
        assert all(np.array_equal(host[1:-1, j], rows[key]) for j, key in enumerate(KEYS))
        assert np.array_equal(tot, tot2)
    finally:
        m.close()


def test_refusals_name_the_family_or_the_limit(ctx):
    from stark_amd import _lib, engine
    from stark_amd._lib import StarkHipError
    m = engine.Model(ctx, "schools", [{"y": [28.0, 8.0, -3.0], "sigma": [15.0, 10.0, 16.0]}])
    try:
        with pytest.raises(StarkHipError, match="schools") as e:
            m.loo(np.zeros((4, m.D[0])), 0)
        assert e.value.code == -1
    finally:
        m.close()
    rng = np.random.default_rng(3)
    m = engine.Model(ctx, "logistic", [{"x": rng.normal(size=(20, 129)), "y": rng.integers(0, 2, 20)}])
    try:
        with pytest.raises(StarkHipError, match="d = 129") as e:
            m.loo(np.zeros((4, 130)), 0)
        assert e.value.code == -1
    finally:
        m.close()
    m = engine.Model(ctx, "logistic", [{"x": rng.normal(size=(20, 5)), "y": rng.integers(0, 2, 20)}])
    try:
        with pytest.raises(StarkHipError, match="S = 1025") as e:
            m.loo(np.zeros((1025, 6)), 0)
        assert e.value.code == -1
        q, tot = np.zeros((4, 6)), np.zeros(8)
        fn = _lib.load().stk_loo
        for args, word in (((m._h, 0, q.ctypes.data, 0, None, tot.ctypes.data), "S = 0"),
                           ((m._h, 0, q.ctypes.data, 4, None, None), "both NULL"),
                           ((m._h, 0, None, 4, None, tot.ctypes.data), "q is NULL")):
            assert fn(*args) == -1
            msg = _lib.load().stk_last_error().decode()
            assert word in msg and ("logistic" in msg or "d = 5" in msg), msg
        assert np.isfinite(m.loo(q, 0)).all()                            # the model still works
    finally:
        m.close()


# ---------------------------------------------------------------- the driver
PARTS = (200, 333, 64)


def _driver(rows):
    import os
    from conftest import ROOT
    from stark_amd import stark
    from stark_amd.rdd import LocalContext, LocalRDD

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": 5, "x": a[:, :5], "y": a[:, 5].astype(np.int64)}

    cuts = np.concatenate([[0], np.cumsum(PARTS)])
    rdd = LocalRDD([rows[cuts[i]:cuts[i + 1]] for i in range(len(PARTS))])     # three partitions of these sizes
    st = stark.Stark(LocalContext(), rdd, prep)
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "logistic.stan"))
    return st


def test_driver_loo(ctx):
    """Stark.loo over 3 logistic partitions (n = 200, 333, 64; d = 5; S = 256) equals the restatement over
    the union of rows; elpd_loo and elpd_waic of the same draws differ by less than their se (a sanity
    check, not a bar)."""
    from stark_amd import engine
    from stark_amd import rdd as _rdd
    n, d, S = sum(PARTS), 5, 256
    rng, X, y, truth = make_data("logistic", n, d)
    rows = [tuple(X[i]) + (int(y[i]),) for i in range(n)]
    st = _driver(rows)
    assert [len(p) for p in _rdd.partitions_of(st.rdd)] == list(PARTS)
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        _, _, H = m.hessian(0, truth)
    finally:
        m.close()
    sd = np.sqrt(np.diag(np.linalg.inv(-H)))
    Q = truth[None, :] + rng.normal(size=(S, d + 1)) * sd[None, :]
    samples = np.vstack([Q.T, np.zeros((1, S))])                       # P x S with an lp__ row
    ref, kbar, rtot, tscale = ref_loo("logistic", X, y, Q)
    out = st.loo(samples)
    assert out["partition_totals"].shape == (3, 8) and out["n"] == n
    assert [int(v) for v in out["partition_totals"][:, 0]] == list(PARTS)
    for key, j in (("lppd", 1), ("p_loo", 2), ("elpd_loo", 3)):
        assert abs(out[key] - rtot[j]) <= BAR * tscale[j], (key, out[key], rtot[j])
    assert out["looic"] == -2 * out["elpd_loo"] and out["n_non_finite"] == 0
    assert out["n_k_gt_0.5"] == rtot[5] and out["n_k_gt_0.7"] == rtot[6]
    e = ref["elpd_loo"].astype(L)
    se = float(np.sqrt(n / L(n - 1) * ((e * e).sum() - e.sum() ** 2 / n)))
    assert abs(out["se"] - se) <= 1e-8 * se
    w = st.waic(samples)
    print(f"elpd_loo {out['elpd_loo']:.6f} (se {out['se']:.3f})  elpd_waic {w['elpd_waic']:.6f} (se {w['se']:.3f})")
    assert abs(out["elpd_loo"] - w["elpd_waic"]) < min(out["se"], w["se"])
    with pytest.raises(ValueError, match="1024"):
        st.loo(np.zeros((d + 2, 1025)))
