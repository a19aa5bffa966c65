"""dense_e against the CPU oracle's dense metric (oracle/stark_oracle.c: dense_e_metric and
covar_adaptation restated with plain loops), at every edge of the blocked cold routines of
nuts.hip's dense instantiation:

  (a) fixed-step transitions under a general SPD metric (alpha - beta - log sigma cross terms),
      stk_transition_dense vs orc_transition_dense, at the D where dense_backsolve_cold gains a
      block / a panel chunk, dense_matvec_cold<16> its second group of 8 chunks, and NCH changes;
  (b) the window's linear algebra (dense_window_cold's Welford update, dense_cholesky_cold):
      M^-1 against covar_adaptation's formula on the run's own draws, and the factor read back
      through Sampler.metric_factor() against Higham's backward-error bound for Cholesky;
  (c) adaptive dense runs: one tracked transition by transition by run_chain(metric="dense_e")
      (init_stepsize and the dual-averaging restart under a dense metric), the others replayed
      transition by transition after warmup.

Bars (those of test_gpu_dense_metric.py's _check_rows): q rtol 1e-8 / atol 1e-10, lp 1e-9
relative, treedepth / n_leapfrog / divergent equal, accept_stat and energy rtol 1e-9 / atol 1e-12.
A replay at these bars means something only where the oracle replays ITSELF from starts perturbed
by 1e-13 relative (oracle.self_replay): every case asserts that, by the oracle alone, first."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _check_rows(orc, tag, rows):
    """rows: (where, q, lp, stats, want q, want lp, want stats).  Prints the largest errors in units
    of the bars, then asserts every bar on every row."""
    eq = max(orc.over_bar(r[1], r[4], 1e-8, 1e-10) for r in rows)
    elp = max(orc.over_bar(r[2], r[5], 0.0, 1e-9 * max(1.0, abs(r[5]))) for r in rows)
    est = max(orc.over_bar(r[3][[0, 5]], r[6][[0, 5]], 1e-9, 1e-12) for r in rows)
    flips = sum(int(not np.array_equal(r[3][2:5], r[6][2:5])) for r in rows)
    print(f"MAXERR {tag} transitions={len(rows)} flipped={flips} q_over_bar={eq:.3e} lp_over_bar={elp:.3e} "
          f"stat_over_bar={est:.3e}")
    for where, q, lp, st, oq, olp, ost in rows:
        assert st[2] == ost[2] and st[3] == ost[3] and st[4] == ost[4], (where, st, ost)
        np.testing.assert_allclose(q, oq, rtol=1e-8, atol=1e-10, err_msg=str(where))
        assert abs(lp - olp) <= 1e-9 * max(1.0, abs(olp)), (where, lp, olp)
        np.testing.assert_allclose(st[[0, 5]], ost[[0, 5]], rtol=1e-9, atol=1e-12, err_msg=str(where))


def _pmap(fn, items):
    """fn over items on 8 threads, in order: the oracle's C calls are independent and release the GIL."""
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(fn, items))


def _nch_for(D):
    return 1 if D <= 64 else 2 if D <= 128 else 4 if D <= 256 else 16


def _regression_rows(orc, family, d, rows, seed):
    """Shards of `rows` rows from one generator (that of test_gpu_nuts_widths.py's _regression_case)."""
    rng = np.random.default_rng(seed)
    N = sum(rows)
    X = rng.uniform(-1.7, 1.7, (N, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    if family == "logistic":
        y = (rng.uniform(size=N) < 1 / (1 + np.exp(-(0.2 + X @ beta)))).astype(np.int32)
        fam = orc.FAM_LOGREG
    else:
        y = 0.3 + X @ beta + rng.normal(size=N)
        fam = orc.FAM_LINREG
    cuts = np.cumsum([0] + list(rows))
    shards = [{"x": X[a:b], "y": y[a:b]} for a, b in zip(cuts[:-1], cuts[1:])]
    return shards, [orc.Model(fam, X=sh["x"], y=sh["y"]) for sh in shards]


# ================================================================ (a) fixed-step transitions, general metric
# (family, d, D, NCH, chains, small step, large step).  The steps come from a probe of the oracle alone
# (eps in 0.05 .. 2.0): at the small one the largest treedepth is >= 5, at the large one the mean
# accept_stat is < 0.95 while at least 3/4 of the chains move; the test asserts both, and the oracle's
# self-replay, before it touches the GPU.  16 chains where d <= 128, else 8; 4 at logistic D = 1024, whose
# every tree has 63 leapfrogs at both steps (the oracle takes 0.4 s per such transition).
FIXED = [
    ("logistic", 62, 63, 1, 16, 0.2, 2.0),       # a single backsolve block, nr = 63
    ("logistic", 63, 64, 1, 16, 0.2, 2.0),       # ... nr = 64
    ("logistic", 64, 65, 2, 16, 0.2, 2.0),       # first two-block backsolve: nr = 1, a one-row panel
    ("linear", 127, 129, 4, 16, 0.1, 0.7),       # first D of NCH 4, b0 = 128, nr = 1, log sigma cross terms
    ("logistic", 255, 256, 4, 8, 0.2, 1.6),      # last of NCH 4 (Dp = D)
    ("logistic", 256, 257, 16, 8, 0.2, 2.0),     # first of NCH 16: matvec KG = 8, lanes past D on column D - 1
    ("linear", 256, 258, 16, 8, 0.1, 0.55),
    ("logistic", 320, 321, 16, 8, 0.4, 1.7),     # b0 = 320: the panel's second column chunk, part of in[g] false
    ("linear", 320, 322, 16, 8, 0.1, 0.55),
    ("logistic", 511, 512, 16, 8, 0.4, 1.6),     # the matvec's second group of 8 chunks and its break
    ("logistic", 512, 513, 16, 8, 0.4, 1.4),
    ("linear", 513, 515, 16, 8, 0.1, 0.47),
    ("linear", 1021, 1023, 16, 8, 0.1, 0.35),    # D not a multiple of 8 under Dp = 1024
    ("logistic", 1023, 1024, 16, 4, 0.4, 1.0),   # the largest D the sampler takes
]


def _general_metric(D, n):
    """(G G^T / D + I / 2) / n, symmetric to the bit: every alpha - beta - log sigma cross term nonzero."""
    G = np.random.default_rng(D).normal(size=(D, D))
    M = (G @ G.T / D + 0.5 * np.eye(D)) / n
    return np.tril(M) + np.tril(M, -1).T


def _fixed_case(orc, family, d, D, chains, eps_small, eps_large):
    """The data, the metric and the oracle's transitions of one FIXED row, with the assertions that
    make the row what it is meant to be (by the oracle alone)."""
    n = 300 if D >= 1023 else 400
    (shard,), (om,) = _regression_rows(orc, family, d, [n], 1000 * d + (16 if d <= 128 else 8))
    assert om.D == D
    q0 = np.random.default_rng(5).normal(0, 0.1, (chains, D))
    Minv = _general_metric(D, n)
    assert Minv[0, 1] != 0 and Minv[1, 0] == Minv[0, 1]                           # alpha - beta
    if family == "linear":
        assert Minv[-1, 1] != 0 and Minv[-1, 0] != 0                              # log sigma - beta, - alpha
    kw = dict(seed=41, inv_metric=Minv, factor=orc.cholesky(Minv), max_depth=6)
    want = {eps: _pmap(lambda c: om.transition(q0[c], gid=c, iteration=6, eps=eps, **kw), range(chains))   # noqa: B023
            for eps in (eps_small, eps_large)}
    depths = sorted({int(w[2][2]) for ws in want.values() for w in ws})
    assert max(int(w[2][2]) for w in want[eps_small]) >= 5, depths
    accept = float(np.mean([w[2][0] for w in want[eps_large]]))
    moved = sum(bool(np.any(w[0] != q0[c])) for c, w in enumerate(want[eps_large]))
    assert accept < 0.95 and 4 * moved >= 3 * chains, (accept, moved, chains)
    flips, worst = 0, 0.0
    for eps, ws in want.items():
        f, w = orc.self_replay(om, [(q0[c], c, 6, eps) for c in range(chains)], want=ws, **kw)
        flips, worst = flips + f, max(worst, w)
    assert flips == 0 and worst <= 1e-2, (flips, worst)
    note = f"depths={depths} accept[{eps_large}]={accept:.3f} moved={moved}/{chains} self_replay={worst:.1e}"
    return shard, q0, Minv, want, note


@pytest.mark.parametrize("family,d,D,nch,chains,eps_small,eps_large", FIXED,
                         ids=[f"{r[0]}-{r[1]}-D{r[2]}-nch{r[3]}" for r in FIXED])
def test_general_dense_metric_fixed_step_matches_oracle(ctx, orc, family, d, D, nch, chains, eps_small, eps_large):
    from stark_amd import engine
    assert _nch_for(D) == nch
    shard, q0, Minv, want, note = _fixed_case(orc, family, d, D, chains, eps_small, eps_large)
    m = engine.Model(ctx, family, [shard])
    rows = []
    try:
        for eps, ws in want.items():
            q, lp, st = m.transition(0, q0, seed=41, iteration=6, eps=eps, inv_metric=Minv, max_depth=6)
            for c in range(chains):
                rows.append(((eps, c), q[c], lp[c], st[c], ws[c][0], ws[c][1], ws[c][2]))
    finally:
        m.close()
    assert len(rows) == 2 * chains
    _check_rows(orc, f"dense_general[{family}-{d}-D{D}-NCH{nch}] {note}", rows)


# ================================================================ (b) the window's linear algebra
def _covar_formula(draws):
    """Stan 2.19.1 covar_adaptation at a window's end, on the window's draws (n x D)."""
    n = draws.shape[0]
    cov = np.cov(draws.T, ddof=1)
    return (n / (n + 5.0)) * cov + 1e-3 * (5.0 / (n + 5.0)) * np.eye(draws.shape[1]), cov


def _assert_metric(got, draws, where):
    want, cov = _covar_formula(draws)
    sc = np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    over = float((np.abs(got - want) / (1e-8 * sc)).max())
    np.testing.assert_array_equal(got, got.T, err_msg=str(where))
    assert np.all(np.abs(got - want) <= 1e-8 * sc), (where, over)
    return over


def _lower_product(A):
    """The lower triangle of A A^T for a lower triangular long-double A, by blocks (the terms past
    min(i, j) are exact zeros and are left out; the upper triangle is not formed)."""
    D, bs = A.shape[0], 128
    out = np.zeros((D, D), np.longdouble)
    for i0 in range(0, D, bs):
        i1 = min(D, i0 + bs)
        for j0 in range(0, i1, bs):
            j1 = min(D, j0 + bs)
            out[i0:i1, j0:j1] = A[i0:i1, :j1] @ A[j0:j1, :j1].T
    return out


def _factor_ratio(L, M, where):
    """L against M = L L^T: lower triangular with an exactly zero upper triangle and a positive
    diagonal, and |L L^T - M| <= gamma_(D+1) |L| |L^T| elementwise, gamma_k = k u / (1 - k u), u = 2^-53:
    the backward error of a Cholesky factorisation in any order of summation (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., Theorem 10.3), with no margin.  The products are formed
    in long double; both sides are symmetric, so the lower triangle is the whole statement.  Returns
    the largest ratio to the bound."""
    D = M.shape[0]
    assert L.shape == M.shape
    assert np.all(np.triu(L, 1) == 0.0), where
    assert np.all(np.diag(L) > 0.0), where
    Lx = L.astype(np.longdouble)
    resid = np.abs(_lower_product(Lx) - np.tril(M).astype(np.longdouble))
    ku = np.longdouble(D + 1) * np.longdouble(2.0) ** -53
    bound = ku / (1 - ku) * _lower_product(np.abs(Lx))
    lo = np.tril(np.ones((D, D), bool))
    assert np.all(bound[lo] > 0)
    ratio = float((resid[lo] / bound[lo]).max())
    assert np.all(resid[lo] <= bound[lo]), (where, ratio)
    return ratio


@pytest.mark.parametrize("D", [65, 130, 258, 515, 1024])
def test_dense_window_metric_and_factor(ctx, orc, D):
    """One window of 20 draws (num_warmup 40: buffers 10 / 10, window 20, draws 10..29) at the widths
    where dense_cholesky_cold's column scaling takes a second pass of 4 x 64 rows (D - k - 1 > 256),
    its trailing update and dense_window_cold's Welford update end in a partial group of 8 rows, and
    D is or is not a multiple of 8 and 64.  max_depth 3 bounds the run (a dense step is 1.7 ms at
    D = 1001); n = 20 < D makes the matrix singular but for the 2e-4 I of the formula, which is where
    a factorisation is worth checking."""
    from stark_amd import engine
    chains = 2
    if D == 1024:
        family, d, n = "logistic", 1023, 3000
    else:
        family, d, n = "linear", D - 2, 3 * D
    (shard,), _ = _regression_rows(orc, family, d, [n], 77 + D)
    init = np.random.default_rng(D).normal(0, 0.1, (chains, D))
    m = engine.Model(ctx, family, [shard])
    s = m.sampler(num_warmup=40, num_samples=2, chains=chains, seed=17, save_warmup=True, metric="dense_e",
                  max_depth=3, adapt_init_buffer=10, adapt_term_buffer=10, adapt_window=20, init=init)
    try:
        s.run()
        eps, im = s.adaptation()
        L = s.metric_factor()
        uq = s.unconstrained(0)
        info = s.info()
    finally:
        s.close()
        m.close()
    assert info["errors"] == 0 and info["done"] == chains
    assert im.shape == L.shape == (chains, D, D) and uq.shape == (chains, 42, D)
    over = max(_assert_metric(im[c], uq[c, 10:30], (D, c)) for c in range(chains))
    ratio = max(_factor_ratio(L[c], im[c], (D, c)) for c in range(chains))
    print(f"MAXERR dense_window[D={D}] chains={chains} n=20 metric_over_bar={over:.3e} factor_over_higham={ratio:.3e}")
    assert np.all(eps > 0) and np.all(np.isfinite(uq))


def test_dense_factor_after_each_window(ctx, orc):
    """D = 14 on the correlated linear data, default buffers at num_warmup 200: the factor after the
    first window (draws 75..99) and after the last (100..149), and the identity before any."""
    from stark_amd import engine
    rng = np.random.default_rng(5)
    X = np.sqrt(0.9) * rng.normal(size=(400, 1)) + np.sqrt(0.1) * rng.normal(size=(400, 12))
    y = 0.3 + X @ rng.normal(0, 1, 12) + rng.normal(size=400)
    chains, D = 4, 14
    m = engine.Model(ctx, "linear", [{"x": X, "y": y}])
    s = m.sampler(num_warmup=200, num_samples=10, chains=chains, seed=5, save_warmup=True, metric="dense_e")
    dg = m.sampler(num_warmup=20, num_samples=2, chains=2)
    try:
        np.testing.assert_array_equal(s.metric_factor(), np.broadcast_to(np.eye(D), (chains, D, D)))
        s.run(100)
        im1, L1 = s.adaptation()[1], s.metric_factor()
        s.run()
        im2, L2 = s.adaptation()[1], s.metric_factor()
        uq = s.unconstrained(0)
        info = s.info()
        with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
            dg.metric_factor()                                         # a diag_e sampler has no factor
    finally:
        s.close()
        dg.close()
        m.close()
    assert info["errors"] == 0 and info["done"] == chains
    over = max(max(_assert_metric(im1[c], uq[c, 75:100], (c, "w1")), _assert_metric(im2[c], uq[c, 100:150], (c, "w2")))
               for c in range(chains))
    ratio = max(max(_factor_ratio(L1[c], im1[c], (c, "w1")), _factor_ratio(L2[c], im2[c], (c, "w2")))
                for c in range(chains))
    assert np.any(L1 != L2)
    print(f"MAXERR dense_window[D=14] chains={chains} windows=2 metric_over_bar={over:.3e} "
          f"factor_over_higham={ratio:.3e}")


# ================================================================ (c) adaptive dense runs
def test_dense_adaptive_run_tracks_oracle(ctx, orc):
    """The data of test_gpu_nuts.py's test_adaptive_run_tracks_oracle (logistic, n = 500, d = 3; a
    well-conditioned posterior, so both implementations follow one path): 30 warmup transitions (the
    4 / 23 / 3 short-warmup split) + 20 draws under dense_e against run_chain(metric="dense_e") from
    the same seed -- init_stepsize under the unit and under the adapted dense metric, the window, the
    refactorisation and the dual-averaging restart.

    The seed is chosen by the oracle alone.  An adaptive run feeds every rounding difference back through
    accept_stat into the step size, so it amplifies them: the oracle's own run from the same start moved
    by 1e-15 relative (a few ulp, the size of the differences between two implementations) ends 1e-11 to
    1e-10 away at 8 of the 10 seeds 2024..2033.  At 2024, that test's seed, chain 1 ends 2.5e-7 away
    (1.1e-7 from 3e-16), and the GPU run 9.9e-8: no implementation holds 1e-8 there.  The first assertion
    is that precondition at a tenth of the bar; seed 2025 gives 1.2e-10 and 8.2e-12."""
    from stark_amd import engine
    rng = np.random.default_rng(31)
    n, d = 500, 3
    X = rng.uniform(-1.7, 1.7, (n, d))
    y = (rng.uniform(size=n) < 1 / (1 + np.exp(-(0.3 + X @ np.array([0.8, -0.4, 0.2]))))).astype(np.int32)
    om = orc.Model(orc.FAM_LOGREG, X=X, y=y)
    nw, ns, C, seed = 30, 20, 2, 2025
    kw = dict(num_warmup=nw, num_samples=ns, seed=seed, metric="dense_e")
    want = [om.run_chain(gid=c, **kw) for c in range(C)]
    amp = 0.0
    for c in range(C):
        init = np.array([-2.0 + 4.0 * orc.lib().orc_uniform(seed, c, 0, i, orc.TAG_INIT) for i in range(d + 1)])
        np.testing.assert_array_equal(om.run_chain(gid=c, init=init, **kw)["q"], want[c]["q"])
        for sg in (1.0, -1.0):
            moved = init * (1.0 + 1e-15 * sg * np.array([1.0, -1.0, 1.0, -1.0]))
            amp = max(amp, float(np.abs(om.run_chain(gid=c, init=moved, **kw)["q"] - want[c]["q"]).max()))
    assert amp <= 1e-9, amp
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    s = m.sampler(num_warmup=nw, num_samples=ns, chains=C, seed=seed, save_warmup=True, metric="dense_e")
    try:
        s.run()
        eps, im = s.adaptation()
        uq = s.unconstrained(0)
        _, st = s.draws(0)
        info = s.info()
    finally:
        s.close()
        m.close()
    assert info["errors"] == 0 and info["done"] == C
    worst = max(float(np.abs(uq[c] - want[c]["q"]).max()) for c in range(C))
    wm = max(orc.over_bar(im[c], want[c]["inv_metric"], 1e-8, 0.0) for c in range(C))
    we = max(orc.over_bar(eps[c], want[c]["stepsize"], 1e-8, 0.0) for c in range(C))
    print(f"MAXERR dense_track[logistic-3] transitions={C * (nw + ns)} q_abs={worst:.3e} metric_over_bar={wm:.3e} "
          f"stepsize_over_bar={we:.3e} oracle_own_amplification_of_1e-15={amp:.1e}")
    for c in range(C):
        o = want[c]
        assert np.abs(uq[c] - o["q"]).max(axis=1).max() < 1e-8
        np.testing.assert_allclose(st[c * ns:(c + 1) * ns, 1], o["stats"][nw:, 1], rtol=1e-8)
        np.testing.assert_array_equal(st[c * ns:(c + 1) * ns, 2:5], o["stats"][nw:, 2:5])
        np.testing.assert_allclose(eps[c], o["stepsize"], rtol=1e-8)
        np.testing.assert_allclose(im[c], o["inv_metric"], rtol=1e-8)
        assert np.abs(o["inv_metric"] - np.diag(np.diag(o["inv_metric"]))).max() > 0        # a dense matrix
        assert o["stepsize"] != 1.0


def _replay_precondition(orc, oms, chains, nw, ns, seed):
    """By the oracle alone: its own dense_e run of the first chain of every shard stays bounded, and its
    post-warmup transitions replay themselves (no flipped stat, at most 1e-2 of the bars)."""
    flips, worst = 0, 0.0
    for k, om in enumerate(oms):
        o = om.run_chain(num_warmup=nw, num_samples=ns, seed=seed, gid=k * chains, metric="dense_e")
        assert np.abs(o["q"]).max() < 10
        starts = [(o["q"][t - 1], k * chains, t, o["stats"][t, 1]) for t in range(nw, nw + ns)]
        f, w = orc.self_replay(om, starts, seed=seed, inv_metric=o["inv_metric"], factor=orc.cholesky(o["inv_metric"]))
        flips, worst = flips + f, max(worst, w)
    assert flips == 0 and worst <= 1e-2, (flips, worst)
    return worst


def _replay_dense_run(ctx, orc, tag, family, shards, oms, chains, nw, ns, seed):
    """A dense_e run of every shard; every post-warmup transition replayed by the oracle from the run's
    own previous draw, step size and adapted matrix."""
    from stark_amd import engine
    worst = _replay_precondition(orc, oms, chains, nw, ns, seed)
    m = engine.Model(ctx, family, shards)
    s = m.sampler(num_warmup=nw, num_samples=ns, chains=chains, seed=seed, save_warmup=True, metric="dense_e")
    try:
        s.run()
        eps, im = s.adaptation()
        L = s.metric_factor()
        out = [(s.draws(k), s.unconstrained(k)) for k in range(len(shards))]
        info = s.info()
    finally:
        s.close()
        m.close()
    assert info["errors"] == 0 and info["done"] == len(shards) * chains
    ratio = 0.0

    def chain_rows(kc):
        k, c = kc
        (d, st), uq = out[k]
        g = k * chains + c
        ch = orc.cholesky(im[g])
        rows = []
        for t in range(nw, nw + ns):
            i = c * ns + t - nw
            oq, olp, ost, _ = oms[k].transition(uq[c, t - 1], seed=seed, gid=g, iteration=t, eps=st[i, 1],
                                                inv_metric=im[g], factor=ch)
            rows.append(((k, c, t), uq[c, t], d[-1, i], st[i], oq, olp, ost))
        return rows

    for k, ((d, st), uq) in enumerate(out):
        for c in range(chains):
            g = k * chains + c
            ratio = max(ratio, _factor_ratio(L[g], im[g], (k, c)))
            assert np.all(st[c * ns:(c + 1) * ns, 1] == eps[g])
    rows = sum(_pmap(chain_rows, [(k, c) for k in range(len(shards)) for c in range(chains)]), [])
    assert len(rows) == len(shards) * chains * ns
    depths = sorted({int(r[6][2]) for r in rows})
    _check_rows(orc, f"dense_replay[{tag}] depths={depths} self_replay={worst:.1e} factor_over_higham={ratio:.3e}", rows)


def test_dense_adaptive_run_replays_on_oracle_correlated(ctx, orc):
    """The correlated linear data (D = 14), num_warmup 200 (windows of 25 and 50), 4 chains."""
    rng = np.random.default_rng(5)
    X = np.sqrt(0.9) * rng.normal(size=(400, 1)) + np.sqrt(0.1) * rng.normal(size=(400, 12))
    y = 0.3 + X @ rng.normal(0, 1, 12) + rng.normal(size=400)
    _replay_dense_run(ctx, orc, "linear-12-D14", "linear", [{"x": X, "y": y}], [orc.Model(orc.FAM_LINREG, X=X, y=y)],
                      4, 200, 20, 5)


@pytest.mark.parametrize("d,chains", [(100, 16), (64, 8)])
def test_dense_adaptive_run_replays_on_oracle_headline(ctx, orc, d, chains):
    """k_nuts_step<2, DENSE> at the headline width (logistic d = 100, D = 101, 16 chains) and at D = 65,
    on the two shards (1000 and 600 rows) of test_step_kernel_adaptive_run_replays_on_oracle;
    num_warmup 150 is one window of n = 25 < D draws."""
    shards, oms = _regression_rows(orc, "logistic", d, [1000, 600], 1000 * d + chains)
    assert _nch_for(d + 1) == 2
    _replay_dense_run(ctx, orc, f"logistic-{d}-D{d + 1}-{chains}", "logistic", shards, oms, chains, 150, 20, 91)
