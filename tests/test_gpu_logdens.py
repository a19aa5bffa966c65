"""The per-draw log-density sweep (stk_log_density_draws, logdens.hip) and the Laplace proposal generator
(stk_laplace_draws) against numpy restatements.

The density, with eta_is = alpha_s + x_i . beta_s (draw s, row i), is Stan's log_prob, propto, with the
Jacobian -- the lp of stk_log_density_grad:
    logistic  ll_i = min(z, 0) - log1p(exp(-|z|)), z = (2 y_i - 1) eta
    poisson   ll_i = y_i eta - exp(eta)                                    (no lgamma(y + 1))
    linear    ll_i = -u - (y_i - eta)^2 e^{-2u} / 2, Jacobian + u          (no log(2 pi) / 2)
    prior     - alpha^2 / (2 s_a^2) - |beta|^2 / (2 s_b^2) under stk_model_set_prior
restated in np.longdouble.  The bar is the project's density bar: 1e-10 of the scale, the scale being
sum_i |ll_i| plus the absolute prior and Jacobian terms.  Every case prints its largest error in units of
the bar as a MAXERR line.  The bit-level contract: lp of a draw depends on that draw and the shard alone.

The generator: xi_{s,j} = Box-Muller of Philox4x32-10 at {stream, s, j / 2, 0x20}, theta_s = mode + F xi_s,
log_q[s] = -sum xi^2 / 2; the bar is 1e-12 of max |theta - mode| for both outputs (the device's log, sin and
cos are within a few ulp of numpy's; this is the combine's flat bar).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 1e-10
FAMILIES = ("logistic", "poisson", "linear")
NS = (1, 15, 16, 17, 63, 64, 65, 257, 1030)
DS = (1, 3, 4, 5, 16, 17, 100, 128)
SS = (1, 15, 16, 17, 33, 100, 1025)
PRIOR = (2.5, 1.5)                   # sds of alpha and beta
L = np.longdouble
_cache = {}


def make_case(family, d):
    """1030 rows of X ~ U(-1.7, 1.7) (one all-zero), y from the family, 1025 draws near the truth, and the
    longdouble per-row log likelihood ll [1030, 1025]; computed once per (family, d) and left unchanged."""
    key = (family, d)
    if key in _cache:
        return _cache[key]
    n, S = max(NS), max(SS)
    rng = np.random.default_rng(7000 + 10 * d + FAMILIES.index(family))
    X = rng.uniform(-1.7, 1.7, (n, d))
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
    Q = truth[None, :] + rng.normal(0, 0.1, (S, truth.size))
    case = {"X": X, "y": y, "Q": Q, "ll": ref_ll(family, X, y, Q)}
    _cache.clear()                   # one case at a time: 8 MB of longdouble each
    _cache[key] = case
    return case


def ref_ll(family, X, y, Q):
    d = X.shape[1]
    Xl, Ql, yl = X.astype(L), np.asarray(Q).astype(L), np.asarray(y).astype(L)[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        eta = Ql[:, 0][None, :] + Xl @ Ql[:, 1:d + 1].T
        if family == "logistic":
            z = (2 * yl - 1) * eta
            return np.minimum(z, 0) - np.log1p(np.exp(-np.abs(z)))
        if family == "poisson":
            return yl * eta - np.exp(eta)
        u = Ql[:, -1][None, :]
        r = yl - eta
        return -u - L(0.5) * r * r * np.exp(-2 * u)


def ref_lp(family, ll, Q, d, prior):
    """(lp [S], scale [S]) of the rows in ll, in longdouble."""
    Ql = np.asarray(Q).astype(L)
    lp, scale = ll.sum(axis=0), np.abs(ll).sum(axis=0)
    if family == "linear":
        lp, scale = lp + Ql[:, -1], scale + np.abs(Ql[:, -1])
    if prior is not None:
        pa = Ql[:, 0] ** 2 / (2 * L(prior[0]) ** 2)
        pb = (Ql[:, 1:d + 1] ** 2).sum(axis=1) / (2 * L(prior[1]) ** 2)
        lp, scale = lp - pa - pb, scale + pa + pb
    return lp, scale


def shard_of(case, n):
    return {"x": np.ascontiguousarray(case["X"][:n]), "y": np.ascontiguousarray(case["y"][:n])}


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("family", FAMILIES)
def test_log_density_matches_the_restatement_and_the_gradient_hook(ctx, family, d):
    """Every n of NS (one model each, the first n rows) x every S of SS (the first S draws) x priors off and
    on, against the restatement; the first 17 draws also against log_density_grad's lp."""
    from stark_amd import engine
    case = make_case(family, d)
    worst, worst_hook = 0.0, 0.0
    for n in NS:
        m = engine.Model(ctx, family, [shard_of(case, n)])
        try:
            for prior in (None, PRIOR):
                m.set_prior(*(prior or (None, None)))
                rlp, scale = ref_lp(family, case["ll"][:n], case["Q"], d, prior)
                full = None
                for S in SS[::-1]:
                    lp = m.log_density(case["Q"][:S], 0)
                    assert lp.shape == (S,) and np.isfinite(lp).all()
                    err = float((np.abs(lp.astype(L) - rlp[:S]) / (BAR * scale[:S])).max())
                    worst = max(worst, err)
                    assert err <= 1.0, (family, n, d, S, prior, err)
                    if full is None:
                        full = lp
                    assert np.array_equal(lp, full[:S]), (family, n, d, S)      # the same bits at any S
                hook, _ = m.log_density_grad(0, case["Q"][:17])
                eh = float((np.abs(hook - full[:17]) / (BAR * scale[:17].astype(np.float64))).max())
                worst_hook = max(worst_hook, eh)
                assert eh <= 1.0, (family, n, d, prior, eh)
        finally:
            m.close()
    print(f"MAXERR logdens family={family} d={d} vs_restatement={worst:.3e} vs_log_density_grad={worst_hook:.3e}")


@pytest.mark.parametrize("family", FAMILIES)
def test_unequal_shards_in_one_grouped_launch(ctx, family):
    from stark_amd import engine
    d = 17
    case = make_case(family, d)
    ns = (257, 1, 1030, 17, 64)
    cuts = np.concatenate([[0], np.cumsum(ns)])
    X, y = np.tile(case["X"], (2, 1)), np.tile(case["y"], 2)
    ll = np.concatenate([case["ll"], case["ll"]])
    m = engine.Model(ctx, family, [{"x": np.ascontiguousarray(X[a:b]), "y": np.ascontiguousarray(y[a:b])}
                                   for a, b in zip(cuts[:-1], cuts[1:])])
    try:
        m.set_prior(*PRIOR)
        Q = case["Q"][:100]
        lp = m.log_density(Q)
        assert lp.shape == (len(ns), 100)
        worst = 0.0
        for s, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            rlp, scale = ref_lp(family, ll[a:b], case["Q"], d, PRIOR)
            worst = max(worst, float((np.abs(lp[s].astype(L) - rlp[:100]) / (BAR * scale[:100])).max()))
            assert np.array_equal(lp[s], m.log_density(Q, s)), s               # grouped = single, bit for bit
        print(f"MAXERR logdens_grouped family={family} vs_restatement={worst:.3e}")
        assert worst <= 1.0
    finally:
        m.close()


@pytest.mark.parametrize("family,n,d", (("logistic", 1030, 100), ("poisson", 257, 5), ("linear", 333, 16)))
def test_bit_level_contract(ctx, family, n, d):
    from stark_amd import engine
    case = make_case(family, d)
    m = engine.Model(ctx, family, [shard_of(case, n)])
    try:
        m.set_prior(*PRIOR)
        Q = case["Q"][:100]
        lp = m.log_density(Q, 0)
        assert np.array_equal(lp, m.log_density(Q, 0))                          # two identical runs
        perm = np.random.default_rng(5).permutation(100)
        assert np.array_equal(m.log_density(Q[perm], 0), lp[perm])              # any position, any companions
        for cut in (1, 16, 37):                                                 # S split over two calls
            assert np.array_equal(np.concatenate([m.log_density(Q[:cut], 0), m.log_density(Q[cut:], 0)]), lp)
        for s in (0, 15, 16, 99):                                               # alone
            assert m.log_density(Q[s:s + 1], 0)[0] == lp[s]
    finally:
        m.close()


def test_a_non_finite_draw_poisons_only_itself(ctx):
    from stark_amd import engine
    d = 5
    for family in FAMILIES:
        case = make_case(family, d)
        m = engine.Model(ctx, family, [shard_of(case, 257)])
        try:
            Q = case["Q"][:40].copy()
            clean = m.log_density(Q, 0)
            Q[7, 2] = np.nan
            Q[21, 0] = np.nan
            if family == "poisson":
                Q[16, 0] = 800.0                                               # exp(eta) overflows on every row
            lp = m.log_density(Q, 0)
            bad = [7, 21] + ([16] if family == "poisson" else [])
            assert not np.isfinite(lp[bad]).any(), lp[bad]
            assert np.isnan(lp[[7, 21]]).all()
            ok = np.setdiff1d(np.arange(40), bad)
            assert np.array_equal(lp[ok], clean[ok])
        finally:
            m.close()


# ---------------------------------------------------------------- the generator
def philox(seed, c0, c1, c2, c3):
    """Philox4x32-10 on uint64 arrays of 32-bit counters: the two 64-bit output words."""
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    c0, c1, c2, c3 = (np.array(np.broadcast_to(np.asarray(c, np.uint64), np.broadcast(c0, c1, c2, c3).shape))
                      for c in (c0, c1, c2, c3))
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return (c1 << s32) | c0, (c3 << s32) | c2


def ref_laplace_draws(mode, F, S, seed, stream):
    D = mode.size
    s = np.arange(S, dtype=np.uint64)[:, None]
    j = np.arange(D, dtype=np.uint64)[None, :]
    a, b = philox(seed, np.uint64(stream), s, j >> np.uint64(1), np.uint64(0x20))
    u1 = ((a >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = ((b >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    rad, th = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    xi = np.where((j & np.uint64(1)) == 1, rad * np.sin(th), rad * np.cos(th)).astype(L)
    return (mode.astype(L)[None, :] + xi @ F.astype(L).T), -L(0.5) * (xi * xi).sum(axis=1)


@pytest.mark.parametrize("S", (1, 17, 1000))
@pytest.mark.parametrize("D", (1, 2, 63, 64, 65, 130))
def test_laplace_draws_match_the_restatement(ctx, D, S):
    from stark_amd import engine
    rng = np.random.default_rng(100 * D + S)
    mode, F = rng.normal(0, 0.5, D), rng.normal(0, 1.0, (D, D))
    seed, stream = 0x1234_5678_9ABC_DEF0 + D, 7
    q, lq = engine.laplace_draws(ctx, mode, F, S, seed, stream)
    rq, rlq = ref_laplace_draws(mode, F, S, seed, stream)
    bar = 1e-12 * float(np.abs(rq - mode.astype(L)).max())
    eq, el = float(np.abs(q - rq).max()), float(np.abs(lq - rlq).max())
    print(f"MAXERR laplace_draws D={D} S={S} theta={eq / bar:.3e} log_q={el / bar:.3e} (units of the bar {bar:.3e})")
    assert eq <= bar and el <= bar
    q2, lq2 = engine.laplace_draws(ctx, mode, F, S, seed, stream + 1)
    assert not np.array_equal(q, q2) and not np.array_equal(lq, lq2)           # two streams differ
    q3, lq3 = engine.laplace_draws(ctx, mode, F, S + 5, seed, stream)           # the same stream in another call
    assert np.array_equal(q3[:S], q) and np.array_equal(lq3[:S], lq)


def test_device_buffers_give_the_host_path_bits(ctx):
    """q, lp, and the generator's four pointers as device memory (cuda tensors) through the C ABI."""
    import torch
    from stark_amd import _lib, engine
    case = make_case("logistic", 5)
    m = engine.Model(ctx, "logistic", [shard_of(case, 257), shard_of(case, 64)])
    try:
        Q = case["Q"][:33]
        host = m.log_density(Q)
        dev = torch.device("cuda", ctx.device)
        qd = torch.as_tensor(Q, device=dev).contiguous()
        lpd = torch.empty((2, 33), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        engine.check(_lib.load().stk_log_density_draws(m._h, -1, qd.data_ptr(), 33, lpd.data_ptr()))
        assert np.array_equal(lpd.cpu().numpy(), host)
        rng = np.random.default_rng(3)
        mode, F = rng.normal(size=6), rng.normal(size=(6, 6))
        hq, hl = engine.laplace_draws(ctx, mode, F, 40, 9, 2)
        md, Fd = torch.as_tensor(mode, device=dev), torch.as_tensor(F, device=dev).contiguous()
        oq, ol = torch.empty((40, 6), dtype=torch.float64, device=dev), torch.empty(40, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        engine.check(_lib.load().stk_laplace_draws(ctx._h, md.data_ptr(), Fd.data_ptr(), 6, 40, 9, 2, oq.data_ptr(),
                                                   ol.data_ptr()))
        assert np.array_equal(oq.cpu().numpy(), hq) and np.array_equal(ol.cpu().numpy(), hl)
    finally:
        m.close()
