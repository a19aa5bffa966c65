"""Host side of Laplace sampling: the per-draw log-density sweep's launch info and refusals, the PSIS
weights (engine.psis_weights) against an np.longdouble restatement of csrc/psis_math.h's definitions,
and stratified resampling (engine.resample) on hand-computed weights.  No GPU.

The restatement, for S log ratios sorted ascending as v, mx = v[S-1], M = ceil(min(S / 5, 3 sqrt S)):
    no smoothing (khat = +inf) when M < 5 (S <= 20) or v[S-1] == v[S-M];
    ecut = exp(v[S-M-1] - mx), x_i = exp(v[S-M+i] - mx) - ecut, Mg = 30 + floor(sqrt M),
    theta_j = 1 / x_M + (1 - sqrt(Mg / (j - 1/2))) / (3 x*), x* = x at 1-based index floor(M / 4 + 1/2),
    k(theta) = mean_i log1p(-theta x_i), l_j = M (log(-theta_j / k_j) - k_j - 1), w_j = 1 / sum_i exp(l_i - l_j),
    theta^ = sum theta_j w_j, k = k(theta^), sigma = -k / theta^, khat = (k M + 5) / (M + 10),
    tail value j = log(sigma expm1(-khat log1p(-(j - 1/2) / M)) / khat + ecut),
    lw = min(., 0), normalised by its logsumexp, returned in the input's order.
"""
import numpy as np
import pytest

L = np.longdouble


def psis_ref(log_ratio):
    """(log_w, khat) in np.longdouble."""
    lr = np.asarray(log_ratio, np.float64).astype(L)
    S = lr.size
    order = np.argsort(np.asarray(log_ratio, np.float64), kind="stable")
    v = lr[order]
    mx = v[-1]
    b = 0
    while b * b < 9 * S:
        b += 1
    M = min((S + 4) // 5, b)
    lw = v - mx
    khat = L(np.inf)
    if M >= 5 and v[S - 1] - v[S - M] > 0:
        ecut = np.exp(v[S - M - 1] - mx)
        x = np.exp(v[S - M:] - mx) - ecut
        r = 0
        while (r + 1) * (r + 1) <= M:
            r += 1
        Mg = 30 + r
        xN, xstar = x[M - 1], x[(M + 2) // 4 - 1]
        th = np.array([1 / xN + (1 - np.sqrt(L(Mg) / (L(j) - L(0.5)))) / 3 / xstar for j in range(1, Mg + 1)], L)
        kb = np.array([np.log1p(-t * x).sum() / M for t in th], L)
        prof = M * (np.log(-th / kb) - kb - 1)
        w = np.array([1 / np.exp(prof - prof[i]).sum() for i in range(Mg)], L)
        that = (th * w).sum()
        k = np.log1p(-that * x).sum() / M
        sigma = -k / that
        kh = (k * M + 5) / (L(M) + 10)
        if np.isfinite(kh):
            khat = kh
            p = (np.arange(1, M + 1).astype(L) - L(0.5)) / M
            lw = lw.copy()
            lw[S - M:] = np.log(sigma * np.expm1(-kh * np.log1p(-p)) / kh + ecut)
    lw = np.minimum(lw, 0)
    m1 = lw.max()
    lw = lw - (m1 + np.log(np.exp(lw - m1).sum()))
    out = np.empty(S, L)
    out[order] = lw
    return out, khat


def philox_ref(seed, c0, c1, c2, c3):
    """Philox4x32-10 on python ints: the two 64-bit output words (csrc/philox.h)."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return (c1 << 32) | c0, (c3 << 32) | c2


def u53_ref(x):
    return ((x >> 11) + 0.5) * 2.0 ** -53


def test_launch_info_is_pure_and_its_geometry_ignores_S():
    from stark_amd import engine
    for n, d in ((1, 1), (64, 5), (65, 100), (1030, 128), (12_500_000, 100)):
        a = engine.logdens_launch(n, d, 1)
        assert a == engine.logdens_launch(n, d, 1)
        for S in (2, 16, 17, 1024, 16000):
            b = engine.logdens_launch(n, d, S)
            assert b == engine.logdens_launch(n, d, S)
            assert [b[k] for k in ("T", "G", "waves", "lds_bytes")] == [a[k] for k in ("T", "G", "waves", "lds_bytes")]
            tiles = (S + 15) // 16
            assert b["ws_bytes_per_shard"] == 8 * 16 * tiles * b["G"]
            assert b["image_bytes"] == engine.predictive_launch(n, d, S)["image_bytes"]
        assert a["T"] == 16 and a["waves"] == 4 and a["lds_bytes"] <= 160 * 1024
        assert 1 <= a["G"] <= 256 and a["G"] <= (n + 63) // 64
    assert engine.logdens_launch(12_500_000, 100, 1024)["G"] == 256


def test_refusals_name_the_value():
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    with pytest.raises(StarkHipError, match="d = 129"):
        engine.logdens_launch(100, 129, 16)
    with pytest.raises(StarkHipError, match="S = 0"):
        engine.logdens_launch(100, 5, 0)
    with pytest.raises(ValueError):
        engine.psis_weights([])
    with pytest.raises(ValueError):
        engine.psis_weights([0.0, np.nan])
    with pytest.raises(ValueError):
        engine.resample([0.0], 0, 1, 0)


@pytest.mark.gpu
def test_device_refusals_name_the_value(ctx):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    m = engine.Model(ctx, "schools", [{"y": np.arange(8.0), "sigma": np.ones(8)}])
    try:
        with pytest.raises(StarkHipError, match="schools"):
            m.log_density(np.zeros((3, m.D[0])), 0)
    finally:
        m.close()
    rng = np.random.default_rng(0)
    m = engine.Model(ctx, "linear", [{"x": rng.normal(size=(40, 129)), "y": rng.normal(size=40)}])
    try:
        with pytest.raises(StarkHipError, match="d = 129"):
            m.log_density(np.zeros((3, 131)), 0)
    finally:
        m.close()
    m = engine.Model(ctx, "linear", [{"x": rng.normal(size=(40, 3)), "y": rng.normal(size=40)}])
    try:
        lp = np.empty(1)
        rc = engine._lib.load().stk_log_density_draws(m._h, 0, np.zeros(5).ctypes.data, 0, lp.ctypes.data)
        assert rc == -1 and b"S = 0" in engine._lib.load().stk_last_error()
        with pytest.raises(StarkHipError, match="D = 131"):
            engine.laplace_draws(ctx, np.zeros(131), np.eye(131), 4, 1, 0)
        with pytest.raises(StarkHipError, match="S = 0"):
            engine.laplace_draws(ctx, np.zeros(3), np.eye(3), 0, 1, 0)
    finally:
        m.close()


def _check(lr, tag):
    from stark_amd import engine
    lw, kh = engine.psis_weights(lr)
    rw, rk = psis_ref(lr)
    err_w = float(np.abs(lw.astype(L) - rw).max())
    assert np.isfinite(kh) == np.isfinite(rk), tag
    err_k = float(abs(L(kh) - rk)) if np.isfinite(rk) else 0.0
    print(f"MAXERR psis_weights {tag} S={len(lr)} log_w={err_w:.3e} khat={err_k:.3e} khat_ref={float(rk):.4f}")
    assert err_w <= 1e-10 and err_k <= 1e-10, (tag, err_w, err_k)
    assert abs(float(np.exp(lw).sum()) - 1.0) < 1e-12
    return lw, kh


@pytest.mark.parametrize("S", (5, 20, 21, 100, 1024, 5000))
def test_psis_weights_match_the_longdouble_restatement(S):
    rng = np.random.default_rng(100 + S)
    for tag, lr in (("normal", rng.normal(0, 1.0, S)), ("heavy", -0.6 * np.log(rng.uniform(size=S))),
                    ("offset", 1234.5 + rng.normal(0, 0.05, S))):
        lw, kh = _check(lr, tag)
        assert np.isfinite(kh) == (S > 20)
        if S <= 20:                                       # not smoothed: the plain normalised ratios
            ref = lr.astype(L) - lr.max()
            ref = ref - np.log(np.exp(ref).sum())
            assert float(np.abs(lw - ref).max()) <= 1e-12


def test_psis_weights_constant_tail_and_one_dominant_ratio():
    rng = np.random.default_rng(7)
    S = 200                                               # M = 40
    lr = rng.normal(0, 1.0, S)
    lr[np.argsort(lr)[-40:]] = 3.25                       # the whole tail at one value: not smoothed
    lw, kh = _check(lr, "constant_tail")
    assert kh == np.inf
    ref = lr - 3.25
    assert float(np.abs(lw - (ref - np.log(np.exp(ref).sum()))).max()) <= 1e-12
    lw, kh = _check(np.zeros(100), "all_equal")
    assert kh == np.inf and np.allclose(lw, -np.log(100.0), rtol=0, atol=1e-14)
    lr = rng.normal(0, 0.3, 1000)
    lr[123] = 40.0                                        # one ratio e^40 above the rest
    lw, kh = _check(lr, "dominant")
    assert np.isfinite(kh) and kh > 0.7 and np.argmax(lw) == 123 and lw[123] <= 0.0


@pytest.mark.parametrize("k,lo,hi", ((0.3, 0.0, 0.6), (0.9, 0.45, 1.35)))
def test_khat_recovers_a_pareto_tail(k, lo, hi):
    """r = U^-k has a generalised Pareto tail of shape k.  Over seeds 0..19 at S = 5000 the longdouble
    restatement alone gave khat in [0.134, 0.548] (sd 0.117) around k = 0.3 and in [0.611, 1.208] (sd 0.173)
    around k = 0.9: the fit sees M = 213 tail values of a tail that is only asymptotically Pareto above
    the cut.  The intervals are k -+ 0.3 and k -+ 0.45, about 2.6 of those sds; the seed is fixed at 3,
    where the restatement gives 0.4067 and 1.0215."""
    from stark_amd import engine
    lr = -k * np.log(np.random.default_rng(3).uniform(size=5000))
    kh = engine.psis_weights(lr)[1]
    rk = float(psis_ref(lr)[1])
    print(f"MAXERR khat_pareto k={k} khat={kh:.4f} restatement={rk:.4f}")
    assert lo < rk < hi and lo < kh < hi and abs(kh - rk) <= 1e-10


def test_resample_on_hand_computed_weights():
    from stark_amd import engine
    # uniform weights, n = S: stratum k holds exactly draw k
    for S in (1, 7, 64):
        assert np.array_equal(engine.resample(np.full(S, -3.0), S, 11, 2), np.arange(S))
    # one draw holds all the weight
    lw = np.full(9, -np.inf)
    lw[4] = 0.0
    assert np.array_equal(engine.resample(lw, 13, 5, 0), np.full(13, 4))
    # weights 0.1, 0.2, 0.3, 0.4: running sums 0.1, 0.3, 0.6, 1.0 against u_k = (k + U_k) / 10
    w = np.array([0.1, 0.2, 0.3, 0.4])
    seed, stream, n = 77, 3, 10
    U = np.array([u53_ref(philox_ref(seed, stream, k, 0, 0x21)[0]) for k in range(n)])
    assert np.all((U > 0) & (U < 1)) and len(set(U)) == n
    u = (np.arange(n) + U) / n
    want = np.array([int(np.sum(np.cumsum(w) <= v)) for v in u])
    assert np.array_equal(want, [0, 1, 1, 2, 2, 2, 3, 3, 3, 3])          # strata of width 0.1: no boundary is crossed
    got = engine.resample(np.log(w), n, seed, stream)
    assert np.array_equal(got, want)
    assert np.array_equal(engine.resample(np.log(w) + 5.0, n, seed, stream), want)      # unnormalised: the same
    # n = 3 strata of width 1/3 straddle the boundaries: the uniforms decide, as restated
    u3 = (np.arange(3) + np.array([u53_ref(philox_ref(seed, stream, k, 0, 0x21)[0]) for k in range(3)])) / 3
    assert np.array_equal(engine.resample(np.log(w), 3, seed, stream), [int(np.sum(np.cumsum(w) <= v)) for v in u3])
    # another stream, other uniforms
    other = np.array([u53_ref(philox_ref(seed, stream + 1, k, 0, 0x21)[0]) for k in range(n)])
    assert not np.array_equal(other, U)
