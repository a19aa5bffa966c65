"""Host side of the weighted-likelihood bootstrap: the weights' host twin (stk_boot_weights_host, compiled from
csrc/boot_math.h, the header the kernel uses) against an independent numpy restatement, the Poisson
thresholds, the weights' distribution, engine.bootstrap's iteration on a numpy stand-in model, and the
argument errors of the host entry points.  No GPU.

The restatement (tests/boot_ref.py): Philox4x32-10 (engine.philox_words) at the counter
{row >> 4, (row >> 36) << 2 | row & 3, stream << 12 | b, 0x22}, the four 32-bit words in the order first
output low, high, second output low, high, word (row >> 2) & 3; poisson: the number of thresholds
floor(2^32 cdf_k) <= word, the thresholds recomputed in 60-digit decimal; exponential: -log((word + 1/2) 2^-32).
"""
import warnings

import numpy as np
import pytest

import boot_ref as br

L = np.longdouble
ROWS = np.array([0, 1, 2, 3, 4, 5, 14, 15, 16, 17, 62, 63, 64, 65, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 36 - 1,
                 2 ** 36, 2 ** 36 + 1], np.int64)
REPS = (0, 3, 4, 15, 16, 4095)
STREAMS = (0, 1, 7, 2 ** 20 - 1)


@pytest.mark.parametrize("kind", ("poisson", "exponential"))
def test_twin_matches_the_numpy_restatement(kind):
    """Rows around 0, 15/16, 63/64, 2^32 and 2^36, replicates 0, 3, 4, 15, 16, 4095, four streams, two seeds:
    poisson bit for bit, exponential within 4 ulp (two correctly rounded-ish logs of the same argument)."""
    from stark_amd import engine
    for seed in (0, 0x9E3779B97F4A7C15):
        for stream in STREAMS:
            ref = br.weights_np(seed, stream, ROWS, REPS, kind)
            got = np.empty_like(ref)
            for i, r in enumerate(ROWS):
                for j, b in enumerate(REPS):
                    got[i, j] = engine.boot_weights(seed, stream, int(r), 1, b, 1, kind)[0, 0]
            if kind == "poisson":
                assert np.array_equal(got, ref), (seed, stream)
            else:
                assert np.all(np.abs(got - ref) <= 4 * np.spacing(np.abs(ref))), (seed, stream)
    # a block call is the single calls: out[r - row0][b - rep0]
    blk = engine.boot_weights(5, 3, 60, 10, 14, 4, kind)
    assert blk.shape == (10, 4)
    ref = br.weights_np(5, 3, np.arange(60, 70), np.arange(14, 18), kind)
    assert np.array_equal(blk, ref) if kind == "poisson" else np.all(np.abs(blk - ref) <= 4 * np.spacing(ref))


def test_rows_of_a_tile_share_one_philox_call():
    """Rows lh, lh + 4, lh + 8, lh + 12 of a tile that starts at a multiple of 16 are the four words of ONE
    counter: the restated words of those rows, taken as a set per counter, are distinct outputs of one call."""
    from stark_amd import engine
    u = np.uint64
    for base in (0, 16, 2 ** 36 + 32):
        for lh in range(4):
            rows = np.array([base + lh + 4 * k for k in range(4)], np.int64)
            w = br.words_np(11, 2, rows, [5])[:, 0]
            ra, rb = engine.philox_words(11, u(base >> 4), u(((base >> 36) << 2) | lh), u((2 << 12) | 5), u(0x22))
            assert [int(v) for v in w] == [int(ra) & 0xFFFFFFFF, int(ra) >> 32, int(rb) & 0xFFFFFFFF, int(rb) >> 32]


def test_poisson_thresholds():
    from stark_amd import engine
    T = engine.boot_poisson_thresholds()
    assert T.dtype == np.uint32 and T.shape == (13,)
    Ti = [int(v) for v in T]
    assert all(a < b for a, b in zip(Ti, Ti[1:]))
    ref, cdf = br.thresholds_ref()
    assert Ti == ref
    for t, c in zip(Ti, cdf):
        assert abs(L(t) - L(2) ** 32 * L(str(c))) <= 1


@pytest.mark.parametrize("kind", ("poisson", "exponential"))
def test_weights_have_mean_one(kind):
    """10^6 weights (62500 rows x 16 replicates): Poisson(1) and Exp(1) both have variance 1, so the mean's sd
    is 1e-3 and the bar 5 of them."""
    from stark_amd import engine
    w = engine.boot_weights(20240, 1, 0, 62500, 0, 16, kind)
    assert w.shape == (62500, 16) and np.isfinite(w).all() and w.min() >= 0
    assert abs(w.mean() - 1.0) <= 5 / np.sqrt(1e6), w.mean()
    if kind == "poisson":
        assert np.array_equal(w, np.round(w)) and w.max() <= 13
    else:
        assert 0 < w.min() and w.max() <= 22.9


SOLVER_SHAPES = ((257, 3), (1030, 16))


@pytest.mark.parametrize("n,d", SOLVER_SHAPES)
@pytest.mark.parametrize("kind", ("poisson", "exponential"))
@pytest.mark.parametrize("family", br.FAMILIES)
def test_solver_reaches_the_newton_solution(family, kind, n, d):
    """engine.bootstrap on the numpy stand-in: every one of 20 replicates (a tile and a tail) converges and ends
    within 1e-7 sd of a full Newton solve on the same twin weights -- ten times the stopping tolerance."""
    from stark_amd import engine
    X, y, truth = br.make_data(family, n, d, 100 + n + d)
    shards = [{"x": X, "y": y}]
    mode, cov = br.newton(family, shards, None, truth)
    model = br.NumpyModel(family, shards)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = engine.bootstrap(model, 20, kind=kind, seed=3, fit=(mode, cov))
    assert res["converged"].all() and res["iterations"].max() <= 60
    assert res["estimates"].shape == (20, mode.size) and np.isfinite(res["lp"]).all()
    ref = br.newton_replicates(family, shards, [0], 20, kind, 3, mode)
    sd = np.sqrt(np.diag(cov))
    err = np.abs(res["estimates"] - ref) / sd
    print(f"MAXERR solver {family} {kind} n={n} d={d}: {err.max() / 1e-7:.3g} bars, "
          f"iterations {res['iterations'].min()}..{res['iterations'].max()}")
    assert err.max() <= 1e-7
    W = engine.boot_weights(3, 0, 0, n, 0, 20, kind)
    assert np.allclose(res["wsum"], W.sum(axis=0), rtol=1e-13)


def test_solver_marks_a_non_finite_replicate():
    from stark_amd import engine
    X, y, truth = br.make_data("logistic", 257, 3, 5)
    shards = [{"x": X[:130], "y": y[:130]}, {"x": X[130:], "y": y[130:]}]
    mode, cov = br.newton("logistic", shards, None, truth)
    clean = engine.bootstrap(br.NumpyModel("logistic", shards), 18, seed=1, fit=(mode, cov), streams=[4, 9])
    with pytest.warns(RuntimeWarning, match="1 of 18 replicates") as rec:
        res = engine.bootstrap(br.NumpyModel("logistic", shards, poison=[5]), 18, seed=1, fit=(mode, cov), streams=[4, 9])
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert not res["converged"][5] and np.isnan(res["estimates"][5]).all() and np.isnan(res["lp"][5])
    keep = np.arange(18) != 5
    assert res["converged"][keep].all()
    assert np.array_equal(res["estimates"][keep], clean["estimates"][keep])
    # combine= replaces the shard-order sum
    seen = []

    def combine(blocks):
        seen.append(blocks.shape)
        return blocks[0] + blocks[1]

    via = engine.bootstrap(br.NumpyModel("logistic", shards), 18, seed=1, fit=(mode, cov), streams=[4, 9], combine=combine)
    assert seen and all(s == (2, 16, 6) or s == (2, 2, 6) for s in seen)
    assert np.array_equal(via["estimates"], clean["estimates"])


def test_argument_errors():
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    info = engine.boot_launch(1030, 16)
    assert info["T"] == 16 and info["waves"] == 4 and info["G"] >= 1
    assert info["ws_bytes_per_shard"] == 8 * 16 * (16 + 3) * info["G"]
    assert engine.boot_launch(10 ** 9, 100)["G"] == engine.boot_launch(10 ** 9, 3)["G"]      # a function of n alone
    with pytest.raises(StarkHipError, match="d = 129"):
        engine.boot_launch(100, 129)
    with pytest.raises(StarkHipError, match="n_rows >= 1"):
        engine.boot_launch(0, 3)
    with pytest.raises(StarkHipError, match="kind = 2"):
        engine.boot_weights(0, 0, 0, 4, 0, 4, 2)
    with pytest.raises(ValueError, match="kind"):
        engine.boot_weights(0, 0, 0, 4, 0, 4, "gamma")
    with pytest.raises(StarkHipError, match="R = 0"):
        engine.boot_weights(0, 0, 0, 4, 0, 0, "poisson")
    with pytest.raises(StarkHipError, match="4097"):
        engine.boot_weights(0, 0, 0, 4, 4090, 7, "poisson")
    with pytest.raises(StarkHipError, match=f"stream = {2 ** 20}"):
        engine.boot_weights(0, 2 ** 20, 0, 4, 0, 4, "poisson")
    with pytest.raises(StarkHipError, match="row0 = -1"):
        engine.boot_weights(0, 0, -1, 4, 0, 4, "poisson")
    for B in (0, 4097):
        with pytest.raises(ValueError, match="1 <= B <= 4096"):
            engine.bootstrap(None, B)
