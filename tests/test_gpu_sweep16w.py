"""k_sweep16w, the 16-chain fp64-MFMA sweep for 128 < d <= 1024 (sweep16w.hip): NW = ceil(d / 128)
waves share each 16-row sub-tile, wave w owns the column slab [w DW, w DW + DW), DW = 16 ceil(d / (16 NW)).
Reached through Model.log_density_grad_chains / the sampler at 16 chains per shard (the single-launch
hook log_density_grad_shards keeps refusing 16 points past d = 128)."""
import numpy as np
import pytest

from test_gpu_chain_batches import _gated_transition
from test_gpu_sweep_shards import ROWS, _check_against_oracle, _grouped_case

pytestmark = pytest.mark.gpu


def _shape(d):
    """(waves per block, slab width) of k_sweep16w at d; the kernel is instantiated per slab width."""
    nw = (d + 127) // 128
    return nw, 16 * ((d + 16 * nw - 1) // (16 * nw))


# the widths the issue names, plus both sides of every width at which the slab count (block shape) or
# the slab width (instantiation) changes
WIDTHS = sorted({129, 130, 131, 144, 191, 192, 255, 256, 257, 400, 511, 512, 513, 640, 767, 1000, 1022, 1023,
                 160, 161, 193, 224, 225, 288, 289, 336, 337, 384, 385, 448, 449, 560, 561, 641, 672, 673, 768, 769,
                 784, 785, 896, 897})
CASES = [(fam, d) for fam in ("logistic", "linear") for d in WIDTHS if not (fam == "linear" and d == 1023)]


def test_dispatch_shapes_are_covered():
    """Every (slab count, slab width) pair of 129 .. 1023 is in WIDTHS at its first and last width."""
    first, last = {}, {}
    for d in range(129, 1024):
        first.setdefault(_shape(d), d)
        last[_shape(d)] = d
    assert {s[1] for s in first} == {80, 96, 112, 128} and {s[0] for s in first} == set(range(2, 9))
    for s in first:
        assert first[s] in WIDTHS and last[s] in WIDTHS, (s, first[s], last[s])


@pytest.mark.parametrize("family,d", CASES, ids=[f"{f}-{d}-NW{_shape(d)[0]}-KF{_shape(d)[1] // 4}" for f, d in CASES])
def test_sweep16w_matches_oracle(ctx, orc, family, d):
    """Six shards in five equal-n groups at 16 points each vs the oracle, all outputs finite, and every
    shard bit-identical to its launch as a one-shard model (the chunks depend on (n, d) only)."""
    from stark_amd import engine
    assert engine.chain_batches(16, d) == [16]
    shards, oms, q = _grouped_case(orc, family, d, 16)
    m = engine.Model(ctx, family, shards)
    try:
        lp, g = m.log_density_grad_chains(q)
    finally:
        m.close()
    assert np.isfinite(lp).all() and np.isfinite(g).all()
    nw, dw = _shape(d)
    _check_against_oracle(oms, q, lp, g, f"sweep16w[{family}-{d}-NW{nw}-KF{dw // 4}]")
    for s in range(len(ROWS)):
        one = engine.Model(ctx, family, [shards[s]])
        try:
            lp1, g1 = one.log_density_grad_chains(q[s:s + 1])
        finally:
            one.close()
        np.testing.assert_array_equal(lp[s], lp1[0], err_msg=f"shard {s}")
        np.testing.assert_array_equal(g[s], g1[0], err_msg=f"shard {s}")


def test_sweep16w_log1p_flushes_twice_in_a_chunk(ctx, orc):
    """The in-loop log1p flush of the logistic lp (every SW_FLUSH = 32 sub-tiles of 16 rows).  A chunk
    flushes twice once it has 64 sub-tiles, i.e. more than 63 * 16 = 1008 rows; the kernel cuts a shard
    into G = min(512, ceil(ceil(n / 64) / 16)) chunks of whole 64-row tiles, so up to n = 1024 the shard
    is ONE chunk: the smallest such n is 1009."""
    from stark_amd import engine

    def flushes(n):
        nt = -(-n // 64)
        G = max(1, min(512, -(-nt // 16)))
        rows = max(min(n, 64 * (nt * (c + 1) // G)) - 64 * (nt * c // G) for c in range(G))
        return -(-rows // 16) // 32
    n = next(n for n in range(1, 5000) if flushes(n) >= 2)
    assert n == 1009
    d = 129
    rng = np.random.default_rng(1000 * d + 16)
    X = rng.uniform(-1.7, 1.7, (n, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    eta = X @ beta
    eta[: n // 50] *= 80.0
    y = (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.int32)
    q = rng.normal(0, 0.2, (1, 16, d + 1))
    q[:, 0, 1:] = beta * 40
    om = orc.Model(orc.FAM_LOGREG, X=X, y=y)
    m = engine.Model(ctx, "logistic", [{"x": X, "y": y}])
    try:
        lp, g = m.log_density_grad_chains(q)
    finally:
        m.close()
    _check_against_oracle([om], q, lp, g, f"sweep16w_flush[logistic-{d}-n{n}]")


def test_plan_uses_sixteen_past_128_columns():
    from stark_amd import engine
    assert engine.chain_batches(16, 200) == [16]
    assert engine.chain_batches(40, 300) == [16, 16, 8]


@pytest.mark.parametrize("d", [257, 640, 1023])
def test_sweep16w_transition_matches_oracle(ctx, orc, d):
    """One fixed-step transition of three shards at 16 chains each through the sampler, vs the oracle's
    twin (the recipe of the gated-shard tests; the oracle idles no shard at these widths)."""
    _gated_transition(ctx, orc, "logistic", d, 16, 0.05, "sweep16w_transition", need_idle=False)
