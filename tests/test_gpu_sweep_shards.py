"""The regression sweeps launched as a sampling run launches them -- several shards per grid,
groups of unequal n starting at shard0 > 0, a partial-sum stride Gs above a group's own G, idle
shards skipped by req_step -- against the CPU oracle (Model.log_density_grad_shards is the hook;
test_gpu_kernels.py covers the one-shard launches)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL_LP = 1e-10   # the bars of test_gpu_kernels.py::test_regression_lpgrad

# rows per shard: five groups of consecutive equal n, shard0 = 0, 2, 3, 4, 5.  Chunks per shard
# (stk_sweep_plan; pinned by test_host_sweep_launch.py): G = 3, 1, 3, 1, 2 for v1 at T = 64, v2, v3 (ceil(ceil(n / 64) / 8)) and
# k_sweep16, more for v1's smaller tiles, 6, 1, 6, 1, 3 for the 64-chain GEMM passes -- so every
# variant runs groups whose own G is below the partial-sum stride Gs = max G.
ROWS = [1500, 1500, 77, 1500, 1, 600]

SHAPES = ([(d, 8) for d in (4, 5, 100, 128, 129, 300, 700, 1024)]     # v2; v1 at T = 64 odd, 32, 16, 8; largest d
          + [(d, 4) for d in (20, 50, 100, 120, 33)]                  # v3 generic, k_sweep3<.., 25, 5>, <.., 50, 3>, v2, v1
          + [(100, 1), (100, 2)]
          + [(d, 16) for d in (4, 33, 100, 113, 128)]                 # k_sweep16
          + [(d, 64) for d in (5, 17, 100, 300)])                     # k_qt_swizzle + k_gemm_fwd / k_gemm_bwd


def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1.0)


def _grouped_case(orc, family, d, C, rows=ROWS, **prior):
    """Shards of `rows` rows from one generator (the recipe of test_regression_lpgrad, its large-|eta|
    rows at the head of every shard), the oracle model of each, and C points per shard."""
    rng = np.random.default_rng(1000 * d + C)
    N = sum(rows)
    off = np.concatenate([[0], np.cumsum(rows)])
    X = rng.uniform(-1.7, 1.7, (N, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    if family == "logistic":
        eta = X @ beta
        for s, n in enumerate(rows):
            eta[off[s]: off[s] + max(1, n // 50)] *= 80.0     # the +-20 cutoff branches
        y = (rng.uniform(size=N) < 1 / (1 + np.exp(-eta))).astype(np.int32)
        fam, D = orc.FAM_LOGREG, d + 1
    else:
        y = 0.3 + X @ beta + rng.normal(size=N)
        fam, D = orc.FAM_LINREG, d + 2
    shards = [{"x": X[off[s]: off[s + 1]], "y": y[off[s]: off[s + 1]]} for s in range(len(rows))]
    oms = [orc.Model(fam, X=sh["x"], y=sh["y"], **prior) for sh in shards]
    q = rng.normal(0, 0.2, (len(rows), C, D))
    if family == "logistic":
        q[:, 0, 1:] = beta * 40          # large |eta| rows
    elif C >= 2:
        q[:, C - 2, d + 1] = -6.0        # log sigma: exp(-u) scales every term
        q[:, C - 1, d + 1] = 6.0
    else:
        q[:, 0, d + 1] = np.where(np.arange(len(rows)) % 2 == 0, -6.0, 6.0)
    return shards, oms, q


def _check_against_oracle(oms, q, lp, g, tag):
    """Prints the largest errors in units of the bars, then asserts the bars."""
    elp, eg = 0.0, 0.0
    ref = []
    for s, om in enumerate(oms):
        for c in range(q.shape[1]):
            olp, og = om.lpgrad(q[s, c])
            ref.append((s, c, olp, og))
            elp = max(elp, float(_rel(lp[s, c], olp)))
            bar = np.maximum(np.abs(og), 1e-3 * (np.abs(og).max() + 1.0))
            eg = max(eg, float((np.abs(g[s, c] - og) / bar).max()))
    print(f"MAXERR {tag} lp_rel={elp:.3e} grad_over_scale={eg:.3e}")
    for s, c, olp, og in ref:
        assert _rel(lp[s, c], olp) < RTOL_LP, (s, c, lp[s, c], olp)
        scale = np.abs(og).max() + 1.0
        assert np.all(np.abs(g[s, c] - og) <= RTOL_LP * np.maximum(np.abs(og), scale * 1e-3)), \
            (s, c, np.abs(g[s, c] - og).max())


@pytest.mark.parametrize("d,C", SHAPES)
@pytest.mark.parametrize("family", ["logistic", "linear"])
def test_grouped_sweep_matches_oracle(ctx, orc, family, d, C):
    """lp and gradient of six shards in five equal-n groups through the sampler's grouped launches,
    vs the oracle at test_regression_lpgrad's bars; and, where the one-shard hook runs the same
    chain batch (every C but 8), bit-identical to it: the reduction order depends on (n, d, C)
    only, not on the grid a shard is launched in."""
    from stark_amd import engine
    shards, oms, q = _grouped_case(orc, family, d, C)
    m = engine.Model(ctx, family, shards)
    try:
        lp, g = m.log_density_grad_shards(q)
        assert np.isfinite(lp).all() and np.isfinite(g).all()
        _check_against_oracle(oms, q, lp, g, f"grouped[{family}-{d}-{C}]")
        if C != 8:
            for s in range(len(ROWS)):
                lp1, g1 = m.log_density_grad(s, q[s])
                np.testing.assert_array_equal(lp[s], lp1)
                np.testing.assert_array_equal(g[s], g1)
    finally:
        m.close()


@pytest.mark.parametrize("family,d,C", [("logistic", 20, 8), ("linear", 20, 16)])
def test_grouped_sweep_prior_matches_oracle(ctx, orc, family, d, C):
    """The normal(0, s) priors, added once per chain in k_sweep_reduce, on the grouped launches."""
    from stark_amd import engine
    shards, oms, q = _grouped_case(orc, family, d, C, prior_alpha=2.5, prior_beta=0.3)
    m = engine.Model(ctx, family, shards).set_prior(alpha=2.5, beta=0.3)
    try:
        lp, g = m.log_density_grad_shards(q)
        _check_against_oracle(oms, q, lp, g, f"grouped_prior[{family}-{d}-{C}]")
    finally:
        m.close()


def test_grouped_hook_rejects_what_the_sampler_rejects(ctx, orc):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    X = np.zeros((5, 129))
    m = engine.Model(ctx, "logistic", [{"x": X, "y": np.zeros(5, np.int32)}])
    for C in (3, 16):                     # no 3-chain sweep; k_sweep16 stops at d = 128
        with pytest.raises(StarkHipError, match="STK_E_ARG"):
            m.log_density_grad_shards(np.zeros((1, C, 130)))
    m.close()
    ms = engine.Model(ctx, "schools", [{"y": orc.SCHOOLS_Y, "sigma": orc.SCHOOLS_SIGMA}])
    with pytest.raises(StarkHipError, match="STK_E_ARG"):
        ms.log_density_grad_shards(np.zeros((1, 4, 10)))
    ms.close()


# ---------------------------------------------------------------- req_step gating
GATED_ROWS = [900, 900, 130]
# (family, d, C, eps).  eps: 0.05 logistic / 0.02 linear; logistic (129, 8) at 0.1, where the
# oracle's longest trees are [15, 7, 15] leapfrogs per shard (at 0.05 every shard reaches 15, so
# no shard would idle); linear at 0.05 for the divergent exits (n_leapfrog 4, 5, 6 occur).
GATED = ([("logistic", d, C, 0.1 if (d, C) == (129, 8) else 0.05) for d, C in ((6, 8), (129, 8), (50, 4), (33, 16), (17, 64))]
         + [("linear", d, C, 0.02) for d, C in ((6, 8), (129, 8), (50, 4), (33, 16), (17, 64))]
         + [("linear", 6, 8, 0.05), ("linear", 17, 64, 0.05)])


@pytest.mark.parametrize("family,d,C,eps", GATED)
def test_transition_gated_shards_match_oracle(ctx, orc, family, d, C, eps):
    """One fixed-step transition of three shards (two of 900 rows in one launch, one of 130) whose
    trees end at different steps: a finished shard asks for no evaluation and every sweep kernel
    and k_sweep_reduce must skip it while the others go on.  Every chain vs the oracle's twin."""
    from stark_amd import engine
    rng = np.random.default_rng(1000 * d + C)
    N = sum(GATED_ROWS)
    off = np.concatenate([[0], np.cumsum(GATED_ROWS)])
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    X = rng.uniform(-1.7, 1.7, (N, d))
    if family == "logistic":
        y = (rng.uniform(size=N) < 1 / (1 + np.exp(-(0.2 + X @ beta)))).astype(np.int32)
        fam, D = orc.FAM_LOGREG, d + 1
    else:
        y = 0.3 + X @ beta + rng.normal(size=N)
        fam, D = orc.FAM_LINREG, d + 2
    shards = [{"x": X[off[s]: off[s + 1]], "y": y[off[s]: off[s + 1]]} for s in range(3)]
    q0 = np.random.default_rng(5).normal(0, 0.1, (C, D))
    kw = dict(seed=7, iteration=11, eps=eps, max_depth=4)
    want = [[orc.Model(fam, X=sh["x"], y=sh["y"]).transition(q0[c], gid=s * C + c, **kw) for c in range(C)]
            for s, sh in enumerate(shards)]
    # the case is what it is meant to be, by the oracle alone
    longest = [max(int(w[2][3]) for w in ws) for ws in want]
    assert len(set(longest)) > 1, longest                       # (i) some shard idles while another sweeps
    divergent = sum(int(w[2][4]) for ws in want for w in ws)
    if divergent == 0:                                          # (ii) the chains moved
        moved = sum(bool(np.any(w[0] != q0[c])) for ws in want for c, w in enumerate(ws))
        assert 4 * moved >= 3 * 3 * C, moved
    else:
        assert {4, 5, 6} & {int(w[2][3]) for ws in want for w in ws}
    m = engine.Model(ctx, family, shards)
    try:
        got = [m.transition(s, q0, **kw) for s in range(3)]
    finally:
        m.close()
    eq = max(float((np.abs(got[s][0][c] - want[s][c][0]) / (1e-10 + 1e-8 * np.abs(want[s][c][0]))).max())
             for s in range(3) for c in range(C))
    elp = max(abs(got[s][1][c] - want[s][c][1]) / max(1.0, abs(want[s][c][1])) for s in range(3) for c in range(C))
    print(f"MAXERR gated[{family}-{d}-{C}-{eps}] longest={longest} divergent={divergent} "
          f"q_over_bar={eq:.3e} lp_rel={elp:.3e}")
    for s in range(3):
        q, lp, st = got[s]
        for c in range(C):
            oq, olp, ost, _ = want[s][c]
            np.testing.assert_allclose(q[c], oq, rtol=1e-8, atol=1e-10, err_msg=f"shard {s} chain {c}")
            assert abs(lp[c] - olp) <= 1e-9 * max(1, abs(olp)), (s, c, lp[c], olp)
            assert st[c, 2] == ost[2] and st[c, 3] == ost[3] and st[c, 4] == ost[4], (s, c, st[c], ost)
            np.testing.assert_allclose(st[c, [0, 5]], ost[[0, 5]], rtol=1e-9, atol=1e-12)
