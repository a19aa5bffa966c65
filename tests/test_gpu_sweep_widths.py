"""Every width of the regression log-density sweeps.  Each sweep is a table of template instantiations
picked from d at launch (k_sweep16<FAM, KF = ceil(d / 4)>, k_sweep3's ring depth and DMA count, v1's tile
size and column passes, the 64-chain passes' column blocks), and within one instantiation d modulo the
tile width picks further runtime paths; the other sweep tests reach 13 of k_sweep16's 32 KF, three of
k_sweep3's seven DMA counts and one of its widths at two chains.

One case per (family, d): two shards of 1483 and 77 rows at 95 points each through
Model.log_density_grad_chains, i.e. the batches [64, 16, 8, 4, 2, 1] -- the two GEMM passes, k_sweep16
(k_sweep16w past d = 128) and the 8-, 4-, 2- and 1-chain VALU sweeps at that width in one call.  What the
planner makes of 1483 and 77 rows (three chunks of eight 64-row tiles, a last tile of 11 rows, a
partial-sum stride above the short shard's own G) and that WIDTHS holds both ends of every launch class
are asserted without a device in test_host_sweep_launch.py.

Logistic and linear: the recipe of test_gpu_sweep_shards._grouped_case against the oracle; Poisson:
test_gpu_poisson.make_data and its points against its longdouble restatement.  Bars: the project's 1e-10
(_check_against_oracle, check_bars), per batch, so a failure names the batch (the kernel) it sits in.  And
every batch equals Model.log_density_grad_shards on its own points bit for bit, as in
test_gpu_chain_batches.py."""
import numpy as np
import pytest

from test_gpu_chain_batches import _batches, _pmap, _single_launch_before
from test_gpu_poisson import check_bars, make_data, ref_lpgrad
from test_gpu_sweep_shards import _check_against_oracle, _grouped_case

pytestmark = pytest.mark.gpu

ROWS = [1483, 77]
POINTS = 95
PLAN = [64, 16, 8, 4, 2, 1]
KIND = {1: "k_sweep", 2: "k_sweep2", 3: "k_sweep3", 4: "k_sweep16", 5: "gemm64", 6: "k_sweep16w"}
FAMILIES = ("logistic", "linear", "poisson")

NARROW = list(range(1, 129))
# both parities on each side of v1's T = 32 | 16 | 8 switches (256 | 257, 512 | 513), of its 3 | 4 column
# passes (768 | 769), of k_gemm_bwd<256>'s 1 .. 4 column blocks, and the first and last widths
PAST = [129, 130, 255, 256, 257, 258, 511, 512, 513, 514, 767, 768, 769, 770, 1023, 1024]
# both parities on each side of every width at which the LD a kernel is handed changes past 128 columns:
# v1's padded LDS row stride (the next value = 8, 16, 0 mod 32 at T = 32, 16, 8) and k_sweep16w's waves
# per block (a multiple of 128; 640 and 896 are v1 edges too)
LD_EDGES = sorted({e + k for e in [*range(136, 256, 32), *range(272, 512, 32), 384, *range(544, 1024, 32)]
                   for k in (-1, 0, 1, 2)} - set(PAST))
WIDTHS = NARROW + sorted(PAST + LD_EDGES)
CASES = [(fam, d) for fam in FAMILIES for d in WIDTHS]


def _errors(lp, g, olp, og):
    """(lp error over max(|lp|, 1), largest gradient error over max(|g_j|, 1e-3 (max |g| + 1))): the two
    figures of _check_against_oracle's MAXERR line, for references held as arrays."""
    elp = float(np.max(np.abs(lp - olp) / np.maximum(np.abs(olp), 1.0)))
    bar = np.maximum(np.abs(og), 1e-3 * (np.abs(og).max(axis=-1, keepdims=True) + 1.0))
    return elp, float(np.max(np.abs(g - og) / bar))


class _Ref:
    """An oracle model's lpgrad at the case's points: computed once, on 8 threads, served by point."""

    def __init__(self, om, q):
        self._at = dict(zip((p.tobytes() for p in q), _pmap(om.lpgrad, list(q))))

    def lpgrad(self, p):
        return self._at[np.ascontiguousarray(p).tobytes()]


def _poisson_case(d):
    """The shards, points and longdouble reference (lp, grad per shard) of test_poisson_lpgrad's recipe."""
    shards, q, ref = [], [], []
    for n in ROWS:
        rng, X, y, beta = make_data(n, d)
        qs = rng.normal(0, 0.2, (POINTS, d + 1))
        qs[0] = np.concatenate([[0.3], 3 * beta])
        qs[1, 1:] = 12 * beta                       # |eta| up to ~45
        parts = _pmap(lambda c: ref_lpgrad(X, y, qs[c:c + 12]), range(0, POINTS, 12))
        olp = np.concatenate([p[0] for p in parts])
        assert np.all(np.isfinite(olp.astype(np.float64))), (n, d)
        shards.append({"x": X, "y": y})
        q.append(qs)
        ref.append((olp, np.concatenate([p[1] for p in parts])))
    return shards, np.stack(q), ref


@pytest.mark.parametrize("family,d", CASES, ids=[f"{f}-{d}" for f, d in CASES])
def test_every_sweep_at_this_width(ctx, orc, family, d):
    from stark_amd import engine
    assert engine.chain_batches(POINTS, d) == PLAN
    if family == "poisson":
        shards, q, ref = _poisson_case(d)
    else:
        shards, oms, q = _grouped_case(orc, family, d, POINTS, rows=ROWS)
        refs = [_Ref(om, q[s]) for s, om in enumerate(oms)]
    m = engine.Model(ctx, family, shards)
    failed = []
    try:
        lp, g = m.log_density_grad_chains(q)
        assert lp.shape == (len(ROWS), POINTS) and np.isfinite(lp).all() and np.isfinite(g).all()
        for c0, B in _batches(POINTS, d):
            kind = KIND[engine.sweep_launch(ROWS[0], d, B)["kind"]]
            tag = f"widths[{family}-{d}-B{B}-{kind}]"
            cs = slice(c0, c0 + B)
            try:
                if family == "poisson":
                    errs = [_errors(lp[s, cs], g[s, cs], ref[s][0][cs].astype(np.float64), ref[s][1][cs].astype(np.float64))
                            for s in range(len(ROWS))]
                    print(f"MAXERR {tag} lp_rel={max(e[0] for e in errs):.3e} grad_over_scale={max(e[1] for e in errs):.3e}")
                    for s in range(len(ROWS)):
                        check_bars(lp[s, cs], g[s, cs], ref[s][0][cs], ref[s][1][cs], (tag, "shard", s))
                else:
                    _check_against_oracle(refs, q[:, cs], lp[:, cs], g[:, cs], tag)
            except AssertionError as e:
                failed.append(f"batch {c0}+{B} ({kind}) misses the bar: {e}")
            if not _single_launch_before(B, d):
                continue
            lp1, g1 = m.log_density_grad_shards(q[:, cs])
            if not (np.array_equal(lp[:, cs], lp1) and np.array_equal(g[:, cs], g1)):
                failed.append(f"batch {c0}+{B} ({kind}) differs from its single launch")
    finally:
        m.close()
    assert not failed, "\n".join(failed)
