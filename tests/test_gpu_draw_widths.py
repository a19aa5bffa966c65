"""Every (family, KF) instantiation of the draw-image sweeps and of the bootstrap sweep, run against the
restatements their own test files use.

k_logdens, k_predictive, k_loo (4 and 8 waves), k_yrep (with and without rows) and k_boot16 are compiled once
per family and per KF = ceil(d / 4), KF = 1 .. 32: 672 code objects (draw_dispatch in csrc/draw_forward.h,
BT_CASE in csrc/boot.hip).  A case here is one (family, KF); it runs the four widths d = 4 KF - 3 .. 4 KF --
every remainder of the column mask col < d -- and at each d all five sweeps on ONE model, so the 3 x 32 cases
execute every instantiation: both LOO block widths by the two S below, both ROWS values of k_yrep by the two
posterior_predict calls.

The shapes are the smallest at which the width-specific code can still go wrong:
    rows      n = 85: a 64-row group, then a group of one full 16-row tile and a ragged 5-row tile (waves 2
              and 3 get nothing).  The second group restages rows over the LDS area the slab ring just used;
              which of the two is larger depends on d.  Rows 16 and 80 of X are all zero.
    draws     S = 33: three draw tiles, both ring slots reused, the last tile with 1 live draw of 16.
    LOO       the first 33 rows (three tiles, two chunks) as a shard of their own, at S = 33 (tail length 7: the
              Pareto fit runs, 4 waves) and S = 257 (Sp = 512: 8 waves).
    boot      R = 17: two tiles of 16 replicates, the second with one live column; both kinds, priors set (the
              prior loop of the reduce runs to d).
What k_boot16's geometry (boot_geom, boot_pre, boot_lds_bytes_kf) switches on, and where the KF sweep reaches it:
    VREM      the last column tile goes to the VALU when REM <= 4: KF in {1, 5, 9, 13, 17, 21, 25, 29};
    PRE       the early slot release, KF <= 27: flips between KF = 27 and 28;
    both      KF = 29 is the only width with VREM and !PRE together;
    LDS       max(main, red) bytes: main = 512 d + 8704 grows with d, red = 8192 JT + 14336 with JT = ceil(KF / 4)
              in steps of 16 columns.  main overtakes red only for d > 16 JT + 11, which no d <= 128 reaches: the
              size is red's step function, and the slots of main end 5.5 to 13 KiB below it.
No bar is new: each sweep is held to the bar of its own file (1e-10 of the scale; khat by the measured bar of
test_gpu_loo.ref_loo; counts, replicates and the poisson wsum exactly).  Every case prints its largest error
per sweep, in units of the bar, as a MAXERR line.

The restatements assert things about their own inputs (ref_loo: no khat within 1e-6 of a threshold, float64 and
long double take the same branches; check_shard: no replicate within 1e-10 of a decision boundary).  A fixed
seed formula misses them at a handful of the 384 (family, d), so the data seed is searched: seed0 + attempt,
attempt = 0 .. 3, the first for which every precondition of every sweep holds, judged from the restatements and
the host twins alone.  A (family, d) that exhausts the four fails.
"""
import numpy as np
import pytest

import boot_ref as br
import ppc_ref
import test_gpu_boot as BT
import test_gpu_logdens as LD
import test_gpu_loo as LO
import test_gpu_ppc as PP
import test_gpu_predictive as PR

pytestmark = pytest.mark.gpu

FAMILIES = ("logistic", "poisson", "linear")
KFS = tuple(range(1, 33))
N, N_LOO, S, S_BIG, R = 85, 33, 33, 257, 17
ZERO_ROWS = (16, 80)                 # one in the LOO shard and the first group, one in the ragged tile
PRIOR = BT.PRIOR
KINDS = BT.KINDS
SEED_PPC, STREAM_PPC = 77, 7
SEED_BOOT, STREAM_BOOT = 11, 3
ATTEMPTS = 4
L = np.longdouble


def widths(kf):
    return range(4 * kf - 3, 4 * kf + 1)


def make_data(family, d, seed):
    """X ~ U(-1.7, 1.7) [85, d] with two all-zero rows, y from the family at a true point, 257 draws near it."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.7, 1.7, (N, d))
    X[list(ZERO_ROWS)] = 0.0
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    eta = 0.3 + X @ beta
    if family == "logistic":
        y = (rng.uniform(size=N) < 1 / (1 + np.exp(-eta))).astype(np.int32)
        truth = np.concatenate([[0.3], beta])
    elif family == "poisson":
        y = rng.poisson(np.exp(eta)).astype(np.int32)
        truth = np.concatenate([[0.3], beta])
    else:
        y = eta + 0.7 * rng.normal(size=N)
        truth = np.concatenate([[0.3], beta, [np.log(0.7)]])
    Q = np.ascontiguousarray(truth[None, :] + rng.normal(0, 0.1, (S_BIG, truth.size)))
    return X, y, Q


def references(family, d, seed):
    """Every restatement of one (family, d) at one seed; an AssertionError where a precondition fails."""
    X, y, Q = make_data(family, d, seed)
    q = Q[:S]
    c = {"seed": seed, "X": X, "y": y, "Q": Q}
    ll = LD.ref_ll(family, X, y, q)
    c["lp"] = {prior: LD.ref_lp(family, ll, q, d, prior) for prior in (None, PRIOR)}
    assert all(np.isfinite(v[0].astype(np.float64)).all() for v in c["lp"].values())
    c["pred"] = PR.ref_stats(family, X, y, q)
    assert all(np.isfinite(v).all() for v in c["pred"][0].values()) and np.isfinite(c["pred"][1]).all()
    for s in (S, S_BIG):
        c["loo", s] = LO.ref_loo(family, X[:N_LOO], y[:N_LOO], Q[:s])          # asserts its own preconditions
        rtot = c["loo", s][2]
        assert rtot[7] == 0 and np.isfinite(rtot).all()                        # no non-finite row
    if family != "linear":
        _, mg, _ = PP.twin(family, X, q, SEED_PPC, STREAM_PPC)
        assert not (mg < ppc_ref.FRAGILE).any()                                # 1e-4 of 85 x 33 elements: none
    from stark_amd import engine
    for kind in KINDS:
        W = engine.boot_weights(SEED_BOOT, STREAM_BOOT, 0, N, 0, R, kind)
        c["boot", kind] = br.weighted(family, X, y, q[:R], W, PRIOR)
        assert all(np.isfinite(v.astype(np.float64)).all() for v in c["boot", kind])
    return c


def make_case(family, d):
    """The references at the first of the seeds seed0 + 0 .. 3 whose data meets every precondition, with the
    number of the attempt; never looks at device output."""
    seed0 = 73000 + 16 * d + 4 * FAMILIES.index(family)
    why = []
    for attempt in range(ATTEMPTS):
        try:
            c = references(family, d, seed0 + attempt)
        except AssertionError as e:
            why.append(f"seed {seed0 + attempt}: {e!r}")
            continue
        c["attempt"] = attempt
        return c
    raise AssertionError(f"no seed meets the restatements' preconditions for {family} d = {d}: {why}")


def run_logdens(m, c, family, d):
    q = c["Q"][:S]
    worst = 0.0
    for prior in (None, PRIOR):
        m.set_prior(*(prior or (None, None)))
        rlp, scale = c["lp"][prior]
        lp = m.log_density(q, 1)
        assert lp.shape == (S,) and np.isfinite(lp).all()
        err = float((np.abs(lp.astype(L) - rlp) / (LD.BAR * scale)).max())
        worst = max(worst, err)
        assert err <= 1.0, (family, d, prior, err)
        assert np.array_equal(m.log_density(q[:17], 1), lp[:17]), (family, d, prior)     # the same bits at any S
    m.set_prior(None, None)
    return {"lp": worst}


def run_predictive(m, c, family, d):
    q = c["Q"][:S]
    ref, rtot, tscale = c["pred"]
    tot, rows = m.log_predictive(q, 1, rows=True)
    assert all(np.isfinite(v).all() for v in rows.values()) and np.isfinite(tot).all()
    e_rows, e_tot = PR.row_errors(rows, ref), PR.total_errors(tot, rtot, tscale)
    assert e_rows <= 1 and e_tot <= 1, (family, d, e_rows, e_tot)
    assert np.array_equal(m.log_predictive(q, 1), tot), (family, d)                      # rows = NULL changes no total
    return {"rows": e_rows, "totals": e_tot}


def run_loo(m, c, family, d):
    from stark_amd import engine
    out = {}
    for s, waves in ((S, 4), (S_BIG, 8)):
        assert engine.loo_launch(N_LOO, d, s)["waves"] == waves
        q = c["Q"][:s]
        ref, kbar, rtot, tscale = c["loo", s]
        tot, rows = m.loo(q, 0, rows=True)
        assert tot[7] == 0 and np.isfinite(tot).all()
        LO.check_case(f"{family}-{N_LOO}-{d}-{s}", tot, rows, ref, kbar, rtot, tscale)
        assert np.array_equal(m.loo(q, 0), tot), (family, d, s)                          # rows = NULL changes no total
        e_rows, e_k, _ = LO.row_errors(rows, ref, kbar)
        out.update({f"rows{s}": e_rows, f"totals{s}": LO.total_errors(tot, rtot, tscale), f"khat{s}": e_k})
    return out


def run_ppc(m, c, family, d):
    q = c["Q"][:S]
    stats, obs, rows, yrep = m.posterior_predict(q, 1, seed=SEED_PPC, streams=[STREAM_PPC], rows=True, yrep=True)
    s2, o2 = m.posterior_predict(q, 1, seed=SEED_PPC, streams=[STREAM_PPC])              # k_yrep<.., false>: the same bits
    assert np.array_equal(stats, s2) and np.array_equal(obs, o2), (family, d)
    err = PP.check_shard(family, c["X"], c["y"], q, SEED_PPC, STREAM_PPC, stats, obs, rows, yrep)
    assert all(v <= 1.0 for v in err.values()), (family, d, err)
    return err


def run_boot(m, c, family, d):
    q = c["Q"][:R]
    worst = {"lp": 0.0, "grad": 0.0, "wsum": 0.0}
    m.set_prior(*PRIOR)
    for kind in KINDS:
        lp, g, ws = m.log_density_grad_boot(q, 1, seed=SEED_BOOT, streams=[STREAM_BOOT], kind=kind)
        assert lp.shape == (R,) and g.shape == (R, q.shape[1]) and ws.shape == (R,)
        assert np.isfinite(lp).all() and np.isfinite(g).all()
        e = BT.errors(lp, g, ws, c["boot", kind], kind)
        assert max(e) <= 1.0, (family, d, kind, e)
        for k, v in zip(("lp", "grad", "wsum"), e):
            worst[k] = max(worst[k], v)
        one = m.log_density_grad_boot(q[:1], 1, seed=SEED_BOOT, streams=[STREAM_BOOT], kind=kind)
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(one, (lp, g, ws))), (family, d, kind)
    m.set_prior(None, None)
    return worst


SWEEPS = (("logdens", run_logdens), ("predictive", run_predictive), ("loo", run_loo), ("ppc", run_ppc),
          ("boot", run_boot))


@pytest.mark.parametrize("kf", KFS)
@pytest.mark.parametrize("family", FAMILIES)
def test_every_width_of_the_five_sweeps(ctx, family, kf):
    from stark_amd import engine
    worst = {name: {} for name, _ in SWEEPS}
    attempts = []
    for d in widths(kf):
        assert (d + 3) // 4 == kf
        c = make_case(family, d)
        attempts.append(c["attempt"])
        X, y = c["X"], c["y"]
        m = engine.Model(ctx, family, [{"x": X[:N_LOO], "y": y[:N_LOO]}, {"x": X, "y": y}])
        try:
            for name, run in SWEEPS:
                for k, v in run(m, c, family, d).items():
                    if v >= worst[name].get(k, (-1.0, 0))[0]:
                        worst[name][k] = (v, d)
        finally:
            m.close()
    for name, _ in SWEEPS:
        txt = " ".join(f"{k}={v:.3e}@d={d}" for k, (v, d) in worst[name].items())
        print(f"MAXERR widths {name} family={family} kf={kf}: {txt} (units of the bar)")
    print(f"seed attempts family={family} kf={kf}: {attempts}")


def test_the_widths_cover_both_sides_of_64_kib_of_lds():
    """Host arithmetic (the launch infos).  Past 64 KiB of dynamic LDS a launch first needs allow_big_lds; the
    first such d of every sweep, from the LDS formulas of the .hip files (doubles, x 8 bytes):
        logdens     1024 + 128 + max(ring, 64 d) > 8192    <=>  d >= 111      (ring <= 4608 doubles)
        predictive  1024 + max(ring, 64 d)                  <=>  d >= 113
        ppc         1024 + 896 + max(ring, 64 d)            <=>  d >= 99
        boot        max(512 d + 8704, 8192 JT + 14336) bytes: JT = 7 from KF = 25, d = 97 (main from d = 112)
        loo         1024 + max(16 d, scratch) + 16 Sp + 8: below at every d at S = 33 (Sp = 64), above at every d
                    at S = 257 (Sp = 512: the matrix alone is 64 KiB) -- it crosses in S, and both S are run.
    d - 1 and d are both among the widths of test_every_width_of_the_five_sweeps."""
    from stark_amd import engine
    swept = {d for kf in KFS for d in widths(kf)}
    assert swept == set(range(1, 129))
    infos = {"logdens": (lambda d: engine.logdens_launch(N, d, S), 111),
             "predictive": (lambda d: engine.predictive_launch(N, d, S), 113),
             "ppc": (lambda d: engine.ppc_launch(N, d, S), 99),
             "boot": (lambda d: engine.boot_launch(N, d), 97),
             "loo S=33": (lambda d: engine.loo_launch(N_LOO, d, S), None),
             "loo S=257": (lambda d: engine.loo_launch(N_LOO, d, S_BIG), 1)}
    for name, (info, want) in infos.items():
        lds = {d: info(d)["lds_bytes"] for d in range(1, 129)}
        first = next((d for d in range(1, 129) if lds[d] > 65536), None)
        print(f"{name}: lds_bytes {lds[1]} at d = 1, {lds[128]} at d = 128; first d above 64 KiB: {first}")
        assert first == want, (name, first, want)
        assert all(lds[a] <= lds[b] for a, b in zip(range(1, 128), range(2, 129))), name     # one crossing
        if name.startswith("loo"):
            continue
        assert 2 <= first <= 128 and {first - 1, first} <= swept
