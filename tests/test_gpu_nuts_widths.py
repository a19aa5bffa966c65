"""The NUTS kernels at every chain-vector width against the CPU oracle's recursive Stan twin.

Fused 8-schools kernel (k_nuts_fused_schools, dispatched by stk_launch_nuts_fused / fused_cpw on
Dp = roundup8(max_s J_s + 2)); the instantiation a shard list reaches stands next to it in FUSED:

  nch1cpw4    Dp = 8        J <= 6      <1, 4>  SEG 16, plain (vectors in LDS, masked ok())
  nch1cpw4zp  Dp = 16       J = 7..14   <1, 4, .., ZP = true>  (nuts_fused4.hip: vectors in registers, padding +0)
  nch1cpw2    Dp = 24, 32   J = 15..30  <1, 2>  SEG 32 (seg_sum<32>: DPP row + __shfl_xor 16)
  nch1cpw1    Dp = 40..64   J = 31..62  <1, 1>  SEG 64
  nch2cpw1    Dp = 72..128  J = 63..126 <2, 1>  two lane chunks per vector

Generic step kernel of the regressions (k_nuts_step<NCH>, stk_nch_for on D): NCH = 1 for D <= 64,
2 for D <= 128, 4 for D <= 256, 16 for D <= 1024; REGRESSIONS names the NCH of every shape.

Bars (the project's own): q within rtol 1e-9 (8 schools) / 1e-8 (regressions), atol 1e-10; lp within
1e-9 max(1, |lp|); treedepth, n_leapfrog, divergent equal; accept_stat and energy within rtol 1e-9 /
atol 1e-12.  Every chain of every shard and every transition is compared; each case prints one
MAXERR line in units of those bars before it asserts them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C = 5          # chains per shard of the 8-schools cases: 5 chains leave the last wave partly empty at
               # 4 and at 2 chains per wave, and 2 x 5 put chains of both shards into one wave
EPS = (0.05, 0.3, 0.9, 2.5)

# (shard list: J per shard, the instantiation <NCH, CPW> it reaches, what is particular about it)
FUSED = [
    ([3], "nch1cpw4", "Dp=8"),
    ([6], "nch1cpw4", "Dp=8, D = Dp"),
    ([7], "nch1cpw4zp", "Dp=16"),
    ([14], "nch1cpw4zp", "Dp=16, D = SEG: no padding lane"),
    ([4, 8], "nch1cpw4zp", "Dp=16, short shard"),
    ([14, 3], "nch1cpw4zp", "Dp=16, short shard"),
    ([15], "nch1cpw2", "Dp=24"),
    ([22], "nch1cpw2", "Dp=24, D = Dp < SEG"),
    ([30], "nch1cpw2", "Dp=32, D = SEG"),
    ([30, 5], "nch1cpw2", "Dp=32, short shard"),
    ([31], "nch1cpw1", "Dp=40"),
    ([62], "nch1cpw1", "Dp=64, D = SEG"),
    ([63], "nch2cpw1", "Dp=72, second chunk holds one element"),
    ([94], "nch2cpw1", "Dp=96"),
    ([126], "nch2cpw1", "Dp=128, D = 2 SEG"),
    ([126, 8], "nch2cpw1", "Dp=128, a shard wholly in chunk 0"),
]


def _ids(cases):
    return ["J" + "_".join(str(j) for j in js) + "-" + kern for js, kern, _ in cases]


def _schools_shards(js):
    out = []
    for J in js:
        rng = np.random.default_rng(J)
        y = rng.normal(0, 10, J)
        out.append({"y": y, "sigma": rng.uniform(5, 20, J)})
    return out


def _schools_oracles(orc, shards):
    return [orc.Model(orc.FAM_SCHOOLS, y=sh["y"], sigma=sh["sigma"]) for sh in shards]


def _over(a, b, rtol, atol):
    """max |a - b| / (atol + rtol |b|), entries that agree exactly (inf, nan included) counting 0."""
    a, b = np.atleast_1d(np.asarray(a, float)), np.atleast_1d(np.asarray(b, float))
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore"):
        r = np.where(same, 0.0, np.abs(a - b) / (atol + rtol * np.abs(b)))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


class _Tally:
    """Collects (GPU, oracle) transitions; report() prints the largest errors in units of the bars,
    then asserts every bar on every row."""

    def __init__(self, tag, rtol_q):
        self.tag, self.rtol_q, self.rows = tag, rtol_q, []

    def add(self, where, q, lp, st, oq, olp, ost):
        self.rows.append((where, np.array(q), float(lp), np.array(st), np.array(oq), float(olp), np.array(ost)))

    def report(self, extra=""):
        eq = elp = est = 0.0
        flips = 0
        for _, q, lp, st, oq, olp, ost in self.rows:
            eq = max(eq, _over(q, oq, self.rtol_q, 1e-10))
            elp = max(elp, _over(lp, olp, 0.0, 1e-9 * max(1.0, abs(olp))))
            est = max(est, _over(st[[0, 5]], ost[[0, 5]], 1e-9, 1e-12))
            flips += int(not np.array_equal(st[2:5], ost[2:5]))
        print(f"MAXERR {self.tag} transitions={len(self.rows)} flipped={flips} q_over_bar={eq:.3e} "
              f"lp_over_bar={elp:.3e} stat_over_bar={est:.3e}{extra}")
        assert self.rows
        for where, q, lp, st, oq, olp, ost in self.rows:
            assert st[2] == ost[2] and st[3] == ost[3] and st[4] == ost[4], (where, st, ost)
            np.testing.assert_allclose(q, oq, rtol=self.rtol_q, atol=1e-10, err_msg=str(where))
            assert abs(lp - olp) <= 1e-9 * max(1.0, abs(olp)), (where, lp, olp)
            np.testing.assert_allclose(st[[0, 5]], ost[[0, 5]], rtol=1e-9, atol=1e-12, err_msg=str(where))
        return eq, elp, est


# ================================================================ 1. fused kernel, fixed-step transitions
def _fused_fixed_inputs(js, eps):
    """Start points and metric of every shard at one eps (one generator per case and eps)."""
    rng = np.random.default_rng(1000 * sum(js) + int(eps * 100))
    return [(rng.normal(0, 1, (C, J + 2)), rng.uniform(0.5, 2.0, J + 2)) for J in js]


def _fused_fixed_oracle(orc, js):
    oms = _schools_oracles(orc, _schools_shards(js))
    want = {}
    for eps in EPS:
        for s, (q0, im) in enumerate(_fused_fixed_inputs(js, eps)):
            for c in range(C):
                want[eps, s, c] = oms[s].transition(q0[c], seed=77, gid=s * C + c, iteration=5, eps=eps, inv_metric=im)
    return want


def _assert_fused_fixed_shape(js, want):
    """The case is what it is meant to be, by the oracle alone, across its eps values."""
    depth = {eps: sorted({int(w[2][2]) for (e, _, _), w in want.items() if e == eps}) for eps in EPS}
    assert max(max(v) for v in depth.values()) >= 4, depth                  # a deep tree: merges at 4 levels
    assert len({tuple(v) for v in depth.values()}) > 1, depth               # depths differ between eps values
    assert sum(int(w[2][4]) for w in want.values()) >= 1                    # a divergent chain
    moved = 0
    for eps in EPS:
        for s, (q0, _) in enumerate(_fused_fixed_inputs(js, eps)):
            moved += sum(bool(np.any(want[eps, s, c][0] != q0[c])) for c in range(C))
    assert moved >= 1
    return depth


@pytest.mark.parametrize("js,kern,what", FUSED, ids=_ids(FUSED))
def test_fused_fixed_step_matches_oracle(ctx, orc, js, kern, what):
    """One fixed-step transition of every chain of every shard at four step sizes (deep trees,
    mixed depths, divergences at the first leaves) vs the oracle's twin on the same RNG stream.
    The models with the longer shard first ([14, 3], [30, 5], [126, 8]) also pin the explicit-init
    layout: packed at the chain's own D, a short shard's inits overwrote the long shard's."""
    from stark_amd import engine
    want = _fused_fixed_oracle(orc, js)
    depth = _assert_fused_fixed_shape(js, want)
    m = engine.Model(ctx, "schools", _schools_shards(js))
    t = _Tally(f"fused_fixed[{'-'.join(map(str, js))}]", 1e-9)
    try:
        for eps in EPS:
            for s, (q0, im) in enumerate(_fused_fixed_inputs(js, eps)):
                q, lp, st = m.transition(s, q0, seed=77, iteration=5, eps=eps, inv_metric=im)
                for c in range(C):
                    oq, olp, ost, _ = want[eps, s, c]
                    t.add((eps, s, c), q[c], lp[c], st[c], oq, olp, ost)
    finally:
        m.close()
    assert len(t.rows) == len(EPS) * len(js) * C
    t.report(f" depths={[depth[e] for e in EPS]} kernel={kern}")


# ================================================================ 2. adaptive runs, replayed transition by transition
NW, NS, SEED = 30, 25, 91


def _run_arrays(s, nshards):
    """Everything a run leaves behind, for bitwise comparisons."""
    out = {"eps": s.adaptation()[0], "metric": s.adaptation()[1]}
    for k in range(nshards):
        d, st = s.draws(k)
        out[f"draws{k}"], out[f"stats{k}"], out[f"uq{k}"] = d, st, s.unconstrained(k)
    info = s.info()
    for k in ("grad_evals", "leapfrogs", "divergent", "done", "errors"):
        out[k] = np.array(info[k])
    return out


def _assert_same_run(a, b):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _replay(orc, tally, oms, run, nw, ns, chains, seed, ext, streams, max_depth=10):
    """Every post-warmup transition t of every chain, redone by the oracle from the GPU's own
    previous draw with the GPU's step size and adapted metric: nothing accumulates."""
    for s, om in enumerate(oms):
        D = om.D
        uq, d, st = run[f"uq{s}"], run[f"draws{s}"], run[f"stats{s}"]
        assert uq.shape == (chains, nw + ns, D)
        for c in range(chains):
            gid = s * chains + c
            im = run["metric"][gid, :D]
            for t in range(max(nw, 1), nw + ns):
                i = c * ns + t - nw
                oq, olp, ost, _ = om.transition(uq[c, t - 1], seed=seed, gid=streams[s] * chains + c, iteration=t,
                                                eps=st[i, 1], inv_metric=im, uturn_ext=ext, max_depth=max_depth)
                tally.add((s, c, t), uq[c, t], d[-1, i], st[i], oq, olp, ost)


def _check_schools_draws(js, run, chains, ns):
    """Constrained rows of every shard: mu, tau = exp(u), eta, theta = mu + tau eta, lp__ last."""
    for s, J in enumerate(js):
        D, P = J + 2, 2 * J + 3
        d, uq = run[f"draws{s}"], run[f"uq{s}"][:, -ns:, :].reshape(chains * ns, D)
        assert d.shape == (P, chains * ns)          # lp__ is row P_s - 1 of each shard (_replay reads d[-1])
        np.testing.assert_array_equal(d[0], uq[:, 0])
        np.testing.assert_allclose(d[1], np.exp(uq[:, 1]), rtol=1e-15)
        np.testing.assert_array_equal(d[2:D], uq[:, 2:].T)
        for e in range(2, D):
            np.testing.assert_allclose(d[D + e - 2], d[0] + d[1] * d[e], rtol=1e-12, atol=1e-12)
        assert np.isfinite(d[P - 1]).all()


def _adaptive_schools_case(ctx, orc, js, crit, tag, jitter=0.0, shard_ids=None):
    from stark_amd import engine
    shards = _schools_shards(js)
    oms = _schools_oracles(orc, shards)
    ext = crit == "stan2.23"
    streams = list(shard_ids) if shard_ids is not None else list(range(len(js)))
    m = engine.Model(ctx, "schools", shards)
    s = m.sampler(num_warmup=NW, num_samples=NS, chains=C, seed=SEED, save_warmup=True, nuts_criterion=crit,
                  stepsize_jitter=jitter, shard_ids=shard_ids)
    try:
        s.run()
        run = _run_arrays(s, len(js))
    finally:
        s.close()
        m.close()
    assert run["errors"] == 0 and run["done"] == len(js) * C
    t = _Tally(tag, 1e-9)
    _replay(orc, t, oms, run, NW, NS, C, SEED, ext, streams)
    assert len(t.rows) == len(js) * C * NS
    # the start of the run (init_stepsize, the first warmup transitions) on the twin's own path
    e10 = 0.0
    for k, om in enumerate(oms):
        for c in range(C):
            o = om.run_chain(num_warmup=NW, num_samples=NS, seed=SEED, gid=streams[k] * C + c, stepsize_jitter=jitter,
                             uturn_ext=ext)
            e10 = max(e10, float(np.abs(run[f"uq{k}"][c, :10] - o["q"][:10]).max()))
    t.report(f" first10_abs={e10:.3e}")
    assert e10 < 1e-8, e10
    if jitter:
        assert all(np.ptp(run[f"stats{k}"][:NS, 1]) > 0 for k in range(len(js)))
    _check_schools_draws(js, run, C, NS)
    return run


# [63] keeps the <2,1> image below 64 KiB with both criteria; [126, 8] with stan2.23 lies above it
# (test_fused_lds_image_sides)
ADAPTIVE = [f for f in FUSED if f[0] in ([3], [14], [4, 8], [22], [30, 5], [62], [63], [126, 8])]


@pytest.mark.parametrize("crit", ["stan2.19", "stan2.23"])
@pytest.mark.parametrize("js,kern,what", ADAPTIVE, ids=_ids(ADAPTIVE))
def test_fused_adaptive_run_replays_on_oracle(ctx, orc, js, kern, what, crit):
    """30 warmup + 25 sampling transitions with adaptation; every post-warmup transition of every
    chain replayed by the oracle (the metric at a short shard's padding lanes is not observable:
    the replay of that shard's transitions is the check that the padding stayed inert), the first
    10 transitions against the oracle's own run, and the constrained rows."""
    _adaptive_schools_case(ctx, orc, js, crit, f"fused_adaptive[{'-'.join(map(str, js))}-{crit}]")


def test_fused_adaptive_run_replays_on_oracle_jitter(ctx, orc):
    """<1,4,ZP> with a short shard, stepsize_jitter = 0.5: the per-transition step size is the stat's."""
    _adaptive_schools_case(ctx, orc, [4, 8], "stan2.19", "fused_adaptive[4-8-jitter0.5]", jitter=0.5)


def test_fused_adaptive_run_replays_on_oracle_shard_ids(ctx, orc):
    """<1,2> with a short shard and global shard ids [5, 2]: the RNG stream is shard_ids[s] * C + c."""
    _adaptive_schools_case(ctx, orc, [30, 5], "stan2.23", "fused_adaptive[30-5-ids5,2]", shard_ids=[5, 2])


# ================================================================ 3. packing, launch boundaries, resume: bitwise
def _schools_run(ctx, js, nw=NW, ns=NS, split=None, **cfg):
    """split: None (one run() call), a list of targets, or "launches" (one launch per run() call)."""
    from stark_amd import engine
    m = engine.Model(ctx, "schools", _schools_shards(js))
    s = m.sampler(num_warmup=nw, num_samples=ns, chains=C, seed=SEED, save_warmup=True, **cfg)
    calls = 0
    try:
        if split == "launches":
            while s.info()["done"] < len(js) * C:
                s.run(nw + ns, max_steps=1)
                calls += 1
                assert calls < 1000
        else:
            for target in (split or []):
                s.run(target)
            s.run()
        out = _run_arrays(s, len(js))
    finally:
        s.close()
        m.close()
    out["calls"] = np.array(calls)
    return out


@pytest.mark.parametrize("js,caps", [([3], (1, 2)), ([14], (1, 2)), ([14, 3], (1, 2)),      # default 4: <1,4>, <1,4,ZP>
                                     ([22], (1, 4)), ([30, 5], (1, 4))],                    # default 2: <1,2>
                         ids=["J3-nch1cpw4", "J14-nch1cpw4zp", "J14_3-nch1cpw4zp", "J22-nch1cpw2", "J30_5-nch1cpw2"])
def test_fused_chains_per_wave_changes_no_bit(ctx, js, caps):
    """chains_per_wave caps the packing (fused_cpw takes the minimum with the default): draws,
    stats, step sizes and metric are identical to the default packing."""
    ref = _schools_run(ctx, js)
    assert ref["errors"] == 0
    for cap in caps:
        _assert_same_run(ref, _schools_run(ctx, js, chains_per_wave=cap))


# (shard list, warmup, samples): by the oracle's n_grad at least one chain exceeds the 4096
# evaluations of one launch, so it is saved and reloaded mid-trajectory.
#   [3]  <1,4>   [22] <1,2> (two chains per wave)   [94] <2,1> (two chunks)
BOUNDARY = [([3], 60, 60), ([22], 150, 150), ([94], 100, 100)]


@pytest.mark.parametrize("js,nw,ns", BOUNDARY, ids=["J3-nch1cpw4", "J22-nch1cpw2", "J94-nch2cpw1"])
def test_fused_launch_boundaries_change_no_bit(ctx, orc, js, nw, ns):
    """The host launches the fused kernel with a budget of 4096 evaluations per chain: the unsplit
    run, run(20); run(61); run(), and one launch per run() call are identical."""
    om = _schools_oracles(orc, _schools_shards(js))[0]
    ngrad = [om.run_chain(num_warmup=nw, num_samples=ns, seed=SEED, gid=c)["n_grad"] for c in range(C)]
    assert max(ngrad) > 4096, ngrad
    a = _schools_run(ctx, js, nw, ns)
    assert a["errors"] == 0 and a["done"] == C
    b = _schools_run(ctx, js, nw, ns, split=[20, 61])
    c = _schools_run(ctx, js, nw, ns, split="launches")
    assert c["calls"] >= 2, c["calls"]
    for x in (a, b, c):
        x.pop("calls")
    _assert_same_run(a, b)
    _assert_same_run(a, c)


@pytest.mark.parametrize("js", [[22], [94]], ids=["J22-nch1cpw2", "J94-nch2cpw1"])
def test_fused_save_load_state_in_process(ctx, js):
    """save_state -> fresh sampler -> load_state -> run() continues bit for bit; a blob of a
    chains_per_wave = 1 sampler is refused by a default one (the geometry hash covers the cap)."""
    from stark_amd import engine
    ref = _schools_run(ctx, js)
    m = engine.Model(ctx, "schools", _schools_shards(js))
    cfg = dict(num_warmup=NW, num_samples=NS, chains=C, seed=SEED, save_warmup=True)
    a, b, c1, d = m.sampler(**cfg), m.sampler(**cfg), m.sampler(chains_per_wave=1, **cfg), m.sampler(**cfg)
    try:
        a.run(37)
        blob = a.save_state()
        b.load_state(blob)
        assert int(b.iterations().min()) == 37
        b.run()
        got = _run_arrays(b, 1)
        c1.run(37)
        with pytest.raises(engine.StarkHipError, match="another model geometry or sampler config"):
            d.load_state(c1.save_state())
    finally:
        for x in (a, b, c1, d):
            x.close()
        m.close()
    ref.pop("calls")
    _assert_same_run(ref, got)


# ================================================================ 4. limits of the fused kernel
def _fused_lds_bytes(J, ext, max_depth):
    """launch_fused_zp's dynamic-LDS formula (nuts.hip) for a one-shard model at the default packing."""
    Dp = (J + 2 + 7) // 8 * 8
    cpw = 4 if Dp <= 16 else 2 if Dp <= 32 else 1
    zp = Dp == 16
    V_COUNT, S_COUNT, I_COUNT, SS_COUNT, MT_N = 17, 17, 15, 3, 128 + 4 * 129
    per = (0 if zp else V_COUNT * Dp) + max_depth * (7 if ext else 4) * Dp + max_depth * SS_COUNT \
        + S_COUNT + (I_COUNT + 1) // 2 + 2 * (64 // cpw)
    per += per & 1
    return 8 * (cpw * per + MT_N)


def test_fused_lds_image_sides():
    """Which <2,1> configs of this file lie above the 64 KiB line (allow_big_lds) and which above the
    CU's 160 KiB (refused).  At max_depth 10: stan2.19 stays below 64 KiB up to J = 126 (64,992 B);
    stan2.23 crosses it from J = 79 (Dp = 88) on."""
    K = 1024
    assert _fused_lds_bytes(63, False, 10) < _fused_lds_bytes(63, True, 10) < 64 * K      # section 2, [63]
    assert _fused_lds_bytes(126, False, 10) == 64992 < 64 * K                              # section 1, [126]
    assert _fused_lds_bytes(126, True, 10) == 95712 > 64 * K                               # section 2, [126, 8] stan2.23
    assert _fused_lds_bytes(78, True, 10) < 64 * K < _fused_lds_bytes(79, True, 10)
    assert 64 * K < _fused_lds_bytes(126, False, 30) == 147392 < 160 * K                   # the largest accepted
    assert _fused_lds_bytes(126, True, 19) < 160 * K < _fused_lds_bytes(126, True, 20)     # refused from 20 on
    assert max(_fused_lds_bytes(J, True, 30) for J in range(1, 63)) < 160 * K              # only <2,1> can exceed


def test_fused_refuses_j_127(ctx):
    from stark_amd import engine
    m = engine.Model(ctx, "schools", _schools_shards([127]))
    try:
        with pytest.raises(engine.StarkHipError, match="J <= 126"):
            m.sampler(num_warmup=0, num_samples=1, chains=1)
    finally:
        m.close()


def test_fused_refuses_image_above_the_cu_lds(ctx):
    """J = 126, stan2.23: max_depth >= 20 needs more than 160 KiB of LDS per chain and is refused
    with STK_E_ARG by stk_sampler_create (nothing is launched); max_depth 19 is created."""
    from stark_amd import engine
    m = engine.Model(ctx, "schools", _schools_shards([126]))
    cfg = dict(num_warmup=0, num_samples=1, chains=1, nuts_criterion="stan2.23")
    try:
        for md in (20, 30):
            with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG.*J = 126.*max_depth " + str(md)) as ei:
                m.sampler(max_depth=md, **cfg)
            assert str(160 * 1024) in str(ei.value) and str(_fused_lds_bytes(126, True, md)) in str(ei.value)
        m.sampler(max_depth=19, **cfg).close()
    finally:
        m.close()


def test_fused_largest_accepted_image_replays_on_oracle(ctx, orc):
    """<2,1> at J = 126, stan2.19, max_depth 30: 147,392 B of LDS, through allow_big_lds.  Three
    fixed-step transitions from an explicit init, each replayed by the oracle."""
    from stark_amd import engine
    js, ns = [126], 3
    shards = _schools_shards(js)
    init = np.random.default_rng(126).normal(0, 1, (C, 128))
    m = engine.Model(ctx, "schools", shards)
    s = m.sampler(num_warmup=0, num_samples=ns, chains=C, seed=SEED, max_depth=30, adapt_engaged=False,
                  skip_init_stepsize=True, stepsize=0.3, init=init, nuts_criterion="stan2.19")
    try:
        s.run()
        run = _run_arrays(s, 1)
    finally:
        s.close()
        m.close()
    assert run["errors"] == 0 and run["done"] == C
    om = _schools_oracles(orc, shards)[0]
    t = _Tally("fused_big_lds[126-stan2.19-depth30]", 1e-9)
    _replay(orc, t, [om], run, 0, ns, C, SEED, False, [0], max_depth=30)         # transitions 1, 2
    for c in range(C):                                                            # transition 0, from the init
        oq, olp, ost, _ = om.transition(init[c], seed=SEED, gid=c, iteration=0, eps=0.3, max_depth=30)
        t.add((0, c, 0), run["uq0"][c, 0], run["draws0"][-1, c * ns], run["stats0"][c * ns], oq, olp, ost)
    assert len(t.rows) == C * ns
    np.testing.assert_array_equal(run["stats0"][:, 1], 0.3)
    t.report()
    _check_schools_draws(js, run, C, ns)


# ================================================================ 5. k_nuts_step<NCH> at NCH = 2, 4, 16
# (family, d, chains, D, NCH of k_nuts_step by stk_nch_for)
REGRESSIONS = [
    ("logistic", 64, 4, 65, 2),        # the first D of NCH = 2
    ("logistic", 99, 16, 100, 2),
    ("logistic", 100, 16, 101, 2),     # the headline shape (BASELINE configs[3])
    ("logistic", 127, 8, 128, 2),      # the last D of NCH = 2
    ("linear", 63, 8, 65, 2),
    ("linear", 126, 16, 128, 2),
    ("logistic", 255, 8, 256, 4),      # the last D of NCH = 4
    ("linear", 254, 8, 256, 4),
    ("logistic", 256, 8, 257, 16),     # the first D of NCH = 16
    ("logistic", 300, 64, 301, 16),
    ("logistic", 1023, 8, 1024, 16),   # the last D the sampler takes
    ("linear", 1022, 64, 1024, 16),
]


def _nch_for(D):
    return 1 if D <= 64 else 2 if D <= 128 else 4 if D <= 256 else 16


def _regression_case(orc, family, d, chains, rows=None):
    """Two shards (400 and 130 rows; 300 and 130 where d >= 1022) from one generator, their oracle
    models, and the start points."""
    rows = rows or [300 if d >= 1022 else 400, 130]
    rng = np.random.default_rng(1000 * d + chains)
    N = sum(rows)
    X = rng.uniform(-1.7, 1.7, (N, d))
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    if family == "logistic":
        y = (rng.uniform(size=N) < 1 / (1 + np.exp(-(0.2 + X @ beta)))).astype(np.int32)
        fam, D = orc.FAM_LOGREG, d + 1
    else:
        y = 0.3 + X @ beta + rng.normal(size=N)
        fam, D = orc.FAM_LINREG, d + 2
    shards = [{"x": X[:rows[0]], "y": y[:rows[0]]}, {"x": X[rows[0]:], "y": y[rows[0]:]}]
    oms = [orc.Model(fam, X=sh["x"], y=sh["y"]) for sh in shards]
    q0 = np.random.default_rng(5).normal(0, 0.1, (chains, D))
    return shards, oms, q0, D


@pytest.mark.parametrize("family,d,chains,D,nch", REGRESSIONS,
                         ids=[f"{f}-{d}-{c}-nch{n}" for f, d, c, _, n in REGRESSIONS])
def test_step_kernel_fixed_step_matches_oracle(ctx, orc, family, d, chains, D, nch):
    """One fixed-step transition of every chain of two unequal shards through k_nuts_step<NCH>
    (and the sweeps that feed it) vs the oracle's twin."""
    from stark_amd import engine
    shards, oms, q0, D_ = _regression_case(orc, family, d, chains)
    assert D_ == D and _nch_for(D) == nch
    kw = dict(seed=7, iteration=11, eps=0.05 if family == "logistic" else 0.02, max_depth=5)
    want = [[om.transition(q0[c], gid=s * chains + c, **kw) for c in range(chains)] for s, om in enumerate(oms)]
    leaps = sorted({int(w[2][3]) for ws in want for w in ws})
    assert max(leaps) >= 15, leaps
    assert all(np.any(w[0] != q0[c]) for ws in want for c, w in enumerate(ws))          # every chain moved
    m = engine.Model(ctx, family, shards)
    t = _Tally(f"step_fixed[{family}-{d}-{chains}-NCH{nch}]", 1e-8)
    try:
        for s in range(2):
            q, lp, st = m.transition(s, q0, **kw)
            for c in range(chains):
                oq, olp, ost, _ = want[s][c]
                t.add((s, c), q[c], lp[c], st[c], oq, olp, ost)
    finally:
        m.close()
    assert len(t.rows) == 2 * chains
    t.report(f" leapfrogs={leaps}")


def test_step_kernel_adaptive_run_replays_on_oracle(ctx, orc):
    """k_nuts_step<2> at the headline width (logistic, d = 100, 16 chains, D = 101): 30 warmup + 20
    sampling transitions with adaptation, every post-warmup transition replayed by the oracle.

    Shards of 1000 and 600 rows: an adaptive run needs a proper posterior.  The 130 rows of the
    fixed-step cases are linearly separable at d = 100 (flat priors), the chains run off (|q| reaches
    2.9e3 in the oracle's own run) and the oracle does not replay ITSELF there: from starts perturbed
    by 1e-13 relative, 14 of its 320 transitions change depth and the rest miss the bar by up to
    1e6.  On these shards the same probe of the oracle alone gives 0 of 640, worst 9e-4 of the bar,
    |q| <= 3.3; the first assertion below is that precondition."""
    from stark_amd import engine
    chains, nw, ns, seed = 16, 30, 20, 91
    shards, oms, _, D = _regression_case(orc, "logistic", 100, chains, rows=[1000, 600])
    assert _nch_for(D) == 2
    for k, om in enumerate(oms):
        assert np.abs(om.run_chain(num_warmup=nw, num_samples=ns, seed=seed, gid=k * chains)["q"]).max() < 10
    m = engine.Model(ctx, "logistic", shards)
    s = m.sampler(num_warmup=nw, num_samples=ns, chains=chains, seed=seed, save_warmup=True)
    try:
        s.run()
        run = _run_arrays(s, 2)
    finally:
        s.close()
        m.close()
    assert run["errors"] == 0 and run["done"] == 2 * chains
    t = _Tally("step_adaptive[logistic-100-16-NCH2]", 1e-8)
    _replay(orc, t, oms, run, nw, ns, chains, seed, False, [0, 1])
    assert len(t.rows) == 2 * chains * ns
    t.report()
    for k in range(2):      # logistic: the draws are the unconstrained rows and lp__
        np.testing.assert_array_equal(run[f"draws{k}"][:D], run[f"uq{k}"][:, nw:, :].reshape(chains * ns, D).T)


def test_step_kernel_refuses_d_1024(ctx):
    """logistic d = 1024 (D = 1025): the density hook works, the sampler has no k_nuts_step for it."""
    from stark_amd import engine
    rng = np.random.default_rng(1024)
    X = rng.uniform(-1.7, 1.7, (40, 1024))
    m = engine.Model(ctx, "logistic", [{"x": X, "y": (rng.uniform(size=40) < 0.5).astype(np.int32)}])
    try:
        lp, g = m.log_density_grad(0, np.zeros((8, 1025)))
        assert np.isfinite(lp).all() and np.isfinite(g).all()
        with pytest.raises(engine.StarkHipError, match=r"too large \(max 1024\)"):
            m.sampler(num_warmup=0, num_samples=1, chains=8)
    finally:
        m.close()
