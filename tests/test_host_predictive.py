"""Host side of the pointwise log-predictive sweep: the launch geometry (a pure function), engine.waic,
stark.unconstrain_draws and Stark.waic's exchange on a gloo world of 2 -- no GPU."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import ROOT


def test_launch_info_is_a_pure_function():
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    a = engine.predictive_launch(12500000, 100, 1024)
    assert a == engine.predictive_launch(12500000, 100, 1024)
    assert set(a) == {"T", "G", "waves", "lds_bytes", "image_bytes", "ws_bytes_per_shard"}
    assert a["T"] == 16 and a["waves"] == 4
    # chunks: a function of n alone, whole 64-row groups, never more chunks than groups
    for n in (1, 63, 64, 65, 257, 1030, 10 ** 6, 12500000):
        gs = {engine.predictive_launch(n, d, S)["G"] for d in (1, 17, 100, 128) for S in (1, 16, 1000)}
        assert len(gs) == 1
        G = gs.pop()
        assert 1 <= G <= (n + 63) // 64
        assert engine.predictive_launch(n, 5, 3)["ws_bytes_per_shard"] == G * 8 * 8
    assert engine.predictive_launch(64, 5, 3)["G"] == 1 and engine.predictive_launch(1030, 5, 3)["G"] >= 3
    # the image: ceil(S / 16) tiles of ceil(d / 4) k-steps x 64 lanes plus 64 per-draw scalars, each tile
    # padded to a multiple of 256 doubles
    for d in (1, 4, 5, 100, 127, 128):
        for S in (1, 16, 17, 1024):
            slab = -(-(64 * -(-d // 4) + 64) // 256) * 256
            info = engine.predictive_launch(1000, d, S)
            assert info["image_bytes"] == -(-S // 16) * slab * 8
            assert info["lds_bytes"] == engine.predictive_launch(7, d, 1)["lds_bytes"] <= 80 * 1024   # two blocks per CU
    for bad, word in (((100, 129, 16), "d = 129"), ((100, 1025, 16), "d = 1025"), ((100, 5, 0), "S = 0")):
        with pytest.raises(StarkHipError, match=word) as e:
            engine.predictive_launch(*bad)
        assert e.value.code == -1


def test_waic_from_hand_computed_totals():
    from stark_amd import engine
    e = np.array([-1.0, -2.5, -0.25, -4.0])
    lppd = np.array([-0.5, -2.0, -0.25, -3.0])
    var = lppd - e
    t = np.array([[2, lppd[:2].sum(), var[:2].sum(), e[:2].sum(), (e[:2] ** 2).sum(), 1, 0, 0],
                  [2, lppd[2:].sum(), var[2:].sum(), e[2:].sum(), (e[2:] ** 2).sum(), 1, 0, 0]])
    w = engine.waic(t)
    assert w["n"] == 4 and w["lppd"] == -5.75 and w["p_waic"] == 2.0 and w["elpd_waic"] == -7.75
    assert w["waic"] == 15.5 and w["n_high_var"] == 2 and w["n_non_finite"] == 0
    se = np.sqrt(4 / 3 * ((e ** 2).sum() - e.sum() ** 2 / 4))
    assert abs(w["se"] - se) < 1e-15 and abs(w["se"] - np.sqrt(4 * e.var(ddof=1))) < 1e-14
    assert engine.waic(t[0]) == engine.waic(t[:1])                       # [8] and [1, 8]
    one = engine.waic([1, -0.7, 0.1, -0.8, 0.64, 0, 0, 0])
    assert one["n"] == 1 and one["se"] == 0.0 and one["elpd_waic"] == -0.8 and one["waic"] == 1.6
    bad = engine.waic([[3, np.nan, np.nan, np.nan, np.nan, 0, 1, 0]])
    assert bad["n_non_finite"] == 1 and np.isnan(bad["elpd_waic"]) and np.isnan(bad["se"])
    with pytest.raises(ValueError, match="8"):
        engine.waic(np.zeros((2, 7)))


def test_unconstrain_draws_round_trips_and_refuses():
    from stark_amd import stark
    rng = np.random.default_rng(1)
    S, d = 7, 3
    q = rng.normal(size=(S, d + 1))
    m = np.vstack([q.T, rng.normal(size=(1, S))])                        # alpha, beta, lp__
    for fam in ("logistic", "poisson"):
        assert np.array_equal(stark.unconstrain_draws(fam, m), q)
        assert np.array_equal(stark.unconstrain_draws(fam, m, n_cols=d), q)
    ql = rng.normal(size=(S, d + 2))
    ml = np.vstack([ql[:, :-1].T, np.exp(ql[:, -1])[None, :], rng.normal(size=(1, S))])
    out = stark.unconstrain_draws("linear", ml, n_cols=d)
    assert out.shape == (S, d + 2) and out.flags["C_CONTIGUOUS"]
    assert np.array_equal(out[:, :-1], ql[:, :-1]) and np.abs(out[:, -1] - ql[:, -1]).max() < 1e-15
    with pytest.raises(ValueError, match="pars= selection cannot be scored"):
        stark.unconstrain_draws("logistic", m[1:], n_cols=d)            # a row short: P != D + 1
    with pytest.raises(ValueError, match="pars= selection cannot be scored"):
        stark.unconstrain_draws("linear", ml[[0, -1]])                   # alpha and lp__ alone
    neg = ml.copy()
    neg[d + 1, 4] = -0.5
    with pytest.raises(ValueError, match="draw 4"):
        stark.unconstrain_draws("linear", neg, n_cols=d)
    with pytest.raises(ValueError, match="schools"):
        stark.unconstrain_draws("schools", m)


# ---------------------------------------------------------------- Stark.waic on 1 and 2 processes
N_PARTS, K, S_DRAWS = 5, 3, 6


def _fake_totals(self, datas, q):
    """Stands in for the GPU: eight numbers per partition, a function of its rows and the draws."""
    out = []
    for dct in datas:
        a = float(np.sum(dct["x"])) + float(np.sum(dct["y"]))
        n = float(dct["N"])
        e = -abs(a) - float(np.abs(q).sum())
        out.append(np.array([n, e + 0.125 * n, 0.125 * n, e, e * e / n + 0.5, n // 4, 0, 0]))
    return out


def _waic_driver(monkeypatch):
    from stark_amd import stark
    from stark_amd.rdd import LocalContext
    rng = np.random.default_rng(4)
    rows = [tuple(r) for r in np.column_stack([rng.normal(size=(37, K)), rng.integers(0, 2, 37)])]

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": K, "x": a[:, :K], "y": a[:, K].astype(np.int64)}

    monkeypatch.setattr(stark.Stark, "_partition_totals", _fake_totals)
    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize(rows, N_PARTS), prep)
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "logistic.stan"))
    samples = np.vstack([rng.normal(size=(K + 1, S_DRAWS)), np.zeros((1, S_DRAWS))])
    return st, samples


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mp_ = pytest.MonkeyPatch()
        st, samples = _waic_driver(mp_)
        out = st.waic(samples)
        q.put((rank, {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in out.items()}))
        mp_.undo()
    finally:
        dist.destroy_process_group()


def test_stark_waic_is_the_same_on_one_and_two_ranks(monkeypatch):
    from stark_amd import engine
    st, samples = _waic_driver(monkeypatch)
    one = st.waic(samples)
    assert one["partition_totals"].shape == (N_PARTS, 8) and one["n"] == 37
    assert {k: v for k, v in one.items() if k != "partition_totals"} == engine.waic(one["partition_totals"])
    with pytest.raises(ValueError, match="pars= selection cannot be scored"):
        st.waic(samples[1:])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res.sort(key=lambda r: r[0])
    assert res[0][1] == res[1][1]
    want = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in one.items()}
    assert res[0][1] == want
