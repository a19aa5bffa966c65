"""Host side of the PSIS-LOO sweep: the launch geometry (a pure function), engine.loo, Stark.loo's
refusals before any device call, and the host check of psis_math.h against long double -- no GPU."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def test_launch_info_is_a_pure_function():
    from stark_amd import engine
    a = engine.loo_launch(12500000, 100, 1024)
    assert a == engine.loo_launch(12500000, 100, 1024)
    assert set(a) == {"T", "G", "waves", "lds_bytes", "image_bytes", "ws_bytes_per_shard"}
    assert a["T"] == 16 and a["waves"] in (4, 8)
    assert a["lds_bytes"] <= 160 * 1024                     # the CU's LDS, at the largest S
    assert engine.loo_launch(100, 128, 1024)["lds_bytes"] <= 160 * 1024
    # chunks: a function of n alone, whole 16-row tiles, never more chunks than tiles
    for n in (1, 15, 16, 17, 257, 1030, 10 ** 6, 12500000):
        gs = {engine.loo_launch(n, d, S)["G"] for d in (1, 17, 100, 128) for S in (1, 16, 1000)}
        assert len(gs) == 1
        G = gs.pop()
        assert 1 <= G <= (n + 15) // 16
        assert engine.loo_launch(n, 5, 3)["ws_bytes_per_shard"] == G * 8 * 8
    assert engine.loo_launch(16, 5, 3)["G"] == 1 and engine.loo_launch(1030, 5, 3)["G"] >= 3
    # the LDS holds the 16 x Sp matrix of log ratios (Sp: S padded to a power of two) and is sized from S
    for d in (1, 5, 100, 128):
        prev = 0
        for S in (1, 16, 17, 100, 256, 257, 1024):
            info = engine.loo_launch(1000, d, S)
            Sp = max(16, 1 << (S - 1).bit_length())
            assert info["lds_bytes"] >= 8 * 16 * Sp + 8 * 1024
            assert info["lds_bytes"] >= prev and info["lds_bytes"] == engine.loo_launch(7, d, S)["lds_bytes"]
            prev = info["lds_bytes"]
            assert info["image_bytes"] == engine.predictive_launch(1000, d, S)["image_bytes"]   # the same draw image
    assert engine.loo_launch(1000, 100, 256)["lds_bytes"] < 64 * 1024
    # waves per block: a function of S alone (the totals' summation order follows it)
    for S in (1, 100, 256, 257, 1024):
        assert len({engine.loo_launch(n, d, S)["waves"] for n in (1, 1000, 10 ** 6) for d in (1, 100, 128)}) == 1


def test_launch_info_refuses_with_the_value_named():
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    for bad, word in (((100, 129, 16), "d = 129"), ((100, 5, 0), "S = 0"), ((100, 5, 1025), "S = 1025")):
        with pytest.raises(StarkHipError, match=word) as e:
            engine.loo_launch(*bad)
        assert e.value.code == -1
    assert engine.loo_launch(100, 128, 1024)["G"] >= 1


def test_loo_from_hand_computed_totals():
    from stark_amd import engine
    e = np.array([-1.0, -2.5, -0.25, -4.0])
    lppd = np.array([-0.5, -2.0, -0.25, -3.0])
    p = lppd - e
    t = np.array([[2, lppd[:2].sum(), p[:2].sum(), e[:2].sum(), (e[:2] ** 2).sum(), 2, 1, 0],
                  [2, lppd[2:].sum(), p[2:].sum(), e[2:].sum(), (e[2:] ** 2).sum(), 1, 0, 0]])
    w = engine.loo(t)
    assert set(w) == {"n", "lppd", "p_loo", "elpd_loo", "se", "looic", "n_k_gt_0.5", "n_k_gt_0.7", "n_non_finite"}
    assert w["n"] == 4 and w["lppd"] == -5.75 and w["p_loo"] == 2.0 and w["elpd_loo"] == -7.75
    assert w["looic"] == 15.5 and w["n_k_gt_0.5"] == 3 and w["n_k_gt_0.7"] == 1 and w["n_non_finite"] == 0
    se = np.sqrt(4 / 3 * ((e ** 2).sum() - e.sum() ** 2 / 4))
    assert abs(w["se"] - se) < 1e-15 and abs(w["se"] - np.sqrt(4 * e.var(ddof=1))) < 1e-14
    # the same se formula as engine.waic
    assert w["se"] == engine.waic(np.concatenate([t[:, :5], np.zeros((2, 3))], axis=1))["se"]
    assert engine.loo(t[0]) == engine.loo(t[:1])                         # [8] and [1, 8]
    one = engine.loo([1, -0.7, 0.1, -0.8, 0.64, 1, 1, 0])
    assert one["n"] == 1 and one["se"] == 0.0 and one["elpd_loo"] == -0.8 and one["looic"] == 1.6
    bad = engine.loo([[3, np.nan, np.nan, np.nan, np.nan, 0, 0, 1]])
    assert bad["n_non_finite"] == 1 and np.isnan(bad["elpd_loo"]) and np.isnan(bad["se"])
    with pytest.raises(ValueError, match="8"):
        engine.loo(np.zeros((2, 7)))


def _driver(family_file, rows, K, monkeypatch):
    from stark_amd import stark
    from stark_amd.rdd import LocalContext

    def prep(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": K, "x": a[:, :K], "y": a[:, K].astype(np.int64)}

    def no_device(self, datas, q):
        raise AssertionError("a device call was reached")

    monkeypatch.setattr(stark.Stark, "_partition_loo_totals", no_device)
    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize(rows, 3), prep)
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", family_file))
    return st


def test_stark_loo_refuses_before_any_device_call(monkeypatch):
    rng = np.random.default_rng(4)
    K = 3
    rows = [tuple(r) for r in np.column_stack([rng.normal(size=(37, K)), rng.integers(0, 2, 37)])]
    st = _driver("logistic.stan", rows, K, monkeypatch)
    with pytest.raises(ValueError, match="pars= selection cannot be scored"):
        st.loo(np.zeros((K, 6)))                                        # a pars= selection: rows missing
    with pytest.raises(ValueError, match=r"S = 1025.*1024.*subset"):
        st.loo(np.zeros((K + 2, 1025)))
    with pytest.raises(AssertionError, match="a device call was reached"):   # S = 1024 goes through
        st.loo(np.zeros((K + 2, 1024)))
    sch = _driver("schools.stan", rows, K, monkeypatch)
    with pytest.raises(ValueError, match="schools"):
        sch.loo(np.zeros((K + 2, 6)))


def test_tail_length_in_integers_is_the_definition():
    """The library takes M = ceil(min(0.2 S, 3 sqrt S)) in integers (tests/test_gpu_loo.py restates it so);
    it is the floating-point formula for every S the sweep covers."""
    for S in range(1, 1025):
        M = min(-(-S // 5), math.isqrt(9 * S - 1) + 1)
        assert M == int(np.ceil(min(np.longdouble(S) / 5, 3 * np.sqrt(np.longdouble(S))))), S


def test_psis_math_check_builds_and_passes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "psis_math_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "psis_math_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "max error: elpd_loo" in r.stdout and "khat" in r.stdout
