"""Host side of the metric choice (diag_e / dense_e / unit_e): the pystan control block through
stark.sampling_config, engine.make_config's shape checks and the C struct's new tail."""
import ctypes

import numpy as np
import pytest


def test_sampling_config_maps_the_three_metric_names():
    from stark_amd import stark
    datas = [{"N": 3, "K": 2}]
    assert stark.sampling_config("linear", datas, seed=1)["metric"] == "diag_e"
    for name in ("diag_e", "dense_e", "unit_e"):
        cfg = stark.sampling_config("linear", datas, seed=1, control={"metric": name, "adapt_delta": 0.9})
        assert cfg["metric"] == name and cfg["adapt_delta"] == 0.9
    for bad in ("dense", "diag", "DENSE_E", "", None, 1):
        with pytest.raises(ValueError, match="metric"):
            stark.sampling_config("linear", datas, seed=1, control={"metric": bad})


def test_sampling_config_passes_a_2d_inv_metric_through():
    from stark_amd import stark
    im = np.eye(4) + 0.1
    cfg = stark.sampling_config("linear", [{"N": 3, "K": 2}], seed=1, control={"metric": "dense_e", "inv_metric": im})
    assert cfg["inv_metric"] is im and cfg["metric"] == "dense_e"


def test_make_config_sets_the_struct_tail():
    from stark_amd import _lib, engine
    assert [n for n, _ in _lib.Config._fields_][-2:] == ["metric", "inv_metric_dense"]
    d = _lib.default_config()
    assert d.metric == 0 and not d.inv_metric_dense          # the defaults keep diag_e
    im = np.eye(3) * 2.0
    c = engine.make_config(metric="dense_e", inv_metric=im)
    assert c.metric == 1 and c.inv_metric_dense == c._keep[-1].ctypes.data and not c.inv_metric
    np.testing.assert_array_equal(np.ctypeslib.as_array(ctypes.cast(c.inv_metric_dense, ctypes.POINTER(ctypes.c_double)),
                                                        (9,)), im.ravel())
    assert engine.make_config(metric="unit_e").metric == 2
    v = np.arange(1.0, 4.0)
    c = engine.make_config(inv_metric=v)
    assert c.metric == 0 and c.inv_metric and not c.inv_metric_dense


def test_make_config_refuses_wrong_shapes_and_names():
    from stark_amd import engine
    with pytest.raises(ValueError, match="metric must be one of"):
        engine.make_config(metric="full")
    with pytest.raises(ValueError, match="square 2-D"):
        engine.make_config(metric="dense_e", inv_metric=np.ones(4))
    with pytest.raises(ValueError, match="square 2-D"):
        engine.make_config(metric="dense_e", inv_metric=np.ones((3, 4)))
    with pytest.raises(ValueError, match="1-D"):
        engine.make_config(metric="diag_e", inv_metric=np.eye(3))
    with pytest.raises(ValueError, match="no inv_metric"):
        engine.make_config(metric="unit_e", inv_metric=np.ones(3))


def test_library_exports_the_dense_entry_points():
    from stark_amd import _lib
    lib = _lib.load()
    assert lib.stk_sampler_adaptation_dense and lib.stk_transition_dense and lib.stk_sampler_metric_factor_dense
