"""Sparse design matrices, the parts that need no GPU: the canonical CSR triple, the validation errors (through the
host fingerprint twin, which runs the checks of stk_model_create_sparse), the sparse batch table and launch shape,
the host fingerprint, and the driver's refusals on sparse data."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT


# ---------------------------------------------------------------- canonicalisation
def _triple_eq(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_every_input_format_gives_the_same_canonical_triple():
    """COO with duplicates and an explicit zero, CSC, CSR with unsorted indices, and the raw triple: one (indptr int64,
    indices int32, values float64), indices sorted, duplicates summed, the explicit zero kept."""
    from stark_amd import engine
    r = np.array([0, 0, 2, 2, 2, 1, 3, 3])
    c = np.array([3, 1, 0, 0, 4, 2, 4, 0])
    v = np.array([1.0, 2.0, 3.0, 4.5, 5.0, 0.0, -1.25, 8.0])       # (2, 0) twice: 3 + 4.5; (1, 2) an explicit zero
    coo = sp.coo_matrix((v, (r, c)), shape=(5, 6))
    want = (np.array([0, 2, 3, 5, 7, 7], np.int64), np.array([1, 3, 2, 0, 4, 0, 4], np.int32),
            np.array([2.0, 1.0, 0.0, 7.5, 5.0, 8.0, -1.25]), 6)
    got = engine.canonical_csr({"x": coo})
    assert _triple_eq(got, want), got
    assert _triple_eq(engine.canonical_csr({"x": coo.tocsc()}), want)
    assert _triple_eq(engine.canonical_csr({"x": coo.tocsr()}), want)
    unsorted = sp.csr_matrix((np.array([1.0, 2.0, 0.0, 5.0, 3.0, 4.5, -1.25, 8.0]), np.array([3, 1, 2, 4, 0, 0, 4, 0]),
                              np.array([0, 2, 3, 6, 8, 8])), shape=(5, 6))
    assert _triple_eq(engine.canonical_csr({"x": unsorted}), want)
    raw = {"x_csr": ([0, 2, 3, 6, 8, 8], [3, 1, 2, 4, 0, 0, 4, 0], [1.0, 2.0, 0.0, 5.0, 3.0, 4.5, -1.25, 8.0]), "d": 6}
    assert _triple_eq(engine.canonical_csr(raw), want)
    assert engine.is_sparse_shard({"x": coo}) and engine.is_sparse_shard(raw) and not engine.is_sparse_shard({"x": coo.toarray()})
    empty = engine.canonical_csr({"x": sp.csr_matrix((3, 4))})
    assert _triple_eq(empty, (np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0), 4))


# ---------------------------------------------------------------- validation: every error names its shard and row
def _fp_raw(indptr, indices, values, d, y, family=3):
    """stk_shard_fingerprint_sparse_host on a raw triple (no canonicalisation): (rc, message or value)."""
    from stark_amd import _lib
    ip, ix, vv = np.asarray(indptr, np.int64), np.asarray(indices, np.int32), np.asarray(values, np.float64)
    yy = np.asarray(y, np.int32)
    sh = _lib.ShardSparse(len(ip) - 1, d, ip.ctypes.data, ix.ctypes.data, vv.ctypes.data, None, yy.ctypes.data)
    out = ctypes.c_uint64()
    rc = _lib.load().stk_shard_fingerprint_sparse_host(family, ctypes.byref(sh), ctypes.byref(out))
    return rc, (_lib.load().stk_last_error().decode() if rc else out.value)


GOOD = ([0, 2, 3, 6, 6], [1, 3, 2, 0, 1, 4], [1.0, 2.0, 0.5, 3.0, 4.0, 5.0])
Y4 = [0, 1, 1, 0]


@pytest.mark.parametrize("what,indptr,indices,values,message", [
    ("an index equal to d", GOOD[0], [1, 5, 2, 0, 1, 4], GOOD[2], r"shard 0: row 0: index 5 is outside \[0, 5\)"),
    ("a negative index", GOOD[0], [1, 3, -2, 0, 1, 4], GOOD[2], r"shard 0: row 1: index -2 is outside \[0, 5\)"),
    ("a decreasing indptr", [0, 2, 1, 6, 6], GOOD[1], GOOD[2], r"shard 0: row 1: indptr decreases \(1 after 2\)"),
    ("indptr not from 0", [1, 2, 3, 6, 6], GOOD[1], GOOD[2], r"shard 0: row 0: indptr\[0\] = 1"),
    ("unsorted indices", GOOD[0], [1, 3, 2, 1, 0, 4], GOOD[2], r"shard 0: row 2: indices must be strictly increasing .*\(0 after 1\)"),
    ("a duplicate index", GOOD[0], [1, 3, 2, 0, 0, 4], GOOD[2], r"shard 0: row 2: indices must be strictly increasing .*\(0 after 0\)"),
    ("a NaN value", GOOD[0], GOOD[1], [1.0, 2.0, 0.5, 3.0, np.nan, 5.0], r"shard 0: row 2: the value at column 1 is not finite"),
    ("an infinite value", GOOD[0], GOOD[1], [1.0, np.inf, 0.5, 3.0, 4.0, 5.0], r"shard 0: row 0: the value at column 3 is not finite"),
])
def test_validation_errors_name_shard_and_row(what, indptr, indices, values, message):
    import re
    assert _fp_raw(*GOOD, 5, Y4)[0] == 0
    rc, msg = _fp_raw(indptr, indices, values, 5, Y4)
    assert rc == -1 and re.search(message, msg), (what, rc, msg)


def test_validation_through_the_python_layer():
    """engine.shard_fingerprint on a sparse shard: an out-of-range index is left for the library to name (the Python
    layer sorts and sums, it does not clip); the y rules are the dense path's."""
    from stark_amd import engine
    bad = {"x_csr": (GOOD[0], [1, 5, 2, 0, 1, 4], GOOD[2]), "d": 5, "y": Y4}
    with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG: shard 0: row 0: index 5 is outside \[0, 5\)"):
        engine.shard_fingerprint("logistic", bad)
    with pytest.raises(ValueError, match="y must be 0 or 1"):
        engine.shard_fingerprint("logistic", {"x_csr": GOOD, "d": 5, "y": [0, 2, 1, 0]})
    with pytest.raises(ValueError, match="row counts differ"):
        engine.shard_fingerprint("logistic", {"x_csr": GOOD, "d": 5, "y": [0, 1, 1]})
    rc, msg = _fp_raw(*GOOD, 5, Y4, family=1)
    assert rc == -1 and "schools" in msg


# ---------------------------------------------------------------- host-only function tables
def _greedy(C, sizes):
    out = []
    for s in sizes:
        while C >= s:
            out.append(s)
            C -= s
    return out


@pytest.mark.parametrize("C", [3, 17, 31, 70])
def test_sparse_chain_batches_are_a_table_in_C_and_d(C):
    """Greedy, largest first, over {16, 8, 4, 2, 1} up to d = 512 and {8, 4, 2, 1} past it, up to 1024: both sides of
    each edge of the table.  The dense table is what it was."""
    from stark_amd import engine
    for d in (1, 2, 128, 129, 511, 512):
        assert engine.chain_batches(C, d, sparse=True) == _greedy(C, [16, 8, 4, 2, 1]), d
    for d in (513, 514, 1023, 1024):
        assert engine.chain_batches(C, d, sparse=True) == _greedy(C, [8, 4, 2, 1]), d
    for d in (0, 1025):
        with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
            engine.chain_batches(C, d, sparse=True)
    for d in (1, 128, 129, 512, 513, 1024):                                       # stk_chain_batches is unchanged
        assert engine.chain_batches(C, d) == _greedy(C, [64, 16, 8, 4, 2, 1]), d
        assert engine.chain_batches(C, d, sparse=False) == engine.chain_batches(C, d)
    assert sum(engine.chain_batches(C, 700, sparse=True)) == C


def test_sparse_launch_is_a_function_of_its_arguments():
    from stark_amd import engine
    a = engine.sparse_launch(200000, 128, 8, 16)
    assert a == engine.sparse_launch(200000, 128, 8, 16)
    assert a["kind"] == 7 and a["T"] == 64 and a["G"] == 98 and a["staged"] == 1 and a["ell_bytes"] == 12 * 8 * 200000
    assert a["lds_bytes"] <= 80 * 1024 and a["copies"] == 2                       # two blocks per CU
    # the chunks are a function of n alone
    for d, K, C in ((1, 0, 1), (16, 16, 4), (512, 40, 16), (1024, 1024, 8)):
        assert engine.sparse_launch(200000, d, K, C)["G"] == 98
        assert engine.sparse_launch(1, d, K, C)["G"] == 1 and engine.sparse_launch(2049, d, K, C)["G"] == 2
        assert engine.sparse_launch(10 ** 8, d, K, C)["G"] == 512
        assert engine.sparse_launch(77, d, K, C)["lds_bytes"] <= 160 * 1024
    # a tile's entries are staged while 12 K T bytes fit the 16 KiB stage: the bits do not depend on it
    assert engine.sparse_launch(77, 512, 21, 16)["staged"] == 1 and engine.sparse_launch(77, 512, 22, 16)["staged"] == 0
    assert engine.sparse_launch(77, 512, 512, 16)["lds_bytes"] == 160 * 1024 and engine.sparse_launch(77, 1024, 9, 8)["copies"] == 1
    assert engine.sparse_launch(77, 16, 4, 16)["copies"] == 4
    for bad in ((77, 513, 8, 16), (77, 128, 8, 64), (77, 128, 8, 3), (77, 128, 129, 8), (0, 128, 8, 8), (77, 1025, 8, 1)):
        with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
            engine.sparse_launch(*bad)
    # the dense launch info keeps its meaning: no kind 7 from it
    assert engine.sweep_launch(200000, 128, 16)["kind"] == 4 and engine.sweep_launch(200000, 1024, 8)["kind"] == 1


# ---------------------------------------------------------------- the host fingerprint twin
def test_sparse_fingerprint_host_twin():
    """It changes with one flipped index, one flipped value, one moved padding boundary and with K; it never equals
    the dense twin of the same matrix."""
    from stark_amd import engine
    y = np.array(Y4, np.int32)
    base = _fp_raw(*GOOD, 5, y)[1]
    assert base == _fp_raw(*GOOD, 5, y)[1]
    assert base == int(engine.shard_fingerprint("logistic", {"x_csr": GOOD, "d": 5, "y": y}))
    flipped_index = _fp_raw(GOOD[0], [1, 3, 2, 0, 2, 4], GOOD[2], 5, y)[1]
    flipped_value = _fp_raw(GOOD[0], GOOD[1], [1.0, 2.0, 0.5, 3.0, 4.0000000000000009, 5.0], 5, y)[1]
    moved_boundary = _fp_raw([0, 1, 3, 6, 6], [1, 2, 3, 0, 1, 4], GOOD[2], 5, y)[1]   # row 0 loses an entry to row 1
    wider = _fp_raw([0, 2, 3, 6, 10], GOOD[1] + [0, 1, 2, 3], GOOD[2] + [0.0] * 4, 5, y)[1]   # K = 4: explicit zeros
    other_y = _fp_raw(*GOOD, 5, [0, 1, 0, 0])[1]
    other_d = _fp_raw(*GOOD, 6, y)[1]
    vals = [base, flipped_index, flipped_value, moved_boundary, wider, other_y, other_d]
    assert len(set(vals)) == len(vals), vals
    X = sp.csr_matrix((GOOD[2], GOOD[1], GOOD[0]), shape=(4, 5))
    dense = int(engine.shard_fingerprint("logistic", {"x": X.toarray(), "y": y}))
    assert int(engine.shard_fingerprint("logistic", {"x": X, "y": y})) == base != dense
    # an all-zero matrix (K = 0) against the dense zeros
    z = int(engine.shard_fingerprint("linear", {"x": sp.csr_matrix((4, 5)), "y": np.arange(4.0)}))
    assert z != int(engine.shard_fingerprint("linear", {"x": np.zeros((4, 5)), "y": np.arange(4.0)}))
    # the public word fingerprint keeps its tags 0..4: the padded rows' tags are the library's own
    with pytest.raises(engine.StarkHipError, match="tag must be in 0..4"):
        engine.fingerprint_words(np.zeros(3), 5)


# ---------------------------------------------------------------- the driver's refusals, before a model is built
def test_driver_refuses_the_analysis_calls_on_sparse_data(monkeypatch):
    from stark_amd import engine, frontend, stark
    from stark_amd.rdd import LocalContext
    d = 6
    rng = np.random.default_rng(0)
    rows = [(int(rng.integers(0, d)), int(rng.integers(0, 2))) for _ in range(200)]

    def prep(data):
        X = sp.csr_matrix((np.ones(len(data)), (np.arange(len(data)), [r[0] for r in data])), shape=(len(data), d))
        return {"N": len(data), "K": d, "x": X, "y": [r[1] for r in data]}

    packed = frontend.pack_data("logistic", prep(rows))
    assert engine.is_sparse_shard(packed) and packed["y"].dtype == np.int32            # passed through, y checked
    with pytest.raises(ValueError, match="N = 201"):
        frontend.pack_data("logistic", dict(prep(rows), N=201))
    with pytest.raises(ValueError, match="0 and 1"):
        frontend.pack_data("logistic", dict(prep(rows), y=[2] * 200))
    sc = LocalContext()
    st = stark.Stark(sc, sc.parallelize(rows, 2), prep)
    st.setStanModel(file=os.path.join(ROOT, "stark_amd", "models", "logistic.stan"))

    def boom(*a, **k):
        raise AssertionError("a model was built")

    monkeypatch.setattr(engine, "Model", boom)
    samples = np.zeros((d + 2, 40))
    for what, call in (("waic", lambda: st.waic(samples)), ("loo", lambda: st.loo(samples)), ("ppc", lambda: st.ppc(samples)),
                       ("bootstrap", lambda: st.bootstrap(n=16)),
                       ("weights='laplace'", lambda: st.concensusWeight(weights="laplace", iter=100, seed=1)),
                       ("method='laplace'", lambda: st.concensusWeight(method="laplace", iter=100, seed=1))):
        with pytest.raises(ValueError, match="sparse") as ei:
            call()
        assert what.split("=")[0] in str(ei.value), (what, str(ei.value))
