"""The Poisson (poisson_log) family on the host (CPU only): the program recogniser, data packing, the
extract() rows, the fingerprint's host twin with family word 4 and the chain batches.

The density the family computes (include/stark_hip.h), for the record of this file's GPU sibling
tests/test_gpu_poisson.py: eta = alpha + x . beta, mu = exp(eta), lp = sum(y eta - mu), d lp / d alpha =
sum(y - mu), d lp / d beta = x^T (y - mu) -- Stan 2.19's poisson_log_lpmf<propto = true>.
"""
import ctypes
import os

import numpy as np
import pytest

from stark_amd import frontend

HEAD_OLD = "data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; int<lower=0> y[N]; }\n"
HEAD_NEW = "data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; array[N] int<lower=0> y; }\n"
PARAMS = "parameters { real alpha; vector[K] beta; }\n"
PRIORS = "  alpha ~ normal(0, 2.5);\n  beta ~ normal(0, 0.5);\n"


def program(head=HEAD_OLD, params=PARAMS, lik="y ~ poisson_log(alpha + x * beta);", priors=""):
    return head + params + "model {\n" + priors + "  " + lik + "  // counts\n}\n"


# ---------------------------------------------------------------- recognition
@pytest.mark.parametrize("head", [HEAD_OLD, HEAD_NEW], ids=["y[N]", "array[N]"])
@pytest.mark.parametrize("lik", ["y ~ poisson_log(alpha + x * beta);", "y~poisson_log( x*beta + alpha ) ;"])
@pytest.mark.parametrize("priors", ["", PRIORS], ids=["flat", "priors"])
def test_recognised(head, lik, priors):
    fam, pri = frontend.program_info(program(head=head, lik=lik, priors=priors))
    assert fam == "poisson"
    assert pri == ({"alpha": 2.5, "beta": 0.5} if priors else {})
    assert frontend.recognise(program(head=head, lik=lik, priors=priors)) == "poisson"


def test_shipped_programs():
    d = os.path.join(os.path.dirname(frontend.__file__), "models")
    assert frontend.load_program_info(file=os.path.join(d, "poisson.stan")) == ("poisson", {})
    assert frontend.load_program_info(file=os.path.join(d, "poisson_prior.stan")) == ("poisson", {"alpha": 2.5, "beta": 1.0})
    assert frontend.load_program_info(family="poisson") == ("poisson", {})
    assert frontend.load_program_info(family="poisson", priors={"beta": 2.0}) == ("poisson", {"beta": 2.0})
    # the families that were there are still told apart
    assert frontend.load_program_info(file=os.path.join(d, "logistic.stan")) == ("logistic", {})
    assert frontend.load_program_info(file=os.path.join(d, "linear.stan"))[0] == "linear"


@pytest.mark.parametrize("code", [
    program(head=HEAD_OLD.replace("int<lower=0> y[N]", "real y[N]")),                       # real counts
    program(head=HEAD_OLD.replace("int<lower=0> y[N]", "int y[N]")),                        # no lower bound
    program(params="parameters { real alpha; vector[K] beta; real<lower=0> sigma; }\n"),    # a sigma
    program(lik="y ~ poisson(exp(alpha + x * beta));"),                                     # the exp() spelling
    program(lik="y ~ poisson_log_glm(x, alpha, beta);"),                                    # the glm form
    program(lik="y ~ poisson_log(alpha + x * beta + 1);"),                                  # an offset
], ids=["real-y", "unbounded-y", "sigma", "poisson-exp", "glm", "offset"])
def test_refused(code):
    with pytest.raises(NotImplementedError) as e:
        frontend.program_info(code)
    assert "poisson" in str(e.value) and "family='schools'|'linear'|'logistic'|'poisson'" in str(e.value)


def test_unknown_family_keyword():
    with pytest.raises(ValueError):
        frontend.load_program_info(family="poisson_log")


# ---------------------------------------------------------------- data
def _data(y, n=4, k=2):
    return {"N": n, "K": k, "x": np.arange(n * k, dtype=float).reshape(n, k), "y": y}


def test_pack_data():
    sh = frontend.pack_data("poisson", _data([0, 3, 2 ** 31 - 1, 7]))
    assert sh["y"].dtype == np.int32 and sh["y"].tolist() == [0, 3, 2 ** 31 - 1, 7]
    assert sh["x"].dtype == np.float64 and sh["x"].shape == (4, 2)
    sh = frontend.pack_data("poisson", _data(np.array([0.0, 3.0, 5.0, 1e9])))       # integer-valued floats
    assert sh["y"].dtype == np.int32 and sh["y"].tolist() == [0, 3, 5, 10 ** 9]


@pytest.mark.parametrize("bad", [-1, 0.5, 2 ** 31], ids=["negative", "fraction", "2^31"])
def test_pack_data_refuses(bad):
    with pytest.raises(ValueError):
        frontend.pack_data("poisson", _data([0, 3, bad, 7]))


def test_pack_data_wrong_length():
    with pytest.raises(ValueError):
        frontend.pack_data("poisson", _data([0, 3, 7]))


def test_rows_as_logistic():
    d = {"N": 5, "K": 3}
    assert frontend.column_names("poisson", d) == ["alpha", "beta[1]", "beta[2]", "beta[3]", "lp__"]
    assert frontend.column_names("poisson", d) == frontend.column_names("logistic", d)
    assert frontend.param_rows("poisson", d) == {"alpha": [0], "beta": [1, 2, 3], "lp__": [4]}
    assert frontend.select_pars("poisson", d, pars=["beta"]) == [1, 2, 3, 4]
    assert frontend.select_pars("poisson", d, pars=["beta"], include=False) == [0, 4]
    assert frontend.select_pars("poisson", d) is None
    with pytest.raises(ValueError):
        frontend.select_pars("poisson", d, pars=["sigma"])


def test_unconstrain_as_logistic():
    from stark_amd.stark import _unconstrain, sampling_config
    d = {"N": 5, "K": 3}
    init = {"alpha": 0.25, "beta": [1.0, -2.0, 3.0]}
    assert _unconstrain("poisson", d, init).tolist() == [0.25, 1.0, -2.0, 3.0]
    assert _unconstrain("poisson", d, {}).tolist() == [0.0] * 4
    assert np.array_equal(_unconstrain("poisson", d, init), _unconstrain("logistic", d, init))
    cfg = sampling_config("poisson", [d, d], iter=20, chains=3, init=0, seed=1)
    assert cfg["init"].shape == (2 * 3 * 4,) and not cfg["init"].any()


# ---------------------------------------------------------------- fingerprint (the header's formula)
MASK = (1 << 64) - 1
K = np.uint64(0x9E3779B97F4A7C15)
M = np.uint64(0xD6E8FEB86659FD93)
T = np.array([0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89, 0x452821E638D01377],
             np.uint64)


def fmix(a):
    a = a ^ (a >> np.uint64(32))
    a = a * M
    return a ^ (a >> np.uint64(29))


def words(a, tag):
    a = np.ascontiguousarray(a).reshape(-1)
    w = a.view(np.uint32).astype(np.uint64) if a.dtype == np.int32 else a.view(np.uint64)
    with np.errstate(over="ignore"):
        return int(fmix(w + np.arange(1, w.size + 1, dtype=np.uint64) * K + T[tag]).sum(dtype=np.uint64))


def fingerprint_twin(fam, x, y):
    """fmix(words([family, n, d], 0) + words(x, 1) + words(y_int, 3))."""
    acc = words(np.array([fam, x.shape[0], x.shape[1]], np.uint64), 0) + words(x, 1) + words(y, 3)
    with np.errstate(over="ignore"):
        return int(fmix(np.array([acc & MASK], np.uint64))[0])


@pytest.mark.parametrize("n,d", [(1, 1), (7, 3), (300, 20)])
def test_shard_fingerprint_family_word_4(n, d):
    from stark_amd import engine
    assert engine.FAMILIES["poisson"] == 4
    rng = np.random.default_rng(n)
    x = rng.normal(size=(n, d))
    y = rng.integers(0, 2, n).astype(np.int32)               # bits a logistic shard may hold too
    fp = int(engine.shard_fingerprint("poisson", {"x": x, "y": y}))
    assert fp == fingerprint_twin(4, x, y)
    assert fp == int(engine.shard_fingerprint(4, {"x": x, "y": y}))
    assert fp != int(engine.shard_fingerprint("logistic", {"x": x, "y": y}))
    assert int(engine.shard_fingerprint("logistic", {"x": x, "y": y})) == fingerprint_twin(3, x, y)
    y2 = rng.poisson(3e8, n).astype(np.int32)                # counts past 2^24: every bit of the int32 counts
    y2[0] = 2 ** 31 - 1
    assert int(engine.shard_fingerprint("poisson", {"x": x, "y": y2})) == fingerprint_twin(4, x, y2)


def test_host_shard_refuses_bad_counts():
    from stark_amd import engine
    x = np.zeros((3, 2))
    assert int(engine.shard_fingerprint("poisson", {"x": x, "y": [0.0, 1.0, 2.0]})) == \
        int(engine.shard_fingerprint("poisson", {"x": x, "y": [0, 1, 2]}))           # integer-valued floats are counts
    for y in ([0, -1, 2], [0.0, 1.5, 2.0], np.array([0, 2 ** 31, 1], np.int64), ["a", "b", "c"]):
        with pytest.raises(ValueError):
            engine.shard_fingerprint("poisson", {"x": x, "y": y})


def test_fingerprint_host_needs_y_int():
    from stark_amd import _lib
    x = np.zeros((3, 2))
    sh = _lib.Shard(3, 2, x.ctypes.data, None, None, None)
    out = ctypes.c_uint64()
    assert _lib.load().stk_shard_fingerprint_host(4, ctypes.byref(sh), ctypes.byref(out)) == -1
    assert b"poisson needs y_int" in _lib.load().stk_last_error()
    # counts go in y_int alone: a shard that also carries doubles (y) or a sigma is refused, not half read
    yi, yd = np.zeros(3, np.int32), np.zeros(3)
    ok = _lib.Shard(3, 2, x.ctypes.data, None, yi.ctypes.data, None)
    assert _lib.load().stk_shard_fingerprint_host(4, ctypes.byref(ok), ctypes.byref(out)) == 0
    for extra in (_lib.Shard(3, 2, x.ctypes.data, yd.ctypes.data, yi.ctypes.data, None),
                  _lib.Shard(3, 2, x.ctypes.data, None, yi.ctypes.data, yd.ctypes.data)):
        assert _lib.load().stk_shard_fingerprint_host(4, ctypes.byref(extra), ctypes.byref(out)) == -1
        assert b"y and sigma must be NULL" in _lib.load().stk_last_error()
    assert _lib.load().stk_shard_fingerprint_host(5, ctypes.byref(sh), ctypes.byref(out)) == -1


# ---------------------------------------------------------------- the batches and launch shapes are the family's too
def test_chain_batches_unchanged():
    from stark_amd import engine
    assert engine.chain_batches(3, 100) == [2, 1]
    assert engine.chain_batches(17, 100) == [16, 1]
    assert engine.chain_batches(70, 100) == [64, 4, 2]
    assert engine.chain_batches(20, 104) == [16, 4]
    assert engine.chain_batches(70, 1001) == [64, 4, 2]
    assert engine.chain_batches(16, 129) == [16]
