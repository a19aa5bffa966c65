"""The categorical family (softmax regression) on the host (CPU only): the program recogniser (the two committed
programs, blanks and comments, both orders of the sum, the near-miss programs), data packing and its checks of y and
ncat, the extract() rows, the chain batches and the envelope predicate at its edges, the driver's refusals, and the
longdouble reference tests/categorical_ref.py itself against a finite difference and against the logistic density it
becomes at ncat = 2.
"""
import os

import numpy as np
import pytest

import categorical_ref as R
from stark_amd import frontend

HEAD = ("data { int<lower=0> N; int<lower=1> K; int<lower=2> ncat; matrix[N, K] x; int<lower=1, upper=ncat> y[N]; }\n")
HEAD_ARR = ("data { int<lower=0> N; int<lower=1> K; int<lower=2> ncat; matrix[N, K] x; array[N] int<lower=1, upper=ncat> y; }\n")
PARAMS = "parameters { vector[ncat - 1] alpha; vector[K * (ncat - 1)] beta; }\n"
ETA = "matrix[N, ncat - 1] eta = rep_matrix(alpha', N) + x * to_matrix(beta, K, ncat - 1);"
ETAS = [ETA, "matrix[N,ncat-1] eta=x*to_matrix(beta,K,ncat-1)+rep_matrix(alpha',N);",
        "matrix[ N , ncat - 1 ]  eta  =  x * to_matrix( beta , K , ncat - 1 )  +  rep_matrix( alpha' , N ) ;  /* eta */"]
LIK = "for (n in 1:N) y[n] ~ categorical_logit(append_row(eta[n]', 0));"
LIKS = [LIK, "for(n in 1:N)y[n]~categorical_logit(append_row(eta[n]',0));",
        "for (n in 1:N) {\n    y[n] ~ categorical_logit( append_row( eta[n]' , 0 ) );  // the reference class\n  }"]


def program(head=HEAD, params=PARAMS, eta=ETA, lik=LIK, priors="", extra=""):
    return head + params + extra + "model {\n  " + eta + "\n" + priors + "  " + lik + "  # classes\n}\n"


# ---------------------------------------------------------------- recognition
@pytest.mark.parametrize("head", [HEAD, HEAD_ARR], ids=["y[N]", "array[N]"])
@pytest.mark.parametrize("eta", ETAS, ids=["alpha-first", "x-first-tight", "x-first-wide"])
@pytest.mark.parametrize("lik", LIKS, ids=["plain", "tight", "braces"])
@pytest.mark.parametrize("priors,want", [
    ("", {}),
    ("  alpha ~ normal(0, 2.5);\n  beta ~ normal(0, 0.5);\n", {"alpha": 2.5, "beta": 0.5}),
], ids=["flat", "normal"])
def test_recognised(head, eta, lik, priors, want):
    code = program(head=head, eta=eta, lik=lik, priors=priors)
    assert frontend.program_info(code) == ("categorical", want)
    assert frontend.recognise(code) == "categorical"


def test_shipped_programs():
    d = os.path.join(os.path.dirname(frontend.__file__), "models")
    assert frontend.load_program_info(file=os.path.join(d, "categorical.stan")) == ("categorical", {})
    assert frontend.load_program_info(file=os.path.join(d, "categorical_prior.stan")) == \
        ("categorical", {"alpha": 10.0, "beta": 2.5})
    assert frontend.load_program_info(family="categorical", priors={"beta": 3.0}) == ("categorical", {"beta": 3.0})
    with pytest.raises(ValueError):
        frontend.load_program_info(family="categorial")
    # the families that were there are still told apart
    assert frontend.load_program_info(file=os.path.join(d, "logistic.stan"))[0] == "logistic"
    assert frontend.load_program_info(file=os.path.join(d, "gamma.stan")) == ("gamma", {})
    assert frontend.load_program_info(file=os.path.join(d, "schools.stan"))[0] == "schools"


REFUSED = {
    "matrix-beta": program(params="parameters { vector[ncat - 1] alpha; matrix[K, ncat - 1] beta; }\n",
                           eta="matrix[N, ncat - 1] eta = rep_matrix(alpha', N) + x * beta;"),
    "no-append-row": program(lik="for (n in 1:N) y[n] ~ categorical_logit(eta[n]');"),
    "softmax": program(lik="for (n in 1:N) y[n] ~ categorical(softmax(append_row(eta[n]', 0)));"),
    "offset": program(eta="matrix[N, ncat - 1] eta = rep_matrix(alpha', N) + x * to_matrix(beta, K, ncat - 1) + 1;"),
    "transformed-parameters": program(extra="transformed parameters { vector[ncat - 1] a2 = 2 * alpha; }\n"),
    "first-class-reference": program(lik="for (n in 1:N) y[n] ~ categorical_logit(append_row(0, eta[n]'));"),
    "row-major-beta": program(eta="matrix[N, ncat - 1] eta = rep_matrix(alpha', N) + x * to_matrix(beta, K, ncat - 1, 0);"),
    "beta-first": program(params="parameters { vector[K * (ncat - 1)] beta; vector[ncat - 1] alpha; }\n"),
    "y-from-zero": program(head=HEAD.replace("int<lower=1, upper=ncat> y[N]", "int<lower=0, upper=ncat> y[N]")),
    "shape-prior": program(priors="  shape ~ gamma(2, 0.5);\n"),
    "extra-statement": program(priors="  alpha[1] ~ normal(0, 1);\n"),
    "vector-x": program(head=HEAD.replace("matrix[N, K] x", "vector[N] x")),
    "no-K": program(head=HEAD.replace("int<lower=1> K; ", "")),
    "stray-braces": program(eta="{ " + ETA + " }"),
    "two-loops": program(priors="  " + LIK + "\n"),
}


@pytest.mark.parametrize("code", list(REFUSED.values()), ids=list(REFUSED))
def test_refused(code):
    with pytest.raises(NotImplementedError) as e:
        frontend.program_info(code)
    assert "'categorical'" in str(e.value)


# ---------------------------------------------------------------- data
def _data(y, ncat=3, n=4, d=2):
    return {"N": n, "K": d, "ncat": ncat, "x": np.arange(n * d, dtype=float).reshape(n, d), "y": y}


def test_pack_data():
    sh = frontend.pack_data("categorical", _data([1, 3, 2, 3]))
    assert sh["y"].dtype == np.int32 and sh["y"].tolist() == [1, 3, 2, 3] and sh["ncat"] == 3
    assert sh["x"].shape == (4, 2) and sh["x"].dtype == np.float64
    assert frontend.pack_data("categorical", _data(np.array([1.0, 2.0, 2.0, 1.0]), ncat=2))["y"].tolist() == [1, 2, 2, 1]
    for bad, word in (([0, 1, 2, 3], "y\\[0\\]"), ([1, 2, 3, 4], "y\\[3\\]"), ([1, 2.5, 3, 1], "y\\[1\\]"),
                      (["a", "b", "c", "d"], "integers")):
        with pytest.raises(ValueError, match=word):
            frontend.pack_data("categorical", _data(bad))
    with pytest.raises(ValueError, match="ncat"):
        frontend.pack_data("categorical", _data([1, 1, 1, 1], ncat=1))
    with pytest.raises(ValueError, match="ncat"):
        frontend.pack_data("categorical", _data([1, 1, 1, 1], ncat=2.5))
    d = _data([1, 2, 3, 1])
    del d["ncat"]
    with pytest.raises(ValueError, match="ncat"):
        frontend.pack_data("categorical", d)
    with pytest.raises(ValueError, match="N entries"):
        frontend.pack_data("categorical", _data([1, 2, 3]))


def test_rows():
    data = {"K": 2, "ncat": 4}
    cols = frontend.column_names("categorical", data)
    assert cols == ["alpha[1]", "alpha[2]", "alpha[3]", "beta[1]", "beta[2]", "beta[3]", "beta[4]", "beta[5]", "beta[6]", "lp__"]
    assert frontend.param_rows("categorical", data) == {"alpha": [0, 1, 2], "beta": [3, 4, 5, 6, 7, 8], "lp__": [9]}
    assert frontend.select_pars("categorical", data, None) is None
    assert frontend.select_pars("categorical", data, ["beta"]) == [3, 4, 5, 6, 7, 8, 9]
    assert frontend.select_pars("categorical", data, "alpha", include=False) == [3, 4, 5, 6, 7, 8, 9]
    assert frontend.select_pars("categorical", data, ["lp__", "alpha"]) == [0, 1, 2, 9]
    with pytest.raises(ValueError, match="No parameter sigma"):
        frontend.select_pars("categorical", data, ["sigma"])


# ---------------------------------------------------------------- chain batches, envelope, tables
@pytest.mark.parametrize("C,want", [(1, [1]), (15, [15]), (16, [16]), (17, [16, 1]), (35, [16, 16, 3])])
def test_chain_batches(C, want):
    from stark_amd import engine
    for d, ncat in ((1, 2), (5, 3), (128, 3), (16, 17), (64, 5)):
        assert engine.chain_batches(C, d, ncat=ncat) == want
    assert sum(want) == C


def test_envelope_edges():
    from stark_amd import _lib, engine
    sup = _lib.load().stk_categorical_supported
    # G ceil(d / 16) <= 16 with G <= 16: the corner of every K and one step past it
    for ncat, dmax in ((2, 256), (3, 128), (4, 80), (5, 64), (6, 48), (7, 32), (9, 32), (10, 16), (17, 16)):
        assert sup(ncat, dmax) == 1 and sup(ncat, dmax + 1) == 0, (ncat, dmax)
        assert sup(ncat, 1) == 1
    assert sup(18, 1) == 0 and sup(1, 4) == 0 and sup(0, 4) == 0 and sup(3, 0) == 0
    for ncat, d in ((18, 1), (3, 129), (17, 17), (5, 65)):
        with pytest.raises(engine.StarkHipError) as e:
            engine.chain_batches(4, d, ncat=ncat)
        assert "STK_E_ARG" in str(e.value) and f"K = {ncat}" in str(e.value) and f"d = {d}" in str(e.value)
    with pytest.raises(ValueError):
        engine.chain_batches(4, 8, sparse=True, ncat=3)
    # the tables the other families' batches come from are as they were
    assert engine.chain_batches(35, 100) == [16, 16, 2, 1]


def test_engine_tables_and_driver_refusals():
    from stark_amd import _lib, engine, stark
    assert engine.family_id("categorical") == 8 == _lib.STK_CATEGORICAL and engine.FAMILY_NAMES[8] == "categorical"
    assert engine.family_id("gamma") == 7 and engine.family_id(3) == 3
    q = stark._unconstrain("categorical", {"K": 2, "ncat": 3}, {"alpha": [0.5, -0.5], "beta": [1.0, -1.0, 2.0, -2.0]})
    assert np.array_equal(q, [0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    assert np.array_equal(stark._unconstrain("categorical", {"K": 3, "ncat": 4}, {}), np.zeros(12))
    for what in ("waic", "loo", "ppc", "bootstrap", "method='laplace'", "weights='laplace'"):
        with pytest.raises(ValueError, match="categorical"):
            stark._refuse_analysis("categorical", what)
    stark._refuse_analysis("logistic", "waic")
    from stark_amd.rdd import LocalContext
    sc = LocalContext()
    s = stark.Stark(sc, sc.parallelize([(0.0, 1)], 1), lambda part: {})
    s.setStanModel(family="categorical")
    for kw in ({"weights": "laplace"}, {"method": "laplace"}, {"method": "laplace", "combiner": "semiparametric"}):
        with pytest.raises(ValueError, match="categorical"):   # before any sampling: no device is touched
            s.concensusWeight(chains=2, iter=100, seed=1, **kw)
    # a model's ncat is validated before any device call
    with pytest.raises(ValueError, match="ncat"):
        engine.Model(None, "categorical", [{"x": np.zeros((2, 1)), "y": [1, 2]}])
    with pytest.raises(ValueError, match="ncat"):
        engine.Model(None, "categorical", [{"x": np.zeros((2, 1)), "y": [1, 2], "ncat": 2}, {"x": np.zeros((2, 1)), "y": [1, 2], "ncat": 3}])
    with pytest.raises(ValueError, match="ncat"):
        engine.Model(None, "categorical", [{"x": np.zeros((2, 1)), "y": [1, 2]}], ncat=1)
    with pytest.raises(ValueError, match="one model has one ncat"):   # ncat= against the shards' own entries
        engine.Model(None, "categorical", [{"x": np.zeros((2, 1)), "y": [1, 2], "ncat": 3}], ncat=2)
    with pytest.raises(ValueError, match="categorical family"):
        engine.Model(None, "logistic", [{"x": np.zeros((2, 1)), "y": [0, 1]}], ncat=2)


# ---------------------------------------------------------------- the reference itself
def _case(seed, n, d, ncat, C):
    rng = np.random.default_rng(seed)
    X = np.round(rng.uniform(-1.7, 1.7, (n, d)) * 64) / 64
    y = rng.integers(1, ncat + 1, n)
    q = np.round(rng.normal(0, 0.7, (C, (ncat - 1) * (d + 1))) * 1024) / 1024
    return X, y, q


def test_reference_gradient_is_the_derivative():
    X, y, q = _case(1, 23, 3, 4, 2)
    lp, g = R.ref_lpgrad(X, y, q, 4, prior=(2.0, 0.5))
    h = np.longdouble(1e-7)
    for j in range(q.shape[1]):
        qp, qm = q.astype(np.longdouble), q.astype(np.longdouble)
        qp[:, j] += h
        qm[:, j] -= h
        fd = (R.ref_lpgrad(X, y, qp, 4, prior=(2.0, 0.5))[0] - R.ref_lpgrad(X, y, qm, 4, prior=(2.0, 0.5))[0]) / (2 * h)
        assert np.all(np.abs(fd - g[:, j]) < 1e-9 * (1 + np.abs(g[:, j]))), j


def test_reference_is_logistic_at_two_classes():
    X, y, q = _case(2, 41, 5, 2, 3)
    lp, g = R.ref_lpgrad(X, y, q, 2)
    eta = q[:, :1].T + X @ q[:, 1:].T                      # (n, C)
    y1 = (y == 1).astype(float)[:, None]
    want = (y1 * eta - np.logaddexp(0.0, eta)).sum(0)
    sig = 1 / (1 + np.exp(-eta))
    assert np.allclose(lp.astype(float), want, rtol=1e-13, atol=0)
    assert np.allclose(g[:, 0].astype(float), (y1 - sig).sum(0), rtol=1e-12, atol=1e-13)
    assert np.allclose(g[:, 1:].astype(float), (y1 - sig).T @ X, rtol=1e-12, atol=1e-12)


def test_reference_relabelling():
    X, y, q = _case(3, 37, 2, 4, 2)
    lp, g = R.ref_lpgrad(X, y, q, 4)
    q2, y2 = R.swap_classes(q, y, 4, 2, 1, 3)
    lp2, g2 = R.ref_lpgrad(X, y2, q2, 4)
    g2b, _ = R.swap_classes(g2.astype(float), y, 4, 2, 1, 3)
    assert np.allclose(lp.astype(float), lp2.astype(float), rtol=1e-15)
    assert np.allclose(g.astype(float), g2b, rtol=1e-14, atol=1e-15)
