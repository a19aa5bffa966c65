"""The negative-binomial (neg_binomial_2_log) family on the host (CPU only): the program recogniser, data
packing, the extract() rows, the init mapping, the fingerprint's host twin with family word 5, the phi-only
table sums of stk_negbin_phi_terms_host (the code the reduce kernel runs) against the longdouble reference
tests/negbin_ref.py, the reference's two evaluations against each other, and the phi -> inf limit of the
restated density against Poisson's.
"""
import os

import numpy as np
import pytest

import negbin_ref as R
from stark_amd import frontend
from test_host_poisson import fingerprint_twin

HEAD_OLD = "data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; int<lower=0> y[N]; }\n"
HEAD_NEW = "data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; array[N] int<lower=0> y; }\n"
PARAMS = "parameters { real alpha; vector[K] beta; real<lower=0> phi; }\n"
LIK = "y ~ neg_binomial_2_log(alpha + x * beta, phi);"
PINNED = "family='schools'|'linear'|'logistic'|'poisson'"


def program(head=HEAD_OLD, params=PARAMS, lik=LIK, priors=""):
    return head + params + "model {\n" + priors + "  " + lik + "  // overdispersed counts\n}\n"


# ---------------------------------------------------------------- recognition
@pytest.mark.parametrize("head", [HEAD_OLD, HEAD_NEW], ids=["y[N]", "array[N]"])
@pytest.mark.parametrize("lik", [LIK, "y~neg_binomial_2_log( x*beta + alpha , phi ) ;"])
@pytest.mark.parametrize("priors,want", [
    ("", {}),
    ("  alpha ~ normal(0, 2.5);\n  beta ~ normal(0, 0.5);\n  phi ~ gamma(2, 0.5);\n", {"alpha": 2.5, "beta": 0.5, "phi": (2.0, 0.5)}),
    ("  phi ~ exponential(0.25);\n", {"phi": (1.0, 0.25)}),
    ("  phi ~ gamma(1.5e0, .5);\n  beta ~ normal(0, 1);\n", {"beta": 1.0, "phi": (1.5, 0.5)}),
], ids=["flat", "all", "exponential", "gamma-beta"])
def test_recognised(head, lik, priors, want):
    fam, pri = frontend.program_info(program(head=head, lik=lik, priors=priors))
    assert fam == "neg_binomial" and pri == want
    assert frontend.recognise(program(head=head, lik=lik, priors=priors)) == "neg_binomial"


def test_shipped_programs():
    d = os.path.join(os.path.dirname(frontend.__file__), "models")
    assert frontend.load_program_info(file=os.path.join(d, "neg_binomial.stan")) == ("neg_binomial", {})
    assert frontend.load_program_info(file=os.path.join(d, "neg_binomial_prior.stan")) == \
        ("neg_binomial", {"alpha": 2.5, "beta": 1.0, "phi": (2.0, 0.5)})
    assert frontend.load_program_info(family="neg_binomial", priors={"phi": (2.0, 1.0)}) == ("neg_binomial", {"phi": (2.0, 1.0)})
    # the families that were there are still told apart
    assert frontend.load_program_info(file=os.path.join(d, "poisson.stan")) == ("poisson", {})
    assert frontend.load_program_info(file=os.path.join(d, "linear.stan"))[0] == "linear"


@pytest.mark.parametrize("code", [
    program(lik="y ~ neg_binomial_2(exp(alpha + x * beta), phi);"),                              # the exp() spelling
    program(lik="y ~ neg_binomial_2_log_glm(x, alpha, beta, phi);"),                             # the glm form
    program(params="parameters { real alpha; vector[K] beta; real<lower=0> inv_phi; }\n",
            lik="y ~ neg_binomial_2_log(alpha + x * beta, 1 / inv_phi);"),                       # reciprocal dispersion
    program(params="parameters { real alpha; vector[K] beta; real<lower=0> inv_phi; }\n"
                   "transformed parameters { real phi = 1 / inv_phi; }\n"),                      # the same, transformed
    program(priors="  phi ~ lognormal(0, 1);\n"),                                                # another phi prior
    program(priors="  phi ~ normal(0, 5);\n"),
    program(priors="  phi ~ gamma(2, 0.5);\n  phi ~ exponential(1);\n"),                         # two phi priors
    program(priors="  phi ~ gamma(0, 0.5);\n"),                                                  # shape 0
    program(params="parameters { real alpha; vector[K] beta; real phi; }\n"),                    # phi unbounded
    program(head=HEAD_OLD.replace("int<lower=0> y[N]", "int y[N]")),                             # counts unbounded
    program(lik="y ~ neg_binomial_2_log(alpha + x * beta + 1, phi);"),                           # an offset
    program(lik="y ~ poisson_log(alpha + x * beta);", params="parameters { real alpha; vector[K] beta; }\n",
            priors="  phi ~ gamma(2, 0.5);\n"),                                                  # a phi prior elsewhere
], ids=["nb2-exp", "glm", "inv-phi", "inv-phi-tp", "lognormal", "normal-phi", "two-priors", "shape0", "phi-unbounded",
        "y-unbounded", "offset", "poisson-phi"])
def test_refused(code):
    with pytest.raises(NotImplementedError) as e:
        frontend.program_info(code)
    assert PINNED in str(e.value) and PINNED + "|'neg_binomial'" in str(e.value)


def test_unknown_family_keyword():
    with pytest.raises(ValueError):
        frontend.load_program_info(family="neg_binomial_2_log")


# ---------------------------------------------------------------- data, rows, init
def _data(y, n=4, k=2):
    return {"N": n, "K": k, "x": np.arange(n * k, dtype=float).reshape(n, k), "y": y}


def test_pack_data():
    sh = frontend.pack_data("neg_binomial", _data([0, 3, 2 ** 31 - 1, 7]))
    assert sh["y"].dtype == np.int32 and sh["y"].tolist() == [0, 3, 2 ** 31 - 1, 7]
    assert sh["x"].dtype == np.float64 and sh["x"].shape == (4, 2)
    sh = frontend.pack_data("neg_binomial", _data(np.array([0.0, 3.0, 5.0, 1e9])))
    assert sh["y"].dtype == np.int32 and sh["y"].tolist() == [0, 3, 5, 10 ** 9]


@pytest.mark.parametrize("bad", [-1, 0.5, 2 ** 31], ids=["negative", "fraction", "2^31"])
def test_pack_data_refuses(bad):
    with pytest.raises(ValueError) as e:
        frontend.pack_data("neg_binomial", _data([0, 3, bad, 7]))
    assert "neg_binomial_2_log" in str(e.value)
    with pytest.raises(ValueError):
        frontend.pack_data("neg_binomial", _data([0, 3, 7]))


def test_rows_as_linear_with_phi():
    d = {"N": 5, "K": 3}
    assert frontend.column_names("neg_binomial", d) == ["alpha", "beta[1]", "beta[2]", "beta[3]", "phi", "lp__"]
    assert frontend.param_rows("neg_binomial", d) == {"alpha": [0], "beta": [1, 2, 3], "phi": [4], "lp__": [5]}
    assert frontend.select_pars("neg_binomial", d, pars=["phi"]) == [4, 5]
    assert frontend.select_pars("neg_binomial", d, pars=["beta"], include=False) == [0, 4, 5]
    assert frontend.select_pars("neg_binomial", d) is None
    with pytest.raises(ValueError):
        frontend.select_pars("neg_binomial", d, pars=["sigma"])


def test_unconstrain():
    from stark_amd.stark import _unconstrain, sampling_config, unconstrain_draws
    d = {"N": 5, "K": 3}
    init = {"alpha": 0.25, "beta": [1.0, -2.0, 3.0], "phi": 4.0}
    assert np.array_equal(_unconstrain("neg_binomial", d, init), np.array([0.25, 1.0, -2.0, 3.0, np.log(4.0)]))
    assert _unconstrain("neg_binomial", d, {}).tolist() == [0.0] * 5          # phi = 1
    cfg = sampling_config("neg_binomial", [d, d], iter=20, chains=3, init=0, seed=1)
    assert cfg["init"].shape == (2 * 3 * 5,) and not cfg["init"].any()
    m = np.array([[0.1, 0.2], [1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [2.0, 0.5], [-7.0, -8.0]])   # alpha, beta x3, phi, lp__
    q = unconstrain_draws("neg_binomial", m)
    assert q.shape == (2, 5) and np.array_equal(q[:, :4], m[:4].T) and np.array_equal(q[:, 4], np.log(m[4]))
    m[4, 1] = 0.0
    with pytest.raises(ValueError) as e:
        unconstrain_draws("neg_binomial", m)
    assert "phi" in str(e.value)


def test_driver_refusals_name_the_family():
    """waic, loo, ppc, bootstrap, weights='laplace', method='laplace' (both combiners) and full-data mode refuse the
    family by name before any sampling: no device is touched here."""
    from stark_amd import engine, fulldata, stark
    from stark_amd.rdd import LocalContext
    sc = LocalContext()
    rows = [(0.1 * i, i % 3) for i in range(8)]

    def prep(part):   # never reached
        raise AssertionError("sampled before refusing")

    st = stark.Stark(sc, sc.parallelize(rows, 2), prep)
    st.setStanModel(model_code=program(priors="  phi ~ gamma(2, 0.5);\n"))
    assert st.family == "neg_binomial" and st.priors == {"phi": (2.0, 0.5)}
    draws = np.ones((4, 10))
    for call in (lambda: st.waic(draws), lambda: st.loo(draws), lambda: st.ppc(draws), lambda: st.bootstrap(n=4),
                 lambda: st.concensusWeight(weights="laplace"), lambda: st.concensusWeight(method="laplace"),
                 lambda: st.concensusWeight(method="laplace", combiner="semiparametric")):
        with pytest.raises(ValueError) as e:
            call()
        assert "neg_binomial" in str(e.value)

    class FakeModel:
        family = engine.FAMILIES["neg_binomial"]
        nshards = 1

    with pytest.raises(ValueError) as e:
        fulldata.FullDataSampler(FakeModel())
    assert "neg_binomial" in str(e.value)


# ---------------------------------------------------------------- fingerprint (the header's formula)
@pytest.mark.parametrize("n,d", [(1, 1), (7, 3), (300, 20)])
def test_shard_fingerprint_family_word_5(n, d):
    from stark_amd import engine
    assert engine.FAMILIES["neg_binomial"] == 5
    rng = np.random.default_rng(n)
    x = rng.normal(size=(n, d))
    y = rng.negative_binomial(1.5, 1e-8, n).astype(np.int32)             # counts past 2^24
    y[0] = 2 ** 31 - 1
    fp = int(engine.shard_fingerprint("neg_binomial", {"x": x, "y": y}))
    assert fp == fingerprint_twin(5, x, y)
    assert fp == int(engine.shard_fingerprint(5, {"x": x, "y": y}))
    assert fp != int(engine.shard_fingerprint("poisson", {"x": x, "y": y}))
    assert int(engine.shard_fingerprint("poisson", {"x": x, "y": y})) == fingerprint_twin(4, x, y)
    for bad in ([0, -1, 2], [0.0, 1.5, 2.0]):
        with pytest.raises(ValueError):
            engine.shard_fingerprint("neg_binomial", {"x": np.zeros((3, 2)), "y": bad})


# ---------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("phi", [1e-6, 0.3, 17.5, 1e4, 1e9])
@pytest.mark.parametrize("y", [1100, 2500, 4096])
def test_reference_series_against_finite_sums(phi, y):
    """Where both apply (a count whose finite sum is affordable, the series started at 1024): the finite sum
    against finite sum to 1024 + series.  Longdouble: 1e-17 of the terms' size (64 ulp of the 64-bit mantissa
    on sums of up to 4096 terms, each with a rounded log1p)."""
    a_fin, s_fin = R.finite_sums(y, phi)
    a0, s0 = R.finite_sums(1024, phi)
    ta, ts = R.series_tail(1024, y, phi)
    size = y * (1 + float(np.log1p(R.L(y) / R.L(phi))))       # |x1 L1| + M, the size of the cancelling terms
    assert abs(float(a0 + ta - a_fin)) <= 1e-17 * 4096 * size
    assert abs(float(s0 + ts - s_fin)) <= 1e-17 * 4096 * float(s_fin)


def test_reference_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    for phi, y in [(1e-3, 7), (0.3, 2000), (17.5, 2 ** 31 - 1), (1e9, 100000)]:
        a1, s2 = R.count_terms(y, phi)
        p = mp.mpf(phi)
        ea = mp.loggamma(y + p) - mp.loggamma(p) - y * mp.log(p)
        es = mp.digamma(y + p) - mp.digamma(p)
        assert abs(mp.mpf(float(a1)) + mp.mpf(float(a1 - R.L(float(a1)))) - ea) <= mp.mpf(1e-16) * (abs(ea) + y)
        assert abs(mp.mpf(float(s2)) - es) <= mp.mpf(4e-16) * abs(es)


# ---------------------------------------------------------------- the library's table sums
def _tol(y, phi, a1, s2):
    """What fp64 can be asked: every table entry's term has a few ulp (a division, a log1p, a product) and the
    N = min(max y, 1024) + #{distinct y > 1024} entries are added one by one, all of one sign: (N + 8) 8 eps of
    the sums.  A count past the cap adds 8 eps of the size of the terms whose difference it is, m (x1 L(y) + x0
    L(1024) + M) -- at phi >> y these cancel to M^2 / phi, so that part of the bound is absolute."""
    eps = np.finfo(np.float64).eps
    vals, mult = np.unique(np.asarray(y, np.int64), return_counts=True)
    big = vals > 1024
    N = int(min(vals.max(), 1024)) + int(big.sum())
    size = sum(float(m) * (2.0 * (v + phi) * np.log1p(v / phi) + v) for v, m in zip(vals[big], mult[big]))
    return 8 * eps * ((N + 8) * abs(float(a1)) + size), 8 * eps * (N + 8) * abs(float(s2))


def _counts(kind):
    rng = np.random.default_rng(11)
    return {
        "zeros": np.zeros(50, np.int64),                                       # an empty table
        "one-value": np.full(37, 5, np.int64),
        "distinct": rng.permutation(np.arange(400)),                           # every value once
        "across-cap": np.array([0, 1, 1023, 1024, 1025, 1026, 3000, 3000, 5000, 70000, 12, 12, 12]),
        "int32-max": np.array([3, 0, 2 ** 31 - 1, 17, 2 ** 31 - 1, 1024]),
        "overdispersed": rng.negative_binomial(0.7, 0.7 / (0.7 + 40.0), 3000),
    }[kind]


@pytest.mark.parametrize("phi", [1e-6, 1e-3, 0.3, 1.0, 17.5, 1e4, 1e9])
@pytest.mark.parametrize("kind", ["zeros", "one-value", "distinct", "across-cap", "int32-max", "overdispersed"])
def test_phi_terms_host(kind, phi):
    from stark_amd import engine
    y = _counts(kind)
    a1, s2 = engine.negbin_phi_terms(y, phi)
    r1, r2 = R.phi_terms(y, phi)
    t1, t2 = _tol(y, phi, r1, r2)
    print(f"{kind} phi={phi:g}: A1 {a1!r} err/tol {abs(a1 - float(r1)) / max(t1, 1e-300):.3f}; "
          f"S2 {s2!r} err/tol {abs(s2 - float(r2)) / max(t2, 1e-300):.3f}")
    if kind == "zeros":
        assert a1 == 0.0 and s2 == 0.0
        return
    assert abs(R.L(a1) - r1) <= t1, (a1, float(r1))
    assert abs(R.L(s2) - r2) <= t2, (s2, float(r2))


def test_phi_terms_host_refuses():
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    for y, phi in (([0, -1], 1.0), ([1, 2], 0.0), ([1, 2], -1.0), ([1, 2], np.inf), ([1, 2], np.nan)):
        with pytest.raises(StarkHipError) as e:
            engine.negbin_phi_terms(y, phi)
        assert e.value.code == -1


# ---------------------------------------------------------------- the restatement against an independent formula
def test_phi_to_infinity_is_poisson():
    """At phi = 1e12 the reference's likelihood (its lp less the Jacobian v) is Poisson's sum(y eta - e^eta) to 1e-6
    relative on counts <= 50 (the next term of the expansion is sum (y - mu)^2 / (2 phi) - ..., ~1e-9 here)."""
    rng = np.random.default_rng(3)
    X = rng.uniform(-1.7, 1.7, (500, 4))
    beta = np.array([0.4, -0.3, 0.2, 0.1])
    y = np.minimum(rng.poisson(np.exp(1.0 + X @ beta)), 50)
    q = np.concatenate([[1.0], beta, [np.log(1e12)]])[None, :]
    lp, _g = R.ref_lpgrad(X, y, q)
    pois = R.ref_poisson_lp(X, y, q[:, :-1])
    assert abs(float(lp[0] - q[0, -1] - pois[0])) <= 1e-6 * abs(float(pois[0]))
