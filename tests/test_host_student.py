"""The Student-t (student_t) family on the host (CPU only): the program recogniser (nu as data or as a literal,
never a parameter), data packing and its nu checks, the extract() rows, the init mapping, the driver's refusals, the
fingerprint's host twin with family word 6, the reference's nu -> inf limit against the linear density, and the
host build of the device log1p (csrc/student_math.h) against long double.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import student_ref as R
from stark_amd import frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_NEW = "data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; vector[N] y; real<lower=0> nu; }\n"
HEAD_OLD = "data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; real y[N]; real<lower=0> nu; }\n"
HEAD_ARR = "data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; array[N] real y; real<lower=0> nu; }\n"
HEAD_LIT = "data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; vector[N] y; }\n"
PARAMS = "parameters { real alpha; vector[K] beta; real<lower=0> sigma; }\n"
LIK = "y ~ student_t(nu, alpha + x * beta, sigma);"
PINNED = "family='schools'|'linear'|'logistic'|'poisson'|'neg_binomial'|'student_t'"


def program(head=HEAD_NEW, params=PARAMS, lik=LIK, priors="", extra=""):
    return head + params + extra + "model {\n" + priors + "  " + lik + "  // robust\n}\n"


# ---------------------------------------------------------------- recognition
@pytest.mark.parametrize("head", [HEAD_NEW, HEAD_OLD, HEAD_ARR], ids=["vector", "y[N]", "array[N]"])
@pytest.mark.parametrize("lik", [LIK, "y~student_t( nu , x*beta + alpha , sigma ) ;"], ids=["alpha-first", "x-first"])
@pytest.mark.parametrize("priors,want", [
    ("", {}),
    ("  alpha ~ normal(0, 2.5);\n  beta ~ normal(0, 0.5);\n", {"alpha": 2.5, "beta": 0.5}),
    ("  beta ~ normal(0.0, 1e0);\n", {"beta": 1.0}),
], ids=["flat", "both", "beta"])
def test_recognised_data_nu(head, lik, priors, want):
    fam, pri = frontend.program_info(program(head=head, lik=lik, priors=priors))
    assert fam == "student_t" and pri == want
    assert frontend.recognise(program(head=head, lik=lik, priors=priors)) == "student_t"


@pytest.mark.parametrize("lit,val", [("4", 4.0), ("2.5", 2.5), ("1e6", 1e6), (".5", 0.5), ("3.", 3.0)])
@pytest.mark.parametrize("order", ["alpha + x * beta", "x * beta + alpha"])
def test_recognised_literal_nu(lit, val, order):
    code = program(head=HEAD_LIT, lik=f"y ~ student_t({lit}, {order}, sigma);", priors="  alpha ~ normal(0, 10);\n")
    assert frontend.program_info(code) == ("student_t", {"alpha": 10.0, "nu": val})


def test_shipped_programs():
    d = os.path.join(os.path.dirname(frontend.__file__), "models")
    assert frontend.load_program_info(file=os.path.join(d, "student_t.stan")) == ("student_t", {})
    assert frontend.load_program_info(file=os.path.join(d, "student_t_prior.stan")) == \
        ("student_t", {"alpha": 10.0, "beta": 2.5, "nu": 4.0})
    assert frontend.load_program_info(family="student_t", priors={"nu": 3.0}) == ("student_t", {"nu": 3.0})
    # the families that were there are still told apart
    assert frontend.load_program_info(file=os.path.join(d, "linear.stan"))[0] == "linear"
    assert frontend.load_program_info(file=os.path.join(d, "neg_binomial.stan")) == ("neg_binomial", {})


@pytest.mark.parametrize("code", [
    program(params="parameters { real alpha; vector[K] beta; real<lower=0> sigma; real<lower=0> nu; }\n", head=HEAD_LIT),
    program(params="parameters { real alpha; vector[K] beta; real<lower=0> sigma; real<lower=1> nu; }\n", head=HEAD_LIT),
    program(params="parameters { real alpha; vector[K] beta; real<lower=0> sigma; real nu; }\n", head=HEAD_LIT),
    program(params="parameters { real alpha; vector[K] beta; }\n",
            head=HEAD_NEW.replace("real<lower=0> nu;", "real<lower=0> nu; real<lower=0> sigma;")),           # sigma is data
    program(params="parameters { real alpha; vector[K] beta; real<lower=0> tau; }\n", lik="y ~ student_t(nu, alpha + x * beta, tau);"),
    program(params="parameters { real alpha; vector[K] beta; real<lower=0> tau; }\n",
            extra="transformed parameters { real sigma = 1 / sqrt(tau); }\n"),                                # sigma derived
    program(params="parameters { real alpha; vector[K] beta; real sigma; }\n"),                                 # sigma unbounded
    program(lik="y ~ student_t(nu, alpha + x * beta, 2 * sigma);"),
    program(lik="y ~ student_t(nu, alpha + x * beta + 1, sigma);"),                                             # an offset
    program(lik="y ~ student_t(nu, alpha + x * beta + off, sigma);"),
    program(priors="  nu ~ gamma(2, 0.1);\n"),                                                                  # a nu prior
    program(head=HEAD_LIT),                                                                                     # nu undeclared
    program(head=HEAD_NEW.replace("real<lower=0> nu", "real nu")),                                              # nu unbounded
    program(head=HEAD_LIT, lik="y ~ student_t(0, alpha + x * beta, sigma);"),                                   # nu = 0
    program(head=HEAD_LIT, lik="y ~ student_t(-4, alpha + x * beta, sigma);"),
    program(lik="y ~ student_t(nu + 1, alpha + x * beta, sigma);"),
    program(lik="target += student_t_lpdf(y | nu, alpha + x * beta, sigma);"),
    program(priors="  sigma ~ cauchy(0, 5);\n"),
], ids=["nu-param", "nu-param-lower1", "nu-param-free", "sigma-data", "sigma-other-name", "sigma-derived", "sigma-unbounded",
        "sigma-scaled", "offset", "offset-var", "nu-prior", "nu-undeclared", "nu-unbounded", "nu-zero", "nu-negative", "nu-expr",
        "target", "sigma-prior"])
def test_refused(code):
    with pytest.raises(NotImplementedError) as e:
        frontend.program_info(code)
    assert PINNED in str(e.value) and "student_t" in str(e.value)


def test_family_keyword():
    assert frontend.load_program_info(family="student_t") == ("student_t", {})
    with pytest.raises(ValueError):
        frontend.load_program_info(family="student")


# ---------------------------------------------------------------- data, rows, init
def _data(nu=..., n=4, k=2):
    d = {"N": n, "K": k, "x": np.arange(n * k, dtype=float).reshape(n, k), "y": [0.5, -3.0, 2.0, 1e3]}
    if nu is not ...:
        d["nu"] = nu
    return d


def test_pack_data():
    sh = frontend.pack_data("student_t", _data(4))
    assert sh["y"].dtype == np.float64 and sh["y"].tolist() == [0.5, -3.0, 2.0, 1e3] and sh["nu"] == 4.0
    assert sh["x"].dtype == np.float64 and sh["x"].shape == (4, 2) and isinstance(sh["nu"], float)
    assert frontend.pack_data("student_t", _data(np.array([2.5])))["nu"] == 2.5
    assert frontend.pack_data("student_t", _data(), nu=3.0)["nu"] == 3.0            # the statement's literal
    assert frontend.pack_data("student_t", _data(7.0), nu=3.0)["nu"] == 3.0
    assert "nu" not in frontend.pack_data("linear", _data(4))                        # the other families are as they were


@pytest.mark.parametrize("bad", [..., 0, -1.0, float("inf"), float("nan")], ids=["missing", "zero", "negative", "inf", "nan"])
def test_pack_data_refuses(bad):
    with pytest.raises(ValueError) as e:
        frontend.pack_data("student_t", _data(bad))
    assert "nu" in str(e.value)
    if bad is not ...:
        with pytest.raises(ValueError):
            frontend.pack_data("student_t", _data(), nu=bad)
    d = _data(4)
    d["y"] = d["y"][:3]
    with pytest.raises(ValueError):
        frontend.pack_data("student_t", d)


def test_rows_as_linear():
    d = {"N": 5, "K": 3}
    assert frontend.column_names("student_t", d) == frontend.column_names("linear", d) == \
        ["alpha", "beta[1]", "beta[2]", "beta[3]", "sigma", "lp__"]
    assert frontend.param_rows("student_t", d) == frontend.param_rows("linear", d)
    for kw in (dict(pars=["sigma"]), dict(pars=["beta"], include=False), dict(pars=["beta", "alpha"]), dict(pars="lp__"), {}):
        assert frontend.select_pars("student_t", d, **kw) == frontend.select_pars("linear", d, **kw), kw
    assert frontend.select_pars("student_t", d, pars=["sigma"]) == [4, 5]
    for name in ("nu", "phi"):
        with pytest.raises(ValueError):
            frontend.select_pars("student_t", d, pars=[name])


def test_unconstrain():
    from stark_amd.stark import _unconstrain, sampling_config, unconstrain_draws
    d = {"N": 5, "K": 3}
    init = {"alpha": 0.25, "beta": [1.0, -2.0, 3.0], "sigma": 4.0}
    assert np.array_equal(_unconstrain("student_t", d, init), _unconstrain("linear", d, init))
    assert np.array_equal(_unconstrain("student_t", d, init), np.array([0.25, 1.0, -2.0, 3.0, np.log(4.0)]))
    assert _unconstrain("student_t", d, {}).tolist() == [0.0] * 5          # sigma = 1
    cfg = sampling_config("student_t", [d, d], iter=20, chains=3, init=0, seed=1)
    assert cfg["init"].shape == (2 * 3 * 5,) and not cfg["init"].any()
    m = np.array([[0.1, 0.2], [1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [2.0, 0.5], [-7.0, -8.0]])   # alpha, beta x3, sigma, lp__
    q = unconstrain_draws("student_t", m)
    assert np.array_equal(q, unconstrain_draws("linear", m))
    m[4, 1] = 0.0
    with pytest.raises(ValueError) as e:
        unconstrain_draws("student_t", m)
    assert "sigma" in str(e.value)


def test_driver_refusals_name_the_family():
    """waic, loo, ppc, bootstrap, weights='laplace', method='laplace' (both combiners) and full-data mode refuse the
    family by name before any sampling; partitions whose nu differ are refused before a model is built: no device is
    touched here."""
    from stark_amd import engine, fulldata, stark
    from stark_amd.rdd import LocalContext
    sc = LocalContext()
    rows = [(0.1 * i, 0.3 * i - 1.0) for i in range(8)]

    def prep(part):   # never reached
        raise AssertionError("sampled before refusing")

    st = stark.Stark(sc, sc.parallelize(rows, 2), prep)
    st.setStanModel(model_code=program())
    assert st.family == "student_t" and st.priors == {}
    draws = np.ones((4, 10))
    for call in (lambda: st.waic(draws), lambda: st.loo(draws), lambda: st.ppc(draws), lambda: st.bootstrap(n=4),
                 lambda: st.concensusWeight(weights="laplace"), lambda: st.concensusWeight(method="laplace"),
                 lambda: st.concensusWeight(method="laplace", combiner="semiparametric")):
        with pytest.raises(ValueError) as e:
            call()
        assert "student_t" in str(e.value)

    class FakeModel:
        family = engine.FAMILIES["student_t"]
        nshards = 1

    with pytest.raises(ValueError) as e:
        fulldata.FullDataSampler(FakeModel())
    assert "student_t" in str(e.value)

    def prep_nu(part):
        a = np.array(part, np.float64)
        return {"N": len(part), "K": 1, "x": a[:, :1], "y": a[:, 1], "nu": 4.0 if part[0] == rows[0] else 5.0}

    two = stark.Stark(sc, sc.parallelize(rows, 2), prep_nu)
    two.setStanModel(model_code=program())
    with pytest.raises(ValueError, match="nu differ"):
        two._draw_partitions([prep_nu(p) for p in (rows[:4], rows[4:])], chains=1, iter=10)
    with pytest.raises(ValueError, match="nu="):
        engine.Model(None, "student_t", [])
    with pytest.raises(ValueError, match="poisson"):
        engine.Model(None, "poisson", [], nu=4.0)


# ---------------------------------------------------------------- fingerprint (the header's formula)
@pytest.mark.parametrize("n,d", [(1, 1), (7, 3), (300, 20)])
def test_shard_fingerprint_family_word_6(n, d):
    """The family word is part of the fingerprint: the same rows as "linear" (word 2) fingerprint differently, and
    both are the header's formula with their word."""
    from stark_amd import engine
    from test_host_poisson import MASK, fmix, words

    def twin(fam):   # fmix(words([family, n, d], 0) + words(x, 1) + words(y doubles, 2))
        acc = words(np.array([fam, n, d], np.uint64), 0) + words(x, 1) + words(y, 2)
        with np.errstate(over="ignore"):
            return int(fmix(np.array([acc & MASK], np.uint64))[0])

    assert engine.FAMILIES["student_t"] == 6
    rng = np.random.default_rng(n)
    x = rng.normal(size=(n, d))
    y = rng.standard_t(2, n)
    fp = int(engine.shard_fingerprint("student_t", {"x": x, "y": y}))
    lin = int(engine.shard_fingerprint("linear", {"x": x, "y": y}))
    assert fp == int(engine.shard_fingerprint(6, {"x": x, "y": y})) and fp != lin
    assert lin == twin(2) and fp == twin(6)


# ---------------------------------------------------------------- the reference
def test_reference_gradient_is_the_density_s():
    """student_ref's gradient against central differences of its own lp (longdouble), and nu -> inf against the
    linear density."""
    rng = np.random.default_rng(3)
    X = rng.normal(size=(30, 3))
    y = X @ np.array([0.5, -1.0, 0.2]) + rng.standard_t(3, 30)
    y[0] += 50.0
    q = rng.normal(0, 0.5, (4, 5))
    for nu in (1.0, 4.0, 30.0):
        lp, g = R.ref_lpgrad(X, y, q, nu, prior=(2.0, 0.5))
        for j in range(5):
            h = np.zeros((4, 5), R.L)
            h[:, j] = R.L(1e-9)
            num = (R.ref_lpgrad(X, y, q.astype(R.L) + h, nu, prior=(2.0, 0.5))[0]
                   - R.ref_lpgrad(X, y, q.astype(R.L) - h, nu, prior=(2.0, 0.5))[0]) / (2 * h[:, j])
            assert np.all(np.abs(num - g[:, j]) <= 1e-7 * (1 + np.abs(g[:, j]))), (nu, j)
    big = R.ref_lpgrad(X, y, q, 1e12)[0]
    lin = R.ref_linear_lp(X, y, q)
    assert np.all(np.abs(big - lin) <= 1e-6 * np.abs(lin))


# ---------------------------------------------------------------- the device log1p on a host build
def test_student_math_check_builds_and_passes(tmp_path):
    """tools/student_math_check.cpp compiles csrc/student_math.h as host code and sweeps st_log1p over 0, the
    subnormals, 1e-323 .. 1e308 in decade steps, 40 neighbours either side of every branch point (sqrt(2) - 1, 1,
    2^k - 1 and sqrt(2) 2^k - 1 for every k, 2^52, 2^53) and 4e6 log-uniform arguments, against long double log1p.
    Largest relative error found when the function was written: 2.9 x 2^-53 (3.2e-16, at w = 1e-3); the bar is
    twice that, 5.8 x 2^-53 (6.4e-16).  0 -> 0, +inf -> +inf, NaN -> NaN and log1p(w) = w for tiny w are exact."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "student_math_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "student_math_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "st_log1p: largest relative error" in r.stdout and "special cases wrong: 0" in r.stdout
