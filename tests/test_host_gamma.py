"""The gamma family (gamma, log link) on the host (CPU only): the program recogniser (both rate spellings, both orders
of the sum, the three declarations of y, the shape priors, the near-miss programs), data packing and its y > 0 check,
the extract() rows, the driver's refusals, the shape-only terms kappa and kappa' of csrc/gamma_math.h through
stk_gamma_shape_terms_host against mpmath, and the longdouble reference tests/gamma_ref.py itself against mpmath and
against the exponential density it becomes at shape = 1.
"""
import json
import os

import numpy as np
import pytest

import gamma_ref as R
from stark_amd import frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_VEC = "data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; vector<lower=0>[N] y; }\n"
HEAD_OLD = "data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; real<lower=0> y[N]; }\n"
HEAD_ARR = "data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; array[N] real<lower=0> y; }\n"
PARAMS = "parameters { real alpha; vector[K] beta; real<lower=0> shape; }\n"
LIK = "y ~ gamma(shape, shape ./ exp(alpha + x * beta));"
LIKS = [LIK, "y~gamma(shape,shape./exp(x*beta+alpha));", "y ~ gamma( shape , shape  ./  exp( x * beta + alpha ) ) ;",
        "y ~ gamma(shape, shape * exp(-(alpha + x * beta)));", "y~gamma(shape,shape*exp(-(x*beta+alpha)));",
        "y ~ gamma(shape , shape * exp( - ( x * beta + alpha ) ) );"]
PINNED = "family='schools'|'linear'|'logistic'|'poisson'|'neg_binomial'|'student_t'"


def program(head=HEAD_VEC, params=PARAMS, lik=LIK, priors="", extra=""):
    return head + params + extra + "model {\n" + priors + "  " + lik + "  // severity\n}\n"


# ---------------------------------------------------------------- recognition
@pytest.mark.parametrize("head", [HEAD_VEC, HEAD_OLD, HEAD_ARR], ids=["vector", "y[N]", "array[N]"])
@pytest.mark.parametrize("lik", LIKS, ids=["div", "div-tight-x-first", "div-wide-x-first", "mul", "mul-tight-x-first", "mul-wide-x-first"])
@pytest.mark.parametrize("priors,want", [
    ("", {}),
    ("  alpha ~ normal(0, 2.5);\n  beta ~ normal(0, 0.5);\n  shape ~ gamma(2, 0.5);\n", {"alpha": 2.5, "beta": 0.5, "shape": (2.0, 0.5)}),
    ("  shape ~ exponential(0.25);\n", {"shape": (1.0, 0.25)}),
], ids=["flat", "all", "exponential"])
def test_recognised(head, lik, priors, want):
    code = program(head=head, lik=lik, priors=priors)
    assert frontend.program_info(code) == ("gamma", want)
    assert frontend.recognise(code) == "gamma"


def test_shipped_programs():
    d = os.path.join(os.path.dirname(frontend.__file__), "models")
    assert frontend.load_program_info(file=os.path.join(d, "gamma.stan")) == ("gamma", {})
    assert frontend.load_program_info(file=os.path.join(d, "gamma_prior.stan")) == \
        ("gamma", {"alpha": 10.0, "beta": 2.5, "shape": (2.0, 0.5)})
    assert frontend.load_program_info(family="gamma", priors={"shape": (3.0, 1.0)}) == ("gamma", {"shape": (3.0, 1.0)})
    with pytest.raises(ValueError):
        frontend.load_program_info(family="gama")
    # the families that were there are still told apart
    assert frontend.load_program_info(file=os.path.join(d, "linear.stan"))[0] == "linear"
    assert frontend.load_program_info(file=os.path.join(d, "neg_binomial.stan")) == ("neg_binomial", {})
    assert frontend.load_program_info(file=os.path.join(d, "poisson.stan"))[0] == "poisson"


NB_PROGRAM = ("data { int<lower=0> N; int<lower=0> K; matrix[N, K] x; int<lower=0> y[N]; }\n"
              "parameters { real alpha; vector[K] beta; real<lower=0> phi; }\n"
              "model { shape ~ gamma(2, 0.5); y ~ neg_binomial_2_log(alpha + x * beta, phi); }\n")


@pytest.mark.parametrize("code", [
    program(lik="y ~ gamma(shape, shape ./ exp(alpha + x * beta) + 1);"),
    program(lik="y ~ gamma(shape, exp(-(alpha + x * beta)));"),                                   # rate without the shape
    program(lik="y ~ gamma(shape, 2 * shape ./ exp(alpha + x * beta));"),
    program(lik="y ~ gamma(shape, rate);"),
    program(lik="y ~ gamma(shape, shape ./ exp(alpha + x * beta + 1));"),                         # an offset
    program(lik="y ~ gamma(shape, shape ./ exp(alpha + x * beta + off));"),
    program(lik="y ~ gamma(shape, shape ./ (alpha + x * beta));"),                                # identity link
    program(lik="y ~ gamma(shape, shape .* (alpha + x * beta));"),                                # inverse link
    program(lik="y ~ gamma(shape, shape * (alpha + x * beta));"),
    program(priors="  shape ~ normal(0, 5);\n"),                                                  # another shape prior
    program(priors="  shape ~ cauchy(0, 5);\n"),
    program(priors="  shape ~ gamma(0, 1);\n"),
    program(priors="  shape ~ gamma(2, 0.5);\n  shape ~ exponential(1);\n"),                      # two of them
    NB_PROGRAM,                                                                                   # a shape prior elsewhere
    program(params="parameters { real alpha; vector[K] beta; real shape; }\n"),                   # shape unbounded
    program(params="parameters { real alpha; vector[K] beta; }\n",
            head=HEAD_VEC.replace("y; }", "y; real<lower=0> shape; }")),                          # shape as data
    program(params="parameters { real alpha; vector[K] beta; real<lower=0> phi; }\n",
            extra="transformed parameters { real shape = 1 / phi; }\n"),                          # shape derived
    program(head=HEAD_VEC.replace("vector<lower=0>[N] y", "vector[N] y")),                        # y unbounded
    program(head=HEAD_VEC.replace("vector<lower=0>[N] y", "int<lower=0> y[N]")),
    program(lik="target += gamma_lpdf(y | shape, shape ./ exp(alpha + x * beta));"),
    program(lik="y ~ gamma(shape, shape ./ exp(alpha + x * beta)); y ~ normal(0, 1);"),
], ids=["rate-plus-1", "rate-no-shape", "rate-scaled", "rate-var", "offset", "offset-var", "identity-link", "inverse-link",
        "inverse-link-mul", "shape-normal", "shape-cauchy", "shape-gamma-0", "shape-two-priors", "shape-prior-negbin",
        "shape-unbounded", "shape-data", "shape-derived", "y-unbounded", "y-int", "target", "second-statement"])
def test_refused(code):
    with pytest.raises(NotImplementedError) as e:
        frontend.program_info(code)
    assert PINNED + "|'gamma'" in str(e.value)


# ---------------------------------------------------------------- data, rows
def _data(y, n=None, k=2):
    n = len(y) if n is None else n
    return {"N": n, "K": k, "x": np.arange(n * k, dtype=float).reshape(n, k), "y": y}


def test_pack_data():
    sh = frontend.pack_data("gamma", _data([0.5, 3.0, 2.0, 1e3]))
    assert sh["y"].dtype == np.float64 and sh["y"].tolist() == [0.5, 3.0, 2.0, 1e3] and set(sh) == {"x", "y"}
    assert sh["x"].dtype == np.float64 and sh["x"].shape == (4, 2)
    one = frontend.pack_data("gamma", _data([2.5], k=1))                # K = 1 and N = 1
    assert one["x"].shape == (1, 1) and one["y"].tolist() == [2.5]
    assert frontend.pack_data("gamma", _data([5e-324, 1.7e308]))["y"].tolist() == [5e-324, 1.7e308]
    for bad in (0.0, -1.0, float("nan"), float("inf"), -0.0):
        with pytest.raises(ValueError, match=r"y\[2\]"):
            frontend.pack_data("gamma", _data([0.5, 3.0, bad, 1.0]))
    with pytest.raises(ValueError, match="N entries"):
        frontend.pack_data("gamma", _data([1.0, 2.0], n=3))
    assert frontend.pack_data("linear", _data([0.5, -3.0]))["y"].tolist() == [0.5, -3.0]   # the linear family's y is any real


def test_rows():
    d = {"K": 3}
    assert frontend.column_names("gamma", d) == ["alpha", "beta[1]", "beta[2]", "beta[3]", "shape", "lp__"]
    assert frontend.param_rows("gamma", d) == {"alpha": [0], "beta": [1, 2, 3], "shape": [4], "lp__": [5]}
    assert frontend.select_pars("gamma", d, "shape") == [4, 5]
    assert frontend.select_pars("gamma", d, ["shape", "alpha"]) == [4, 0, 5]
    assert frontend.select_pars("gamma", d, ["beta"], include=False) == [0, 4, 5]
    with pytest.raises(ValueError):
        frontend.select_pars("gamma", d, "sigma")
    assert frontend.column_names("linear", d)[-2] == "sigma" and frontend.column_names("neg_binomial", d)[-2] == "phi"


def test_engine_tables_and_driver_refusals():
    from stark_amd import _lib, engine, stark
    assert engine.FAMILIES["gamma"] == 7 == _lib.STK_GAMMA and engine.FAMILY_NAMES[7] == "gamma"
    assert list(engine.FAMILIES.values()) == [1, 2, 3, 4, 5, 6, 7]
    q = stark._unconstrain("gamma", {"K": 2}, {"alpha": 0.5, "beta": [1.0, -1.0], "shape": 4.0})
    assert np.allclose(q, [0.5, 1.0, -1.0, np.log(4.0)])
    u = stark.unconstrain_draws("gamma", np.array([[0.1, 0.2], [1.0, 2.0], [2.0, 8.0], [-5.0, -6.0]]))
    assert np.allclose(u, [[0.1, 1.0, np.log(2.0)], [0.2, 2.0, np.log(8.0)]])
    with pytest.raises(ValueError, match="shape"):
        stark.unconstrain_draws("gamma", np.array([[0.1], [1.0], [0.0], [-5.0]]))
    for what in ("waic", "loo", "ppc", "bootstrap", "method='laplace'", "weights='laplace'"):
        with pytest.raises(ValueError, match="gamma"):
            stark._refuse_analysis("gamma", what)
    stark._refuse_analysis("linear", "waic")


# ---------------------------------------------------------------- the shape-only terms
def _mp(x):
    """A longdouble or a double as an mpf, exactly."""
    import mpmath as mp
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(np.longdouble(x) - np.longdouble(hi)))


def _kappa_mp(a):
    """kappa(a) and kappa'(a) good to 50 digits: the working precision covers what the subtraction cancels (at
    a = 1e300 kappa' = 5e-301 is left of two terms of 690)."""
    import mpmath as mp
    with mp.workdps(50 + 2 * int(abs(mp.log10(a))) + 20):
        A = mp.mpf(a)
        return +(A * mp.log(A) - A - mp.loggamma(A)), +(mp.log(A) - mp.digamma(A))


def test_shape_terms_against_mpmath():
    """|kappa - kappa_mp| <= 1e-13 max(|kappa|, 1) and |kappa' - kappa'_mp| <= 1e-13 kappa', kappa' > 0, on a log grid
    from 1e-300 to 1e300, at the named points, across the Stirling threshold (16) and on a fine grid over [1e-3, 1e4]:
    three decades inside the 1e-10 density bar, which n kappa and a n kappa' enter with relative weight 1.  Largest
    ratios measured: 0.0084 (kappa) and 0.0057 (kappa') of these bars (profiles/r29a_gamma_errors.json)."""
    mp = pytest.importorskip("mpmath")
    from stark_amd import engine
    grid = [10.0 ** e for e in range(-300, 301, 3)] + [0.5, 1.0, 2.0, 6.4, 19.99, 20.0, 20.01]
    grid += [15.0, 15.99, 16.0 - 2.0 ** -49, 16.0, 16.0 + 2.0 ** -48, 16.01, 17.0, 2.0 ** -1022, 1.7e308]
    grid += list(np.exp(np.linspace(np.log(1e-3), np.log(1e4), 300)))
    w0 = w1 = mp.mpf(0)
    for a in grid:
        k0, k1 = engine.gamma_shape_terms(float(a))
        m0, m1 = _kappa_mp(float(a))
        assert k1 > 0, a
        r0, r1 = abs(k0 - m0) / (mp.mpf("1e-13") * max(abs(m0), 1)), abs(k1 - m1) / (mp.mpf("1e-13") * m1)
        assert r0 <= 1 and r1 <= 1, (a, k0, k1, float(r0), float(r1))
        w0, w1 = max(w0, r0), max(w1, r1)
    print(f"gamma shape terms: kappa {float(w0):.2e} kappa' {float(w1):.2e} of the 1e-13 bars")
    out = os.environ.get("STARK_GAMMA_ERRORS_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"kappa": float(w0), "kappa_prime": float(w1), "points": len(grid)}, f)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert all(np.isnan(v) for v in engine.gamma_shape_terms(bad)), bad


# ---------------------------------------------------------------- the reference itself
def test_reference_against_mpmath():
    """tests/gamma_ref.py on 50 rows, d = 3, shapes 0.01 to 1e6, with both priors, against the density written out
    in mpmath at 50 digits with mpmath's own loggamma and digamma: 1e-17 relative on lp and on every gradient
    component (relative to the largest)."""
    mp = pytest.importorskip("mpmath")
    rng = np.random.default_rng(50)
    X = rng.uniform(-1.7, 1.7, (50, 3))
    b = np.array([0.4, -0.3, 0.2])
    y = np.exp(0.3 + X @ b) * rng.gamma(2.0, 0.5, 50)
    q = np.concatenate([0.3 + rng.normal(0, 0.2, (6, 1)), b + rng.normal(0, 0.2, (6, 3)),
                        np.log([0.01, 0.5, 2.0, 19.5, 1e3, 1e6])[:, None]], axis=1)
    lp, g = R.ref_lpgrad(X, y, q, shape_prior=(2.0, 0.5), prior=(2.0, 0.5))
    with mp.workdps(50):
        for c in range(6):
            al, be, u = mp.mpf(q[c, 0]), [mp.mpf(v) for v in q[c, 1:4]], mp.mpf(q[c, 4])
            a = mp.exp(u)
            t = [mp.log(mp.mpf(y[i])) - (al + sum(mp.mpf(X[i, j]) * be[j] for j in range(3))) for i in range(50)]
            H = sum(mp.expm1(v) - v for v in t)
            Lm = sum(mp.log(mp.mpf(v)) for v in y)
            mlp = (50 * (a * mp.log(a) - a - mp.loggamma(a)) - Lm - a * H + u - (al * al / 4 + sum(v * v for v in be) / mp.mpf("0.25")) / 2
                   + u - a / 2)
            de = [a * mp.expm1(v) for v in t]
            mg = [sum(de) - al / 4] + [sum(de[i] * mp.mpf(X[i, j]) for i in range(50)) - be[j] * 4 for j in range(3)]
            mg.append(a * (50 * (mp.log(a) - mp.digamma(a)) - H) + 1 + 1 - a / 2)
            assert abs(_mp(lp[c]) - mlp) <= mp.mpf("1e-17") * max(abs(mlp), 1), (c, lp[c], mlp)
            gmax = max(abs(v) for v in mg) + 1
            for j in range(5):
                assert abs(_mp(g[c, j]) - mg[j]) <= mp.mpf("1e-17") * gmax, (c, j, g[c, j], mg[j])


def test_reference_is_the_exponential_at_shape_one():
    """At u = 0 (shape 1) the density is the exponential's: lp = -sum (eta_i + y_i exp(-eta_i)), to 1e-15 relative;
    and the deviance form equals the textbook form n (a log a - lgamma a) + (a - 1) L - a sum (eta + y e^-eta) + u at a
    moderate shape, where the latter loses nothing."""
    rng = np.random.default_rng(7)
    L = np.longdouble
    X = rng.uniform(-1.7, 1.7, (200, 4))
    y = np.exp(0.2 + X @ [0.3, -0.2, 0.1, 0.5]) * rng.gamma(2.0, 0.5, 200)
    q = rng.normal(0, 0.3, (5, 6))
    q[:, -1] = 0.0
    lp = R.ref_lpgrad(X, y, q)[0]
    eta = q[:, 0].astype(L)[None, :] + X.astype(L) @ q[:, 1:5].astype(L).T
    want = -(eta + y.astype(L)[:, None] * np.exp(-eta)).sum(0)
    assert np.all(np.abs(lp - want) <= 1e-15 * np.abs(want)), (lp, want)
    q[:, -1] = np.log(3.0)
    a = L(3.0)
    ly = np.log(y.astype(L))
    text = 200 * (a * np.log(a) - R.lgamma(a)[0]) + (a - 1) * ly.sum() - a * (eta + y.astype(L)[:, None] * np.exp(-eta)).sum(0) + np.log(a)
    lp3 = R.ref_lpgrad(X, y, q)[0]
    assert np.all(np.abs(lp3 - text) <= 1e-15 * np.abs(text)), (lp3, text)
    # shape ~ gamma(s, r) adds (s - 1) u - r a and its derivative
    lpp, gp = R.ref_lpgrad(X, y, q, shape_prior=(2.0, 0.5))
    g3 = R.ref_lpgrad(X, y, q)[1]
    assert np.allclose((lpp - lp3).astype(float), np.log(3.0) - 1.5) and np.allclose((gp - g3)[:, -1].astype(float), 1.0 - 1.5)
    # e^u outside the doubles: no density
    q[:, -1] = [800.0, -800.0, 700.0, -700.0, 0.0]
    fin = np.isfinite(R.ref_lpgrad(X, y, q)[0].astype(np.float64))
    assert fin.tolist() == [False, False, True, True, True]
