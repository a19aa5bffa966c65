"""Stan-program front end for ``Stark.setStanModel`` (stark/stark.py:37-39).

The reference compiles any Stan program with pystan (``StanModel(**kwargs)``).  This build
has no Stan compiler: it recognises the program as one of the fixed model families whose
log density and gradient are hand-written gfx950 kernels, and raises
``NotImplementedError`` for anything else.  Recognition works on a normalised token
stream (comments and whitespace removed, old ``real y[J]`` and new ``array[J] real y``
declarations both accepted), so formatting does not matter; an explicit ``family=``
keyword overrides it.
"""
from __future__ import annotations

import re

import numpy as np


def _strip(code: str) -> str:
    code = re.sub(r"/\*.*?\*/", " ", code, flags=re.S)
    code = re.sub(r"//[^\n]*", " ", code)
    code = re.sub(r"#[^\n]*", " ", code)
    code = re.sub(r"\s+", " ", code)
    code = re.sub(r"\s*([{}()\[\];,<>=~*+\-:/])\s*", r"\1", code)
    return code.strip()


def _blocks(code: str) -> dict:
    out = {}
    i = 0
    while i < len(code):
        m = re.compile(r"(functions|transformed data|data|transformed parameters|parameters|model|generated quantities)\{").match(code, i)
        if not m:
            i += 1
            continue
        depth, j = 1, m.end()
        while j < len(code) and depth:
            depth += {"{": 1, "}": -1}.get(code[j], 0)
            j += 1
        out[m.group(1)] = code[m.end():j - 1]
        i = j
    return out


def _decl(block: str, pattern: str) -> bool:
    return re.search(pattern, block) is not None


def _stmts(block: str) -> list:
    return [s for s in block.split(";") if s]


_NUM = r"([0-9]+(?:\.[0-9]*)?(?:[eE][-+]?[0-9]+)?|\.[0-9]+(?:[eE][-+]?[0-9]+)?)"
_PRIOR = re.compile(r"(alpha|beta)~normal\(0(?:\.0*)?," + _NUM + r"\)$")


# phi ~ gamma(a, b) or phi ~ exponential(r) = gamma(1, r): the negative binomial's only phi priors
_PRIOR_PHI = re.compile(r"phi~(?:gamma\(" + _NUM + "," + _NUM + r"\)|exponential\(" + _NUM + r"\))$")


# y ~ student_t(nu, alpha + x * beta, sigma): nu a positive literal or the data variable `nu`
_STUDENT = re.compile(r"y~student_t\((?:" + _NUM + r"|(nu)),(?:alpha\+x\*beta|x\*beta\+alpha),sigma\)$")


# y ~ gamma(shape, shape ./ exp(alpha + x * beta)) or y ~ gamma(shape, shape * exp(-(alpha + x * beta))): the gamma
# GLM with the log link, rate = shape / mean (_strip leaves the blank before `./` where the program has one)
_ETA = r"(?:alpha\+x\*beta|x\*beta\+alpha)"
_GAMMA = re.compile(r"y~gamma\(shape,shape(?: ?\./exp\(" + _ETA + r"\)|\*exp\(-\(" + _ETA + r"\)\))\)$")
# shape ~ gamma(a, b) or shape ~ exponential(r) = gamma(1, r): the gamma family's only shape priors
_PRIOR_SHAPE = re.compile(r"shape~(?:gamma\(" + _NUM + "," + _NUM + r"\)|exponential\(" + _NUM + r"\))$")


# Softmax regression (models/categorical.stan): K = ncat classes, class ncat the reference, beta a column-major vector.
#   matrix[N, ncat - 1] eta = rep_matrix(alpha', N) + x * to_matrix(beta, K, ncat - 1);      (either order of the sum)
#   for (n in 1:N) y[n] ~ categorical_logit(append_row(eta[n]', 0));                          (with or without braces)
_CAT_XB = r"x\*to_matrix\(beta,K,ncat-1\)"
_CAT_A = r"rep_matrix\(alpha',N\)"
_CAT_ETA = re.compile(r"matrix\[N,ncat-1\]eta=(?:" + _CAT_A + r"\+" + _CAT_XB + "|" + _CAT_XB + r"\+" + _CAT_A + ")$")
_CAT_LIK = re.compile(r"for\(n in 1:N\)(\{?)y\[n\]~categorical_logit\(append_row\(eta\[n\]',0\)\)$")
_CAT_PARAMS = re.compile(r"vector\[ncat-1\]alpha;vector\[K\*\(ncat-1\)\]beta;?$")


def _recognise_categorical(b: dict, stm: list):
    """'categorical' for the committed program's blocks.  A `matrix` beta, a missing append_row(., 0), a
    categorical(softmax(.)), an added offset and a transformed parameters block are other programs to this recogniser."""
    lik = [_CAT_LIK.match(t) for t in stm]
    braced = [m for m in lik if m and m.group(1)]
    # one eta statement, one loop; a braced loop body leaves its closing brace behind as the last statement
    rest = [t for t, m in zip(stm, lik) if not m]
    if braced:
        if not rest or rest[-1] != "}":
            return None
        rest = rest[:-1]
    if sum(1 for m in lik if m) != 1 or len(rest) != 1 or not _CAT_ETA.match(rest[0]):
        return None
    data = b.get("data", "")
    if (_CAT_PARAMS.match(b.get("parameters", "")) and not b.get("transformed parameters")
            and _decl(data, r"(^|;)int<lower=[01]>N(;|$)") and _decl(data, r"(^|;)int<lower=[01]>K(;|$)")
            and _decl(data, r"(^|;)matrix\[N,K\]x(;|$)")
            and _decl(data, r"(^|;)int<lower=2>ncat(;|$)")
            and _decl(data, r"(^|;)(int<lower=1,upper=ncat>y\[N\]|array\[N\]int<lower=1,upper=ncat>y)(;|$)")):
        return "categorical"
    return None


def _split_priors(stmts):
    """Separate `alpha ~ normal(0, s)` / `beta ~ normal(0, s)` statements (s > 0) and `phi ~ gamma(a, b)` /
    `phi ~ exponential(r)` (a, b, r > 0; stored as 'phi': (a, b)) from the rest; `shape ~ ...` likewise, as
    'shape': (a, b)."""
    priors, rest = {}, []
    for st in stmts:
        m = _PRIOR.match(st)
        mp = _PRIOR_PHI.match(st)
        msh = _PRIOR_SHAPE.match(st)
        if m and float(m.group(2)) > 0 and m.group(1) not in priors:
            priors[m.group(1)] = float(m.group(2))
        elif mp and "phi" not in priors and all(float(g) > 0 for g in mp.groups() if g is not None):
            priors["phi"] = (float(mp.group(1)), float(mp.group(2))) if mp.group(1) is not None else (1.0, float(mp.group(3)))
        elif msh and "shape" not in priors and all(float(g) > 0 for g in msh.groups() if g is not None):
            priors["shape"] = (float(msh.group(1)), float(msh.group(2))) if msh.group(1) is not None else (1.0, float(msh.group(3)))
        else:
            rest.append(st)
    return priors, rest


def program_info(model_code: str):
    """(family, priors) of a supported Stan program; priors = {'alpha': s, 'beta': s} for the
    regressions' optional `alpha ~ normal(0, s)` / `beta ~ normal(0, s)` statements (absent: flat), and
    'phi': (a, b) for the negative binomial's `phi ~ gamma(a, b)` / `phi ~ exponential(b)`, 'shape': (a, b) for the
    gamma family's `shape ~ gamma(a, b)` / `shape ~ exponential(b)`, and 'nu': v for a
    student_t statement whose nu is the literal v (absent when nu is the data variable: pack_data reads it)."""
    code = _strip(model_code)
    b = _blocks(code)
    priors, rest = _split_priors(_stmts(b.get("model", "")))
    fam = _recognise_blocks(b, sorted(rest)) or _recognise_categorical(b, rest)
    if fam == "student_t":
        lit = _STUDENT.match(rest[0]).group(1)
        if lit is not None:
            priors["nu"] = float(lit)
    if fam == "schools" and priors:
        fam = None
    if fam != "neg_binomial" and "phi" in priors:   # a phi prior belongs to the negative binomial alone
        fam = None
    if fam != "gamma" and "shape" in priors:        # a shape prior belongs to the gamma family alone
        fam = None
    if fam is None:
        raise NotImplementedError(
            "stark_amd runs a fixed set of model families on the GPU (8 schools, Bayesian linear, logistic, "
            "Poisson (poisson_log), negative-binomial (neg_binomial_2_log) and Student-t (student_t with nu a data "
            "variable or a literal, never a parameter) regression with flat or normal(0, s) "
            "priors on alpha and beta, and for the negative binomial a flat, gamma(a, b) or exponential(r) prior on "
            "phi, and gamma regression with the log link (gamma(shape, shape ./ exp(alpha + x * beta))) with a flat, "
            "gamma(a, b) or exponential(r) prior on shape, and softmax regression (categorical_logit with the last class "
            "as reference and beta a column-major vector); see stark_amd/models/*.stan).  This Stan program is not one "
            "of them; pass "
            "family='schools'|'linear'|'logistic'|'poisson'|'neg_binomial'|'student_t'|'gamma'|'categorical' if it is an equivalent program.")
    return fam, priors


def recognise(model_code: str) -> str:
    """Return 'schools', 'linear', 'logistic', 'poisson', 'neg_binomial', 'student_t', 'gamma' or 'categorical' for a supported Stan program."""
    return program_info(model_code)[0]


def _recognise_blocks(b: dict, stm: list):
    params = b.get("parameters", "")
    tp = b.get("transformed parameters", "")
    # 8 schools, non-centred (example/schools.stan:1-18)
    if (_decl(params, r"(^|;)real mu(;|$)") and _decl(params, r"real<lower=0>tau") and
            _decl(params, r"(real eta\[J\]|vector\[J\]eta|array\[J\]real eta)")):
        theta_ok = (re.search(r"theta\[j\]=mu\+tau\*eta\[j\]", tp) or re.search(r"theta=mu\+tau\*eta", tp))
        want = sorted(["eta~normal(0,1)", "y~normal(theta,sigma)"])
        want2 = sorted(["eta~std_normal()", "y~normal(theta,sigma)"])
        if theta_ok and stm in (want, want2):
            return "schools"
    if _decl(params, r"(^|;)real alpha(;|$)") and _decl(params, r"vector\[K\]beta"):
        if stm in (["y~bernoulli_logit(alpha+x*beta)"], ["y~bernoulli_logit(x*beta+alpha)"]):
            if not _decl(params, r"sigma"):
                return "logistic"
        if stm in (["y~poisson_log(alpha+x*beta)"], ["y~poisson_log(x*beta+alpha)"]):
            # counts: int<lower=0> y[N] or array[N] int<lower=0> y (poisson(exp(...)) and poisson_log_glm
            # are other programs to this recogniser)
            if not _decl(params, r"sigma") and _decl(b.get("data", ""), r"(int<lower=0>y\[N\]|array\[N\]int<lower=0>y)(;|$)"):
                return "poisson"
        if stm in (["y~neg_binomial_2_log(alpha+x*beta,phi)"], ["y~neg_binomial_2_log(x*beta+alpha,phi)"]):
            # phi is the dispersion itself, real<lower=0> phi (neg_binomial_2(exp(...), phi), neg_binomial_2_log_glm
            # and a reciprocal dispersion are other programs to this recogniser); counts as for poisson_log
            if (not _decl(params, r"sigma") and _decl(params, r"(^|;)real<lower=0>phi(;|$)") and not b.get("transformed parameters")
                    and _decl(b.get("data", ""), r"(int<lower=0>y\[N\]|array\[N\]int<lower=0>y)(;|$)")):
                return "neg_binomial"
        ms = _STUDENT.match(stm[0]) if len(stm) == 1 else None
        if ms:
            # sigma is the scale parameter itself and nu a constant: the data variable real<lower=0> nu, or a positive
            # literal.  nu in `parameters`, a sigma that is not the parameter, an added offset or a `nu ~ ...` statement
            # (it stays in stm) are other programs to this recogniser
            nu_ok = (_decl(b.get("data", ""), r"(^|;)real<lower=0>nu(;|$)") if ms.group(2) else float(ms.group(1)) > 0)
            if (_decl(params, r"(^|;)real<lower=0>sigma(;|$)") and not _decl(params, r"(^|;)[^;]*[ >\]]nu(;|$)")
                    and not b.get("transformed parameters") and nu_ok):
                return "student_t"
        if len(stm) == 1 and _GAMMA.match(stm[0]):
            # the rate is shape / exp(eta) itself (any other rate expression, an added offset, an identity or inverse
            # link are other programs to this recogniser), shape the parameter real<lower=0> shape, y positive reals
            if (_decl(params, r"(^|;)real<lower=0>shape(;|$)") and not _decl(params, r"sigma|phi") and not b.get("transformed parameters")
                    and _decl(b.get("data", ""), r"(^|;)(vector<lower=0>\[N\]y|real<lower=0>y\[N\]|array\[N\]real<lower=0>y)(;|$)")):
                return "gamma"
        if stm in (["y~normal(alpha+x*beta,sigma)"], ["y~normal(x*beta+alpha,sigma)"]):
            if _decl(params, r"real<lower=0>sigma"):
                return "linear"
    return None


def load_program_info(file=None, model_code=None, family=None, priors=None, **_ignored):
    """Mirror of pystan.StanModel(file=..., model_code=...) argument handling -> (family, priors).
    family= (and priors={'alpha': s, 'beta': s}, for 'neg_binomial' also 'phi': (shape, rate), for 'gamma' also
    'shape': (shape, rate)) override recognition."""
    if family is not None:
        if family not in ("schools", "linear", "logistic", "poisson", "neg_binomial", "student_t", "gamma", "categorical"):
            raise ValueError(f"unknown family {family!r}")
        return family, dict(priors or {})
    if model_code is None:
        if file is None:
            raise ValueError("Either file or model_code must be given (pystan.StanModel)")
        with open(file) as f:
            model_code = f.read()
    return program_info(model_code)


def load_program(file=None, model_code=None, family=None, **kw):
    """The family of the program (stark/stark.py:37-39 setStanModel)."""
    return load_program_info(file=file, model_code=model_code, family=family, **kw)[0]


def pack_data(family: str, data: dict, nu=None) -> dict:
    """Validate a Stan data dict (the prepare_data_callback output, example/stark_ex.py:8-11)
    and turn it into a shard for stk_model_create.  student_t: the shard carries "nu" too -- the statement's
    literal when the program has one (nu=), else data["nu"] (real<lower=0> nu), which must be there, finite and > 0."""
    if family == "schools":
        J = int(data["J"])
        y = np.asarray(data["y"], np.float64).reshape(-1)
        s = np.asarray(data["sigma"], np.float64).reshape(-1)
        if y.shape[0] != J or s.shape[0] != J:
            raise ValueError(f"schools data: J = {J} but len(y) = {y.shape[0]}, len(sigma) = {s.shape[0]}")
        if np.any(s <= 0):
            raise ValueError("schools data: sigma must be positive (real<lower=0> sigma[J])")
        return {"y": y, "sigma": s}
    N, K = int(data["N"]), int(data["K"])
    if hasattr(data["x"], "tocsr") and not isinstance(data["x"], np.ndarray):
        # a scipy.sparse design matrix goes through as it is (engine.Model keeps it as padded rows); N and K are
        # checked against its shape, y below as for dense rows
        x = data["x"]
        if tuple(x.shape) != (N, K):
            raise ValueError(f"sparse x has shape {tuple(x.shape)}, the data say N = {N}, K = {K}")
    else:
        x = np.asarray(data["x"], np.float64).reshape(N, K)
    if family == "logistic":
        y = np.asarray(data["y"]).reshape(-1)
        if y.shape[0] != N:
            raise ValueError("y must have N entries")
        # int<lower=0, upper=1> y[N]: pystan rejects non-integer or out-of-range values
        yf = y.astype(np.float64)
        if not np.all(yf == np.round(yf)) or np.any((yf != 0) & (yf != 1)):
            raise ValueError("bernoulli_logit data: y must hold the integers 0 and 1")
        return {"x": x, "y": yf.astype(np.int32)}
    if family == "categorical":
        # int<lower=2> ncat; int<lower=1, upper=ncat> y[N]: pystan rejects anything else
        if "ncat" not in data:
            raise ValueError("categorical data: ncat is missing (int<lower=2> ncat in the data block)")
        kf = float(np.asarray(data["ncat"], np.float64).reshape(()))
        if kf != np.round(kf) or kf < 2:
            raise ValueError(f"categorical data: ncat must be an integer >= 2, got {data['ncat']!r}")
        ncat = int(kf)
        y = np.asarray(data["y"]).reshape(-1)
        if y.shape[0] != N:
            raise ValueError("y must have N entries")
        if y.dtype.kind not in "iuf":
            raise ValueError("categorical_logit data: y must hold the integers 1 .. ncat")
        yf = y.astype(np.float64)
        if not np.all(yf == np.round(yf)) or np.any(yf < 1) or np.any(yf > ncat):
            bad = int(np.flatnonzero(~((yf == np.round(yf)) & (yf >= 1) & (yf <= ncat)))[0])
            raise ValueError(f"categorical_logit data: y must hold the integers 1 .. ncat = {ncat}, got y[{bad}] = {y[bad]!r}")
        return {"x": x, "y": yf.astype(np.int32), "ncat": ncat}
    if family in ("poisson", "neg_binomial"):
        y = np.asarray(data["y"]).reshape(-1)
        if y.shape[0] != N:
            raise ValueError("y must have N entries")
        # int<lower=0> y[N]: pystan rejects non-integer or negative values; the shard stores int32
        yf = y.astype(np.float64)
        if not np.all(yf == np.round(yf)) or np.any(yf < 0) or np.any(yf > 2147483647):
            raise ValueError(("poisson_log" if family == "poisson" else "neg_binomial_2_log") +
                             " data: y must hold integers >= 0 (and <= 2^31 - 1)")
        return {"x": x, "y": yf.astype(np.int32)}
    y = np.asarray(data["y"], np.float64).reshape(-1)
    if y.shape[0] != N:
        raise ValueError("y must have N entries")
    if family == "student_t":
        if nu is None:
            if "nu" not in data:
                raise ValueError("student_t data: nu is missing (real<lower=0> nu in the data block)")
            nu = data["nu"]
        nu = float(np.asarray(nu, np.float64).reshape(()))
        if not (np.isfinite(nu) and nu > 0):
            raise ValueError(f"student_t data: nu must be finite and > 0 (real<lower=0> nu), got {nu!r}")
        return {"x": x, "y": y, "nu": nu}
    if family == "gamma":
        # vector<lower=0>[N] y: the density needs log y, so 0 is refused too, and so is anything not finite
        if not np.all(np.isfinite(y) & (y > 0)):
            bad = int(np.flatnonzero(~(np.isfinite(y) & (y > 0)))[0])
            raise ValueError(f"gamma data: y must be finite and > 0, got y[{bad}] = {y[bad]!r}")
    return {"x": x, "y": y}


def column_names(family: str, data: dict) -> list:
    """extract() key order flattened to rows of the P x S draw matrix (stark/stark.py:49-56)."""
    if family == "schools":
        J = int(data["J"])
        return (["mu", "tau"] + [f"eta[{j}]" for j in range(1, J + 1)] + [f"theta[{j}]" for j in range(1, J + 1)]
                + ["lp__"])
    K = int(data["K"])
    if family == "categorical":   # alpha[1 .. G], beta[1 .. G K] (class g's coefficients are beta[(g - 1) K + 1 .. g K]), lp__
        G = int(data["ncat"]) - 1
        return [f"alpha[{g}]" for g in range(1, G + 1)] + [f"beta[{k}]" for k in range(1, G * K + 1)] + ["lp__"]
    cols = ["alpha"] + [f"beta[{k}]" for k in range(1, K + 1)]
    if family in ("linear", "student_t"):
        cols.append("sigma")
    if family == "neg_binomial":
        cols.append("phi")
    if family == "gamma":
        cols.append("shape")
    return cols + ["lp__"]


def param_rows(family: str, data: dict) -> "dict[str, list[int]]":
    """extract() keys in model order (parameters, transformed parameters, lp__) -> their rows
    in the P x S draw matrix (stark/stark.py:49-56 flattens each key to consecutive rows)."""
    groups, row = {}, 0
    for name in column_names(family, data):
        key = name.split("[")[0]
        groups.setdefault(key, []).append(row)
        row += 1
    return groups


def select_pars(family: str, data: dict, pars=None, include: bool = True) -> "list[int] | None":
    """pystan 2 ``sampling(pars=..., include=...)`` (forwarded by stark/stark.py:48 **kwargs):
    the rows that ``fit.extract()`` then returns, in its key order.  pars names the parameters
    to keep (include=True, in the given order) or to drop (include=False, model order kept);
    lp__ is always returned, last, once (an explicit 'lp__' in pars is that same row).  Unknown
    names raise ValueError as pystan does.  None: all rows (no selection).
    Parity UNPINNED against pystan itself: pystan is not importable here, and the golden fixture
    (tests/golden/make_golden.py, FakeStanModel) encodes this same reading of pystan 2's
    extract() order, so the driver test pins the reshape, not the selection order."""
    if pars is None:
        return None
    if isinstance(pars, str):
        pars = [pars]
    pars = list(pars)
    groups = param_rows(family, data)
    for p in pars:
        if p not in groups:
            raise ValueError(f"No parameter {p}")
    if include:
        keep = list(dict.fromkeys(p for p in pars if p != "lp__"))
    else:
        keep = [k for k in groups if k not in pars and k != "lp__"]
    keep.append("lp__")
    return [r for k in keep for r in groups[k]]

