"""Drop-in for ``stark/stark.py`` (randommm/stark): same names, arguments, return layout.

    from stark_amd import *                 # binds the submodule `stark` (stark/__init__.py:1)
    st = stark.Stark(sc, rdd, prepare_data_callback)
    st.setStanModel(file="schools.stan")
    weighted = st.concensusWeight(iter=5000)   # P x S consensus draws
    naive = st.distribute(n=4)                 # stacked P x S blocks, one per run

What changed underneath:
  * ``setStanModel`` recognises the program as one of the GPU model families
    (``stark_amd.frontend``) instead of compiling it with pystan;
  * every partition is a shard resident on a GPU; all local shards sample in ONE batched
    NUTS run (``libstark_hip.so``), one process per GPU, partition p on rank p % world;
  * the only exchange is one all-gather of the P x S draw matrices (RCCL), then the
    consensus combine runs as gfx950 kernels in partition order.

Deliberate deviations from the reference code, each mirroring its evident intent
(DESIGN.md "Reference bugs"): the combine accepts any number of partitions (the reference
reducer only works for two); shards with NaN draws are left out of the combine; naive
mode runs ``n`` full-data replicas (the reference's non-accumulating ``union`` runs the
partitions plus one full copy -- available as ``distribute(..., reference_union=True)``).
Draws follow pystan's ``fit.extract()`` (``permuted=True``, stark/stark.py:49): each chain's
post-warmup draws in a seeded random order, chains concatenated; ``permuted=False`` keeps
chain order (what the sampler's diagnostics need).
"""
from __future__ import annotations

import inspect
import warnings

import numpy as np

from . import dist, engine, frontend
from . import rdd as _rdd


def consensus_avg(J):
    """Pairwise reducer of stark/stark.py:7-21 on the GPU.

    ``c(f1, f2)`` returns ``[W1 + W2, W1 f1 + W2 f2]`` with ``W = inv(np.cov(f))``; if f1
    holds a NaN it returns f2 unchanged (:9-10).  Unlike the reference, f1 may also be the
    ``[sum W, sum W theta]`` pair of an earlier step, so ``functools.reduce`` works for any
    number of partitions.  ``J`` is ignored, as in the reference (:7)."""

    def c(f1, f2):
        if isinstance(f1, list):
            sw, swt = f1
            f2 = np.asarray(f2, np.float64)
            if np.isnan(f2).any():          # a NaN shard later in the reduce is left out
                return [sw, swt]
            w2, w2t, _ = engine.consensus_products([f2])
            return [sw + w2, swt + w2t]
        f1 = np.asarray(f1, np.float64)
        if np.isnan(f1).any():
            return f2
        sw, swt, _ = engine.consensus_products([f1, np.asarray(f2, np.float64)])
        return [sw, swt]

    return c


def concatenate_samples(a, b):
    """stark/stark.py:23-24."""
    return np.vstack((a, b))


def permute_draws(draws, chains: int, seed: int, partition: int):
    """pystan 2 ``extract(permuted=True)`` order for one partition's P x (chains * n) matrix
    (chain-major columns): every chain's n draws in a random order, chains concatenated.
    The permutation is a pure function of (seed, partition, chain) -- numpy's Philox
    counter-based generator keyed by the sampling seed -- so a run is reproducible on 1 or N
    GPUs.  (pystan draws its permutations from numpy's global RandomState; the order is
    arbitrary either way, what matters to the reference's combine is that draw i of every
    partition is paired after the shuffle, stark/stark.py:20.)"""
    draws = np.asarray(draws)
    P, S = draws.shape
    if S % chains:
        raise ValueError("draw columns must be chains x draws")
    n = S // chains
    cols = []
    for c in range(chains):
        g = np.random.Generator(np.random.Philox(key=[int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                      (int(partition) << 32) | int(c)]))
        cols.append(c * n + g.permutation(n))
    return np.ascontiguousarray(draws[:, np.concatenate(cols)]) if cols else draws


def _extract_to_matrix(extract):
    """stark/stark.py:49-56: extract() values in key order, 1-D params as (S, 1) columns,
    hstack, transpose -> variables x samples."""
    h = [np.array(v) for v in extract.values()]
    for prm in h:
        if len(prm.shape) == 1:
            prm.shape = (prm.shape[0], 1)
    return np.transpose(np.hstack(h))


_CONTROL_KEYS = {"adapt_delta": "adapt_delta", "max_treedepth": "max_depth", "stepsize": "stepsize",
                 "adapt_gamma": "adapt_gamma", "adapt_kappa": "adapt_kappa", "adapt_t0": "adapt_t0",
                 "adapt_init_buffer": "adapt_init_buffer", "adapt_term_buffer": "adapt_term_buffer",
                 "adapt_window": "adapt_window", "adapt_engaged": "adapt_engaged", "inv_metric": "inv_metric",
                 "stepsize_jitter": "stepsize_jitter", "nuts_criterion": "nuts_criterion"}


def _unconstrain(family, data, init_dict):
    """Constrained parameter values (a pystan init dict) -> unconstrained vector."""
    if family == "schools":
        J = int(data["J"])
        eta = np.asarray(init_dict.get("eta", np.zeros(J)), np.float64).reshape(J)
        return np.concatenate([[float(init_dict.get("mu", 0.0)), np.log(float(init_dict.get("tau", 1.0)))], eta])
    K = int(data["K"])
    if family == "categorical":   # alpha[ncat - 1], then beta[K (ncat - 1)] column-major: Stan's own order, nothing constrained
        G = int(data["ncat"]) - 1
        return np.concatenate([np.asarray(init_dict.get("alpha", np.zeros(G)), np.float64).reshape(G),
                               np.asarray(init_dict.get("beta", np.zeros(G * K)), np.float64).reshape(G * K)])
    v = [float(init_dict.get("alpha", 0.0))] + list(np.asarray(init_dict.get("beta", np.zeros(K)), np.float64).reshape(K))
    if family in ("linear", "student_t"):
        v.append(np.log(float(init_dict.get("sigma", 1.0))))
    if family == "neg_binomial":
        v.append(np.log(float(init_dict.get("phi", 1.0))))
    if family == "gamma":
        v.append(np.log(float(init_dict.get("shape", 1.0))))
    return np.asarray(v)


NO_ANALYSIS_FAMILY = "neg_binomial"   # samples and combines; the analysis sweeps do not cover it
NO_ANALYSIS_FAMILIES = (NO_ANALYSIS_FAMILY, "student_t", "gamma", "categorical")   # Student-t, gamma and categorical likewise


def _refuse_analysis(family, what):
    """ValueError, before any sampling, where `what` is asked of the negative binomial, of Student-t or of gamma: the Hessian,
    log-predictive, PSIS-LOO, per-draw log-density, bootstrap and posterior predictive sweeps cover linear, logistic
    and poisson."""
    if family in NO_ANALYSIS_FAMILIES:
        raise ValueError(f"{what} is not available for the {family} family: the analysis sweeps (Hessian, "
                         "log-predictive, PSIS-LOO, per-draw log density, bootstrap, posterior predictive) cover the "
                         "linear, logistic and poisson families; sample it with NUTS and combine by consensus or "
                         "combiner='semiparametric'")


def _refuse_sparse(datas, what):
    """ValueError, before a model is built, where `what` is asked of partitions whose design matrix is sparse
    (a scipy.sparse data["x"]): the sparse storage serves the sampler and the combiners only."""
    for d in datas:
        if engine.is_sparse_shard({"x": d.get("x")}):
            raise ValueError(f"{what} is not available on sparse data: the analysis sweeps (Hessian, log-predictive, "
                             "PSIS-LOO, per-draw log density, bootstrap, posterior predictive) read dense rows; sparse "
                             "partitions sample and combine (concensusWeight with weights='sample', distribute)")


def unconstrain_draws(family, samples, n_cols=None):
    """The P x S constrained matrix ``concensusWeight`` returns (rows alpha, beta[1..d], [sigma], lp__)
    as the [S][D] unconstrained draws ``engine.Model.log_predictive`` scores: lp__ is dropped and
    linear's sigma becomes u = log sigma (the negative binomial's phi, in sigma's row, v = log phi, and student_t's
    sigma as linear's: their draws convert, though no analysis sweep scores them).  n_cols: the model's covariate count d, when known
    (``Stark.waic`` passes it); None takes it from the row count.
    ValueError for 8 schools (no log-predictive sweep), for P != D + 1 -- the draws of a ``pars=``
    selection cannot be scored: every parameter is needed -- and for a sigma <= 0 (names the draw)."""
    if family not in ("linear", "logistic", "poisson", "neg_binomial", "student_t", "gamma"):
        raise ValueError(f"draws of the {family} family cannot be scored: the log-predictive sweep covers the "
                         "regression families (linear, logistic, poisson), not 8 schools")
    m = np.asarray(samples, np.float64)
    if m.ndim != 2:
        raise ValueError(f"samples must be the P x S draw matrix, got shape {m.shape}")
    scale = {"linear": "sigma", "neg_binomial": "phi", "student_t": "sigma", "gamma": "shape"}.get(family)   # the positive parameter after beta, if any
    extra = 2 if scale else 1                           # parameters besides beta
    d = int(n_cols) if n_cols is not None else m.shape[0] - 1 - extra
    D = d + extra
    if d < 1 or m.shape[0] != D + 1:
        raise ValueError(f"samples has {m.shape[0]} rows, the {family} model with {max(d, 0)} covariates has D + 1 = "
                         f"{D + 1} (alpha, beta, {scale + ', ' if scale else ''}lp__): the draws of a pars= "
                         "selection cannot be scored")
    q = np.ascontiguousarray(m[:D].T)
    if scale:
        bad = np.flatnonzero(~(q[:, -1] > 0))
        if bad.size:
            raise ValueError(f"draw {int(bad[0])}: {scale} = {q[bad[0], -1]!r} is not positive")
        q[:, -1] = np.log(q[:, -1])
    return q


def thin_draws(draws, chains, thin):
    """Stan's num_thin: of each chain's post-warmup iterations m = 0, 1, ... keep those with
    m % thin == 0 (ceil(S / thin) draws per chain; services/util/generate_transitions), columns
    chain-major as the sampler writes them."""
    if thin == 1:
        return draws
    P, n = draws.shape
    return np.ascontiguousarray(draws.reshape(P, chains, n // chains)[:, :, ::thin].reshape(P, -1))


def sampling_config(family, datas, **kw):
    """pystan 2 ``StanModel.sampling`` keywords -> engine config (stark/stark.py:48)."""
    kw = dict(kw)
    it = int(kw.pop("iter", 2000))
    warmup = int(kw.pop("warmup", it // 2))
    chains = int(kw.pop("chains", 4))
    kw.pop("n_jobs", None)
    thin = int(kw.pop("thin", 1))
    if thin < 1:
        raise ValueError("thin must be a positive integer")
    seed = kw.pop("seed", None)
    if seed is None:
        seed = int(np.random.SeedSequence().entropy) & 0x7FFFFFFF
    control = dict(kw.pop("control", None) or {})
    metric = control.pop("metric", "diag_e")
    if metric not in engine.METRICS:
        raise ValueError(f"control['metric'] must be one of {sorted(engine.METRICS)}, got {metric!r}")
    cfg = dict(num_warmup=warmup, num_samples=it - warmup, chains=chains, seed=seed, thin=thin, metric=metric)
    for k, v in control.items():
        if k not in _CONTROL_KEYS:
            raise ValueError(f"unknown control key {k!r}")
        cfg[_CONTROL_KEYS[k]] = v
    init = kw.pop("init", "random")
    init_r = float(kw.pop("init_r", 2.0))
    cfg["init_radius"] = init_r
    if isinstance(init, (int, float)) or (isinstance(init, str) and init == "0"):
        if float(init) != 0.0:
            raise ValueError("numeric init must be 0")
        init = "0"
    if init == "0":
        D = [len(_unconstrain(family, d, {})) for d in datas]
        cfg["init"] = np.concatenate([np.zeros(Ds * chains) for Ds in D])
    elif callable(init):
        # pystan 2: init(chain_id=...) per chain when the function takes a chain_id, else init();
        # decided from the signature, so a TypeError raised inside the user's function propagates
        # (chain_id = 0 .. chains - 1: parity unpinned against pystan)
        try:
            params = inspect.signature(init).parameters
            takes_id = "chain_id" in params or any(p.kind == p.VAR_KEYWORD for p in params.values())
        except (TypeError, ValueError):          # no introspectable signature (some builtins)
            takes_id = False
        dicts = [init(chain_id=c) if takes_id else init() for c in range(chains)]
        cfg["init"] = np.concatenate([_unconstrain(family, d, dicts[c]) for d in datas for c in range(chains)])
    elif isinstance(init, (list, tuple)):
        if len(init) != chains:
            raise ValueError("init list must have one dict per chain")
        cfg["init"] = np.concatenate([_unconstrain(family, d, init[c]) for d in datas for c in range(chains)])
    elif init != "random":
        raise ValueError(f"unsupported init {init!r}")
    for k in ("sample_file", "diagnostic_file"):
        # pystan writes Stan CSV files here; this build returns draws only, so a caller who asks
        # for a file is told, not silently handed none
        if kw.pop(k, None) is not None:
            raise NotImplementedError(f"{k}= (pystan's CSV output) is not supported: the draws are returned in memory")
    for k in ("verbose", "refresh", "check_hmc_diagnostics", "algorithm"):
        v = kw.pop(k, None)
        if k == "algorithm" and v not in (None, "NUTS"):
            raise NotImplementedError("only algorithm='NUTS' is supported")
    if kw:
        raise TypeError(f"unsupported sampling arguments: {sorted(kw)}")
    return cfg


class Stark:
    """Driver of stark/stark.py:26-85 over GPU shards."""
    rdd = None
    n_partitions = None
    prepare_data_callback = None

    def __init__(self, context, rdd, prepare_data_callback):
        self.rdd = rdd
        self.context = context
        self.prepare_data_callback = prepare_data_callback
        self.n_partitions = self.rdd.getNumPartitions()
        self.family = None
        self.priors = {}
        self.last_run = None

    def setStanModel(self, **kwargs):
        """stark/stark.py:37-39; accepts pystan.StanModel's file= / model_code= (+ family=)."""
        self.family, self.priors = frontend.load_program_info(**kwargs)
        self.stan_kwargs = kwargs

    # ---- per-partition sampling (stark/stark.py:41-57), batched over partitions
    def _sample_partitions(self, datas, shard_ids=None, permuted=True, pars=None, include=True, laplace=False,
                           **kwargs):
        """Run every data dict as one shard of a single GPU model; returns one P x S matrix
        per data dict, rows in extract() order (params, transformed params, lp__), columns in
        ``extract(permuted=True)`` order (``permute_draws``) unless permuted=False.
        shard_ids: global partition index of each data dict (keys the RNG streams, so a
        partition samples identically on 1 or N GPUs).  pars / include: pystan 2's parameter
        selection (``frontend.select_pars``): only those rows (+ lp__) reach the P x S matrix,
        and so the combine, as in the reference (stark/stark.py:48-56).
        laplace: also fit every shard's Laplace approximation while the model is resident and return
        (draws, weights): weights[i] is the precision of the selected rows other than lp__."""
        if self.family is None:
            raise RuntimeError("call setStanModel() first")
        rows = [frontend.select_pars(self.family, d, pars, include) for d in datas]   # validates first
        if laplace:
            kwargs = dict(kwargs, laplace=True)           # the "sample" path calls _draw_partitions as before
        draws = self._draw_partitions(datas, shard_ids=shard_ids, permuted=permuted, **kwargs)
        out = [d if r is None else np.ascontiguousarray(d[r]) for d, r in zip(draws, rows)]
        if not laplace:
            return out
        weights = []
        for cov, r in zip(self._laplace_cov, rows):
            if r is not None:
                cov = cov[np.ix_(r[:-1], r[:-1])]     # the marginal of the selected rows (lp__ is r[-1])
            weights.append(np.linalg.inv(cov))
        return out, weights

    def _laplace_covariances(self, model, draws, ids):
        """Per local shard: the covariance (-H)^-1 of its Laplace approximation (engine.laplace on the
        analytic Hessian, started from the shard's draw mean), in the CONSTRAINED space of the draw
        rows other than lp__ -- linear: sigma = e^u, so row and column u are scaled by sigma_hat."""
        covs = []
        for s, d in enumerate(draws):
            D = model.D[s]
            q0 = np.asarray(d[:D], np.float64).mean(axis=1)
            if self.family == "linear":
                q0[-1] = np.log(q0[-1])
            try:
                mode, cov, _ = engine.laplace(model, [s], q0=q0)
            except ValueError as e:
                raise ValueError(f"partition {ids[s]}: no Laplace fit ({e})") from None
            if self.family == "linear":
                sig = float(np.exp(mode[-1]))
                cov = cov.copy()
                cov[-1, :] *= sig
                cov[:, -1] *= sig
            covs.append(cov)
        return covs

    def _draw_partitions(self, datas, shard_ids=None, permuted=True, laplace=False, **kwargs):
        """The GPU run behind _sample_partitions: every extract() row of every partition.
        laplace: the shards' Laplace covariances are fitted before the model is closed
        (self._laplace_cov, one per data dict)."""
        if laplace:
            _refuse_sparse(datas, "weights='laplace'")
        priors = dict(getattr(self, "priors", None) or {})
        model_kw = {}
        if self.family == "student_t":
            # nu: the statement's literal, else every partition's data["nu"] -- one model, so one value
            shards = [frontend.pack_data(self.family, d, nu=priors.get("nu")) for d in datas]
            nus = sorted({sh.pop("nu") for sh in shards})
            if len(nus) != 1:
                raise ValueError(f"student_t: the partitions' nu differ ({nus}): one model has one nu")
            model_kw["nu"] = nus[0]
            priors.pop("nu", None)
        else:
            shards = [frontend.pack_data(self.family, d) for d in datas]
        cfg = sampling_config(self.family, datas, **kwargs)
        if shard_ids is not None:
            cfg["shard_ids"] = shard_ids
        thin = cfg.pop("thin", 1)
        model = engine.Model(engine.default_context(), self.family, shards, **model_kw)
        if priors:
            model.set_prior(**priors)
        try:
            res = model.sample(**cfg)
            if laplace:
                ids = shard_ids if shard_ids is not None else range(len(datas))
                self._laplace_cov = self._laplace_covariances(model, res.draws, list(ids))
        finally:
            model.close()
        draws = [thin_draws(d, cfg["chains"], thin) for d in res.draws]
        if thin > 1:   # last_run holds what the caller got: the thinned draws and their stats
            idx = thin_draws(np.arange(res.chains * res.num_samples)[None, :], res.chains, thin)[0]
            res = engine.SampleResult(draws, [st[idx] for st in res.stats], res.info, res.chains, len(idx) // res.chains)
        res.info["metric"] = cfg["metric"]
        self.last_run = res
        if not permuted:
            return draws
        ids = shard_ids if shard_ids is not None else range(len(datas))
        return [permute_draws(d, cfg["chains"], cfg["seed"], p) for d, p in zip(draws, ids)]

    LAPLACE_MAX_COLS = 128    # the per-draw log-density sweep and the Hessian sweep cover d <= 128
    KHAT_WARN = 0.7           # above it the PSIS weights of a partition are not to be trusted

    def _laplace_partitions(self, datas, shard_ids=None, pars=None, include=True, want_weights=False, permuted=True,
                            **kwargs):
        """method="laplace" behind concensusWeight: every data dict as one shard of a single GPU model; per
        shard a Laplace fit and ``engine.laplace_sample`` with the partition's GLOBAL index as RNG stream.
        Returns (draws, weights, diagnostics): draws[i] is the P x S matrix of the NUTS path (constrained
        parameters -- linear: sigma = e^u -- then lp__ = the log density at the draw; pars / include select
        rows as there), S = ceil((iter - warmup) / thin) * chains; weights[i] the Laplace precision of the
        selected rows other than lp__ (want_weights, from the SAME fit) or None; diagnostics[i] the 1 x 2
        array [khat, ess].  permuted is accepted and ignored: the draws are exchangeable."""
        _refuse_sparse(datas, "method='laplace'")
        rows = [frontend.select_pars(self.family, d, pars, include) for d in datas]   # validates first
        cfg = sampling_config(self.family, datas, **kwargs)
        S = -(-cfg["num_samples"] // cfg["thin"]) * cfg["chains"]
        if S < 1:
            raise ValueError("method='laplace' needs at least one post-warmup draw (iter > warmup)")
        ids = list(shard_ids) if shard_ids is not None else list(range(len(datas)))
        shards = [frontend.pack_data(self.family, d) for d in datas]
        model = engine.Model(engine.default_context(), self.family, shards)
        if getattr(self, "priors", None):
            model.set_prior(**self.priors)
        draws, weights, diags = [], [], []
        try:
            for s, r in enumerate(rows):
                try:
                    fit = engine.laplace(model, [s])
                except ValueError as e:
                    raise ValueError(f"partition {ids[s]}: no Laplace fit ({e})") from None
                res = engine.laplace_sample(model, s, S, cfg["seed"], stream=ids[s], fit=fit)
                if res["khat"] > self.KHAT_WARN:
                    warnings.warn(f"partition {ids[s]}: Pareto khat = {res['khat']:.2f} > {self.KHAT_WARN} (ess = "
                                  f"{res['ess']:.0f} of {S} draws): its Laplace approximation is too far from the "
                                  "subposterior for the importance weights to be trusted -- sample this partition "
                                  "with NUTS (method='nuts')", RuntimeWarning, stacklevel=3)
                theta = res["draws"].T.copy()
                cov = res["cov"]
                if self.family == "linear":
                    theta[-1] = np.exp(theta[-1])
                    sig = float(np.exp(res["mode"][-1]))
                    cov = cov.copy()
                    cov[-1, :] *= sig
                    cov[:, -1] *= sig
                m = np.vstack([theta, res["lp"][None, :]])
                draws.append(np.ascontiguousarray(m if r is None else m[r]))
                if want_weights:
                    if r is not None:
                        cov = cov[np.ix_(r[:-1], r[:-1])]
                    weights.append(np.linalg.inv(cov))
                else:
                    weights.append(None)
                diags.append(np.array([[res["khat"], res["ess"]]]))
        finally:
            model.close()
        return draws, weights, diags

    def _run_laplace_distributed(self, parts, want_weights, **kwargs):
        """_run_distributed for method="laplace": partition p on rank p % world, its global index as the
        stream, so the results are the same at any rank count."""
        rank, ws = dist.world()
        mine = dist.local_partitions(len(parts), rank, ws)
        datas = [self.prepare_data_callback(list(parts[p])) for p in mine]
        for p, d in zip(mine, datas):
            if int(d["K"]) > self.LAPLACE_MAX_COLS:
                raise ValueError(f"method='laplace' covers at most {self.LAPLACE_MAX_COLS} covariates; partition {p} "
                                 f"has K = {int(d['K'])}")
        draws, weights, diags = (self._laplace_partitions(datas, shard_ids=mine, want_weights=want_weights, **kwargs)
                                 if datas else ([], [], []))
        n = len(parts)
        gd = dist.all_gather_partitions(dict(zip(mine, diags)), n)
        self.laplace_diagnostics = {"khat": [float(np.asarray(g)[0, 0]) for g in gd],
                                    "ess": [float(np.asarray(g)[0, 1]) for g in gd]}
        sub = dist.all_gather_partitions(dict(zip(mine, draws)), n)
        prec = dist.all_gather_partitions(dict(zip(mine, weights)), n) if want_weights else None
        return sub, prec

    def _mcmc(self, callback, **kwargs):
        def w(sts):
            sts = list(sts)
            data = callback(sts)
            return [self._sample_partitions([data], **kwargs)[0]]
        return w

    @staticmethod
    def _defaults(kwargs):
        if "iter" not in kwargs:
            kwargs["iter"] = 2000
        if "chains" not in kwargs:
            kwargs["chains"] = 1
        kwargs["n_jobs"] = 1
        return kwargs

    def _run_distributed(self, parts, laplace=False, **kwargs):
        rank, ws = dist.world()
        mine = dist.local_partitions(len(parts), rank, ws)
        datas = [self.prepare_data_callback(list(parts[p])) for p in mine]
        if not laplace:
            local = dict(zip(mine, self._sample_partitions(datas, shard_ids=mine, **kwargs))) if datas else {}
            return dist.all_gather_partitions(local, len(parts))
        draws, weights = self._sample_partitions(datas, shard_ids=mine, laplace=True, **kwargs) if datas else ([], [])
        return (dist.all_gather_partitions(dict(zip(mine, draws)), len(parts)),
                dist.all_gather_partitions(dict(zip(mine, weights)), len(parts)))

    def concensusWeight(self, separate_lp=False, weights="sample", method="nuts", combiner="consensus",
                        combiner_args=None, **kwargs):
        """stark/stark.py:59-71: subposterior per partition, consensus weighted average.

        combiner: "consensus" (default: the weighted average, everything below, bit for bit what omitting
        the argument gives) or "semiparametric": the same subposteriors, sampled by method= as below, go
        through ``engine.consensus_dpe``, the semiparametric density-product estimator, which does not
        assume Gaussian subposteriors (skewed or small shards).  lp__ (the last row)
        stays out of the product and is combined at the chosen draws.  ``combiner_args`` is a dict of
        consensus_dpe's options (T, chains, burn, thin, bandwidth); the sampling seed seeds the index
        chains too.  separate_lp and weights= have no meaning there: a non-default value raises ValueError
        before anything is sampled.  Every rank combines the gathered draws itself, so all ranks hold the
        same bits.  Works with method="nuts" and method="laplace" and every family, 8 schools included.

        method: "nuts" (default: every partition is sampled by NUTS, everything below, bit for bit what
        omitting the argument gives) or "laplace": every partition's draws are importance-resampled
        from its Laplace approximation (``engine.laplace_sample``: proposals from N(mode, (-H)^-1), PSIS-
        smoothed weights of target over proposal, stratified resampling), S = ceil((iter - warmup) / thin)
        * chains per partition.  The matrix has the NUTS path's shape, rows and pars= / include= handling
        (constrained parameters, lp__ = the log density at the draw) and goes through the same combine, so
        separate_lp and weights= keep their meaning; weights="laplace" reuses the fit.  Every partition's
        Pareto ``khat`` and ``ess`` = 1 / sum w^2 are kept in ``self.laplace_diagnostics``; a partition
        with khat > 0.7 raises a RuntimeWarning that names it: its subposterior is not near-Gaussian
        (few rows per covariate) and it should be sampled with NUTS.  The partition's global index is the
        RNG stream, so the result is the same on 1 or N ranks.  Regression families with at most 128
        covariates: ValueError for 8 schools and for more columns, before anything runs.

        weights: "sample" (default: the reference's W_s = inv(cov(draws_s)), everything below) or
        "laplace": W_s is the precision of shard s's Laplace approximation, -H_s at the shard's mode
        (engine.laplace on the analytic Hessian, fitted right after sampling from the shard's draw
        mean, in the constrained space of the draw rows; pars= / include= select its rows too), and
        lp__ gets its own 1 x 1 block as under separate_lp=True.  The sampled weights carry noise that
        falls only as 1 / draws (mean z^2 0.147 .. 0.034 at 100 .. 500 draws per
        chain); the Laplace weights carry none, and combined the same draws to 0.0005 there.  They are
        the right choice when every subposterior is near-Gaussian, i.e. n_s >> d rows per shard and
        (for poisson / logistic) no separation; for small or skewed shards the subposterior's spread
        is not (-H)^-1 and the sampled weights are the honest ones.  Regression families with at most
        128 covariates only: ValueError for 8 schools (raised before anything is sampled) and for a
        shard whose fit does not converge.

        The default reproduces the REFERENCE's combine, for parity: every extract() row is
        combined jointly, lp__ included.  That is not the accurate choice: each shard's lp__
        sits at its own offset, many lp__ sds from the others, and the sampled lp__-parameter
        cross-covariances turn that offset into an error of the parameter means (mean z^2 of
        4-7 at N = 1e8).  For accuracy pass separate_lp=True: lp__ gets a
        1 x 1 weight block of its own and the parameters are combined from their own
        covariance (engine.consensus).  permuted=False keeps chain order in the draws.

        chains= is any count >= 1 (default 1, stark/stark.py:62-63); the regression families run a
        count that is not one of 1, 2, 4, 8, 16, 64 as contiguous batches of those sizes
        (engine.chain_batches), one data sweep per batch and step.

        Raises stark_amd._lib.LinAlgError when a shard holds too few draws for
        its covariance to be invertible: each shard needs more than P draws, i.e.
        ceil((iter - warmup) / thin) * chains > P (P = the model's parameters + lp__; with separate_lp the
        parameters alone).  The reference's np.linalg.inv returns rounding noise there instead
        (DESIGN.md section 9)."""
        if weights not in ("sample", "laplace"):
            raise ValueError(f"weights must be 'sample' or 'laplace', got {weights!r}")
        if method not in ("nuts", "laplace"):
            raise ValueError(f"method must be 'nuts' or 'laplace', got {method!r}")
        if combiner not in ("consensus", "semiparametric"):
            raise ValueError(f"combiner must be 'consensus' or 'semiparametric', got {combiner!r}")
        if combiner == "consensus" and combiner_args:
            raise ValueError("combiner_args are the options of combiner='semiparametric'")
        if combiner == "semiparametric":
            if separate_lp or weights != "sample":
                raise ValueError("combiner='semiparametric' keeps lp__ out of the product and forms its own weights: "
                                 "separate_lp and weights= do not apply")
            args = dict(combiner_args or {})
            unknown = sorted(set(args) - {"T", "chains", "burn", "thin", "bandwidth"})
            if unknown:
                raise ValueError(f"combiner_args {unknown} are not options of engine.consensus_dpe "
                                 "(T, chains, burn, thin, bandwidth)")
            if kwargs.get("seed") is None:
                kwargs["seed"] = int(np.random.SeedSequence().entropy) & 0x7FFFFFFF
            if method == "laplace":
                if self.family is None:
                    raise RuntimeError("call setStanModel() first")
                _refuse_analysis(self.family, "method='laplace'")
                if self.family == "schools":
                    raise ValueError("method='laplace' needs a regression family (linear, logistic, poisson): "
                                     "8 schools has no Hessian or per-draw log-density sweep")
            seed = kwargs["seed"]
            kwargs = self._defaults(kwargs)
            parts = _rdd.partitions_of(self.rdd)
            if method == "laplace":
                sub, _ = self._run_laplace_distributed(parts, False, **kwargs)
            else:
                sub = self._run_distributed(parts, **kwargs)
            out, _, self.combiner_info = engine.consensus_dpe(sub, seed=seed, **args)
            return out
        if method == "laplace":
            if self.family is None:
                raise RuntimeError("call setStanModel() first")
            _refuse_analysis(self.family, "method='laplace'")
            if self.family == "schools":
                raise ValueError("method='laplace' needs a regression family (linear, logistic, poisson): "
                                 "8 schools has no Hessian or per-draw log-density sweep")
            kwargs = self._defaults(kwargs)
            parts = _rdd.partitions_of(self.rdd)
            sub, prec = self._run_laplace_distributed(parts, weights == "laplace", **kwargs)
            if prec is not None:
                out, _ = engine.consensus(sub, weights=prec)
            else:
                out, _ = engine.consensus(sub, separate_lp=separate_lp)
            return out
        if weights == "laplace":
            if self.family is None:
                raise RuntimeError("call setStanModel() first")
            _refuse_analysis(self.family, "weights='laplace'")
            if self.family == "schools":
                raise ValueError("weights='laplace' needs a regression family (linear, logistic, poisson): "
                                 "8 schools has no Hessian sweep")
        kwargs = self._defaults(kwargs)
        parts = _rdd.partitions_of(self.rdd)
        if weights == "laplace":
            subposteriors, precisions = self._run_distributed(parts, laplace=True, **kwargs)
            out, _ = engine.consensus(subposteriors, weights=precisions)
            return out
        subposteriors = self._run_distributed(parts, **kwargs)
        out, _ = engine.consensus(subposteriors, separate_lp=separate_lp)
        return out

    def _partition_totals(self, datas, q):
        """One model of this rank's partitions; their [8] totals of the pointwise log-predictive sweep
        over the draws q [S][D] (engine.Model.log_predictive, no per-row output), one per data dict."""
        shards = [frontend.pack_data(self.family, d) for d in datas]
        model = engine.Model(engine.default_context(), self.family, shards)
        try:
            return list(model.log_predictive(q))
        finally:
            model.close()

    def waic(self, samples):
        """WAIC of a P x S matrix of draws -- what ``concensusWeight`` returns, with either kind of
        weights, or one subposterior -- against EVERY partition's rows, without a full-data run.
        Every rank scores the partitions ``_run_distributed`` places on it (partition p on rank
        p % world) in one grouped launch; the [1, 8] totals are all-gathered and summed in partition
        order, so every rank returns the same bits on 1 or N ranks.  Returns ``engine.waic``'s dict
        (n, lppd, p_waic, elpd_waic, se, waic, n_high_var, n_non_finite) plus ``partition_totals``
        [n_partitions, 8].  Regression families with at most 128 covariates; ``unconstrain_draws``
        says which draws cannot be scored."""
        if self.family is None:
            raise RuntimeError("call setStanModel() first")
        _refuse_analysis(self.family, "waic")
        if self.family == "schools":
            unconstrain_draws(self.family, samples)       # raises: names the family
        parts = _rdd.partitions_of(self.rdd)
        rank, ws = dist.world()
        mine = dist.local_partitions(len(parts), rank, ws)
        datas = [self.prepare_data_callback(list(parts[p])) for p in mine]
        _refuse_sparse(datas, "waic")
        q = unconstrain_draws(self.family, samples, n_cols=int(datas[0]["K"]) if datas else None)
        local = {}
        if datas:
            tots = self._partition_totals(datas, q)
            local = {p: np.asarray(t, np.float64).reshape(1, 8) for p, t in zip(mine, tots)}
        totals = np.concatenate([np.asarray(t, np.float64).reshape(1, 8)
                                 for t in dist.all_gather_partitions(local, len(parts))])
        out = engine.waic(totals)
        out["partition_totals"] = totals
        return out

    LOO_MAX_DRAWS = 1024      # stk_loo keeps a row tile's S log ratios in LDS

    def _partition_loo_totals(self, datas, q):
        """``_partition_totals`` for the PSIS-LOO sweep (engine.Model.loo, no per-row output)."""
        shards = [frontend.pack_data(self.family, d) for d in datas]
        model = engine.Model(engine.default_context(), self.family, shards)
        try:
            return list(model.loo(q))
        finally:
            model.close()

    def loo(self, samples):
        """PSIS-LOO of a P x S matrix of draws against EVERY partition's rows, exchanged exactly as
        ``waic`` does it: every rank scores its own partitions in one grouped launch, the [1, 8] totals
        are all-gathered and summed in partition order, so every rank returns the same bits on 1 or N
        ranks.  Returns ``engine.loo``'s dict (n, lppd, p_loo, elpd_loo, se, looic, n_k_gt_0.5,
        n_k_gt_0.7, n_non_finite) plus ``partition_totals`` [n_partitions, 8].  Regression families
        with at most 128 covariates and at most 1024 draws: more columns raise ValueError."""
        if self.family is None:
            raise RuntimeError("call setStanModel() first")
        _refuse_analysis(self.family, "loo")
        if self.family == "schools":
            unconstrain_draws(self.family, samples)       # raises: names the family
        S = np.asarray(samples).shape[-1] if np.ndim(samples) == 2 else 0
        if S > self.LOO_MAX_DRAWS:
            raise ValueError(f"samples has S = {S} draws; the PSIS-LOO sweep keeps every row's draws in LDS and covers "
                             f"at most {self.LOO_MAX_DRAWS}: pass a column subset (e.g. samples[:, ::{-(-S // self.LOO_MAX_DRAWS)}])")
        parts = _rdd.partitions_of(self.rdd)
        rank, ws = dist.world()
        mine = dist.local_partitions(len(parts), rank, ws)
        datas = [self.prepare_data_callback(list(parts[p])) for p in mine]
        _refuse_sparse(datas, "loo")
        q = unconstrain_draws(self.family, samples, n_cols=int(datas[0]["K"]) if datas else None)
        local = {}
        if datas:
            tots = self._partition_loo_totals(datas, q)
            local = {p: np.asarray(t, np.float64).reshape(1, 8) for p, t in zip(mine, tots)}
        totals = np.concatenate([np.asarray(t, np.float64).reshape(1, 8)
                                 for t in dist.all_gather_partitions(local, len(parts))])
        out = engine.loo(totals)
        out["partition_totals"] = totals
        return out

    PPC_MAX_COLS = 128        # the posterior predictive sweep covers d <= 128

    def ppc(self, samples, seed=0):
        """Posterior predictive checks of a P x S matrix of draws against EVERY partition's rows: would data
        simulated from this fit look like the data?  For every (row, draw) a replicate y_rep is drawn on the
        device from the family's sampling distribution; per draw, the replicated data set's mean, sd, max, min
        and fraction of zeros and the Pearson discrepancy chi2 are compared with the observed ones.  Exchanged
        exactly as ``waic`` does it: every rank scores its own partitions in one grouped launch with RNG stream =
        the partition's global index, the per-partition [S, 8] and [8] arrays are all-gathered and pooled in
        partition order, so every rank returns the same bits on 1 or N ranks.  Returns ``engine.ppc``'s dict
        (per statistic "obs", "rep" [S] and the posterior predictive p-value "p"; n; n_non_finite) plus
        ``partition_stats`` [n_partitions, S, 8] and ``partition_obs`` [n_partitions, 8].  Regression families
        with at most 128 covariates: ValueError otherwise, before a model is built."""
        if self.family is None:
            raise RuntimeError("call setStanModel() first")
        _refuse_analysis(self.family, "ppc")
        if self.family not in ("linear", "logistic", "poisson"):
            raise ValueError(f"no ppc for the {self.family} family: the posterior predictive sweep covers the "
                             "regression families (linear, logistic, poisson), not 8 schools")
        parts = _rdd.partitions_of(self.rdd)
        rank, ws = dist.world()
        mine = dist.local_partitions(len(parts), rank, ws)
        datas = [self.prepare_data_callback(list(parts[p])) for p in mine]
        _refuse_sparse(datas, "ppc")
        for p, d in zip(mine, datas):
            if int(d["K"]) > self.PPC_MAX_COLS:
                raise ValueError(f"ppc covers at most {self.PPC_MAX_COLS} covariates; partition {p} has K = "
                                 f"{int(d['K'])}")
        q = unconstrain_draws(self.family, samples, n_cols=int(datas[0]["K"]) if datas else None)
        S = q.shape[0]
        local = {}
        if datas:
            model = engine.Model(engine.default_context(), self.family, [frontend.pack_data(self.family, d) for d in datas])
            try:
                stats, obs = model.posterior_predict(q, seed=seed, streams=list(mine))
            finally:
                model.close()
            local = {p: np.concatenate([np.asarray(st, np.float64).reshape(-1), np.asarray(ob, np.float64).reshape(-1)])
                     .reshape(1, S * 8 + 8) for p, st, ob in zip(mine, stats, obs)}
        every = np.concatenate([np.asarray(t, np.float64).reshape(1, S * 8 + 8)
                                for t in dist.all_gather_partitions(local, len(parts))])
        pstats, pobs = every[:, :S * 8].reshape(len(parts), S, 8), np.ascontiguousarray(every[:, S * 8:])
        out = engine.ppc(pstats, pobs)
        out["partition_stats"], out["partition_obs"] = pstats, pobs
        return out

    BOOT_MAX_COLS = 128       # the weighted bootstrap sweep and the Hessian sweep cover d <= 128
    BOOT_WEIGHTS = {"bayesian": "exponential", "poisson": "poisson"}

    def bootstrap(self, n=200, weights="bayesian", seed=0, pars=None, include=True):
        """n bootstrap replicates of the FULL-DATA maximiser -- the mode the reference's README names next
        ("if MAP estimates were found instead of full posteriors then one might have something akin to a
        distributed bootstrap"): a P x n matrix with the rows of ``concensusWeight`` (constrained
        parameters -- linear: sigma = e^u -- then lp__ = the replicate's weighted log density at its
        maximiser; pars / include select rows as there).  weights: "bayesian" (Exp(1) row weights: the
        weighted-likelihood bootstrap, whose replicates are approximate posterior draws that do not lean on
        the model being right) or "poisson" (Poisson(1): the classical bootstrap).

        Partitions are placed on ranks as ``waic`` places them and a partition's global index is its RNG
        stream; every iteration's per-partition blocks are all-gathered and summed in partition order
        (the ``combine`` of ``engine.laplace`` and ``engine.bootstrap``), so every rank takes identical steps and
        returns the same matrix, bit for bit, on 1 or N ranks.
        ``self.bootstrap_diagnostics`` keeps ``iterations``, ``converged`` and ``wsum`` per replicate.
        Regression families with at most 128 covariates: ValueError otherwise, before a model is built."""
        if self.family is None:
            raise RuntimeError("call setStanModel() first")
        _refuse_analysis(self.family, "bootstrap")
        if self.family not in ("linear", "logistic", "poisson"):
            raise ValueError(f"no bootstrap for the {self.family} family: the weighted bootstrap sweep covers the "
                             "regression families (linear, logistic, poisson), not 8 schools")
        if weights not in self.BOOT_WEIGHTS:
            raise ValueError(f"weights must be one of {sorted(self.BOOT_WEIGHTS)}, got {weights!r}")
        parts = _rdd.partitions_of(self.rdd)
        rank, ws = dist.world()
        mine = dist.local_partitions(len(parts), rank, ws)
        datas = [self.prepare_data_callback(list(parts[p])) for p in mine]
        _refuse_sparse(datas, "bootstrap")
        for p, d in zip(mine, datas):
            if int(d["K"]) > self.BOOT_MAX_COLS:
                raise ValueError(f"bootstrap covers at most {self.BOOT_MAX_COLS} covariates; partition {p} has K = "
                                 f"{int(d['K'])}")
        rows = [frontend.select_pars(self.family, d, pars, include) for d in datas]   # validates first
        if not datas:
            raise ValueError(f"rank {rank} holds no partition: bootstrap needs at most as many ranks as partitions")
        n_parts = len(parts)

        def combine(blocks):             # [local partitions, R, D + 2] -> the sum over ALL partitions, in their order
            every = dist.all_gather_partitions({p: np.ascontiguousarray(b) for p, b in zip(mine, blocks)}, n_parts)
            tot = np.array(every[0], np.float64)
            for b in every[1:]:
                tot = tot + np.asarray(b, np.float64)
            return tot

        model = engine.Model(engine.default_context(), self.family, [frontend.pack_data(self.family, d) for d in datas])
        try:
            if getattr(self, "priors", None):
                model.set_prior(**self.priors)
            try:
                fit = engine.laplace(model, combine=combine)      # the same partition-order sums
            except ValueError as e:
                raise ValueError(f"no Laplace fit of the full data ({e})") from None
            res = engine.bootstrap(model, int(n), kind=self.BOOT_WEIGHTS[weights], seed=seed, streams=list(mine),
                                   combine=combine, fit=fit)
        finally:
            model.close()
        self.bootstrap_diagnostics = {k: res[k] for k in ("iterations", "converged", "wsum")}
        theta = res["estimates"].T.copy()
        if self.family == "linear":
            theta[-1] = np.exp(theta[-1])
        m = np.vstack([theta, res["lp"][None, :]])
        return np.ascontiguousarray(m if rows[0] is None else m[rows[0]])

    def distribute(self, n=2, reference_union=False, **kwargs):
        """stark/stark.py:73-85: naive parallel runs over the full data, draws stacked with
        ``concatenate_samples`` (row blocks of P x S)."""
        kwargs = self._defaults(kwargs)
        parts = _rdd.partitions_of(self.rdd)
        full = [row for p in parts for row in p]
        if reference_union and n >= 2:
            runs = parts + [full]
        else:
            runs = [full] * n
        posteriors = self._run_distributed(runs, **kwargs)
        out = posteriors[0]
        for b in posteriors[1:]:
            out = concatenate_samples(out, b)
        return out
