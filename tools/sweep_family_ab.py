#!/usr/bin/env python3
"""Sweep time per step of the Poisson, the negative-binomial and the logistic family on the same rows, in
one process.

The models hold the same X (host rows: the count families have no synthetic generator) and counts
y ~ Poisson(exp(eta)) / their indicator y > 0, so the sweeps stream the same n (8d + 4) bytes and
differ in the residual only (the negative binomial also in its reduce, which adds the count table's terms).  Per arm a fresh adaptive sampler runs --steps state-machine steps with
HIP events around every step's sweeps (stk_ctx_set_profiling); the figure is sweep_ms / sweeps.  Arms
alternate, --repeats times.  One JSON line on stdout, the same object to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stark_amd import engine  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--rows", type=float, default=2e5, help="rows per shard")
p.add_argument("--d", type=int, default=100)
p.add_argument("--shards", type=int, default=8)
p.add_argument("--chains", type=int, default=16)
p.add_argument("--steps", type=int, default=60)
p.add_argument("--repeats", type=int, default=3)
p.add_argument("--out", default=None)
a = p.parse_args()

n, d = int(a.rows), a.d
rng = np.random.default_rng(20240)
beta = rng.normal(0, 1 / np.sqrt(d), d)
pois, logi = [], []
for s in range(a.shards):
    X = rng.uniform(-1.7, 1.7, (n, d))
    y = rng.poisson(np.exp(0.3 + X @ beta)).astype(np.int32)
    pois.append({"x": X, "y": y})
    logi.append({"x": X, "y": (y > 0).astype(np.int32)})
ctx = engine.Context(0, profiling=True)
models = {"poisson": engine.Model(ctx, "poisson", pois), "neg_binomial": engine.Model(ctx, "neg_binomial", pois),
          "logistic": engine.Model(ctx, "logistic", logi)}
del pois, logi
launch = engine.sweep_launch(n, d, a.chains if a.chains in (1, 2, 4, 8, 16, 64) else engine.chain_batches(a.chains, d)[0])
ms = {"poisson": [], "neg_binomial": [], "logistic": []}
for r in range(a.repeats):
    for fam in ("poisson", "neg_binomial", "logistic"):
        s = models[fam].sampler(num_warmup=150, num_samples=105, chains=a.chains, seed=20241 + r,
                                shard_ids=list(range(a.shards)))
        s.run(255, max_steps=a.steps)
        info = s.info()
        s.close()
        ms[fam].append(info["sweep_ms"] / max(info["sweeps"], 1))
out = {"what": "sweep time per step (sweep_ms / sweeps, HIP events around every step's sweeps), poisson, neg_binomial "
               "and logistic models on the same X in one process, arms alternating",
       "rows_per_shard": n, "d": d, "shards": a.shards, "chains": a.chains, "steps": a.steps, "sweep": launch,
       "bytes_per_sweep": a.shards * n * (8 * d + 4),
       "poisson_ms": ms["poisson"], "logistic_ms": ms["logistic"],
       "neg_binomial_ms": ms["neg_binomial"],
       "poisson_over_logistic": [x / y for x, y in zip(ms["poisson"], ms["logistic"])],
       "neg_binomial_over_logistic": [x / y for x, y in zip(ms["neg_binomial"], ms["logistic"])],
       "neg_binomial_over_poisson": [x / y for x, y in zip(ms["neg_binomial"], ms["poisson"])],
       "median_ms": {k: float(np.median(v)) for k, v in ms.items()}}
line = json.dumps(out)
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
print(line, flush=True)
for m in models.values():
    m.close()
ctx.close()
