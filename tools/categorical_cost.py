#!/usr/bin/env python3
"""Sweep time per step of the categorical family (k_sweep_cat) against the logistic family's k_sweep16 on the same X,
in one process (tools/gamma_cost.py's method), at the shapes (K, d) given: by default (3, 100), (5, 64) and (9, 32).

Per shape the two models hold the same X (host rows); categorical its classes 1 .. K, logistic 1[y = 1]: one pass of
k_sweep_cat over X feeds G = K - 1 class tiles where the logistic sweep feeds one, so the yardstick is G logistic
sweeps.  Per arm a fresh adaptive sampler runs --steps state-machine steps with HIP events around every step's sweeps
(stk_ctx_set_profiling); the figure is sweep_ms / sweeps.  Arms alternate, --repeats times; medians are reported, and
per shape the ratio categorical / (G x logistic).  A ratio above 1 is reported as it is: the tool sets no bar.

--isa: the per-element vector-instruction counts read from the code objects (given by the caller: they need the
build's object files, not a device).  One JSON line on stdout, the same object to --out.
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
p.add_argument("--shapes", default="3x100,5x64,9x32", help="K x d, comma separated")
p.add_argument("--shards", type=int, default=8)
p.add_argument("--chains", type=int, default=16)
p.add_argument("--steps", type=int, default=60)
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--isa", default=None, help="JSON object recorded as is under 'isa'")
p.add_argument("--out", default=None)
a = p.parse_args()

n = int(a.rows)
ctx = engine.Context(0, profiling=True)
shapes = []
for spec in a.shapes.split(","):
    K, d = (int(v) for v in spec.split("x"))
    G = K - 1
    rng = np.random.default_rng(20310 + 1000 * K + d)
    coef = np.concatenate([rng.normal(0, 0.5, G), rng.normal(0, 1 / np.sqrt(d), G * d)])
    cat, logi = [], []
    for s in range(a.shards):
        X = rng.uniform(-1.7, 1.7, (n, d))
        eta = np.concatenate([coef[:G][None, :] + X @ coef[G:].reshape(G, d).T, np.zeros((n, 1))], axis=1)
        pr = np.exp(eta - eta.max(1, keepdims=True))
        pr /= pr.sum(1, keepdims=True)
        y = (1 + (rng.uniform(size=(n, 1)) > np.cumsum(pr, axis=1)[:, :-1]).sum(1)).astype(np.int32)
        cat.append({"x": X, "y": y})
        logi.append({"x": X, "y": (y == 1).astype(np.int32)})
    models = {"categorical": engine.Model(ctx, "categorical", cat, ncat=K), "logistic": engine.Model(ctx, "logistic", logi)}
    del cat, logi
    ms = {k: [] for k in models}
    for r in range(a.repeats):
        for fam, m in models.items():
            s = m.sampler(num_warmup=150, num_samples=105, chains=a.chains, seed=20311 + r, shard_ids=list(range(a.shards)))
            s.run(255, max_steps=a.steps)
            info = s.info()
            s.close()
            ms[fam].append(info["sweep_ms"] / max(info["sweeps"], 1))
    for m in models.values():
        m.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    shapes.append({"K": K, "G": G, "d": d, "batches": engine.chain_batches(a.chains, d, ncat=K),
                   "logistic_sweep": engine.sweep_launch(n, d, 16) if a.chains == 16 else None,
                   "bytes_per_sweep": a.shards * n * (8 * d + 4), "ms": ms, "median_ms": med,
                   "categorical_over_logistic": med["categorical"] / med["logistic"],
                   "categorical_over_G_logistic": med["categorical"] / (G * med["logistic"])})
out = {"what": "sweep time per step (sweep_ms / sweeps, HIP events around every step's sweeps), a categorical and a logistic "
               "model on the same X in one process, arms alternating; medians over the repeats; the logistic kernels are the "
               "parent commit's, byte for byte (the code-object comparison of the same run)",
       "rows_per_shard": n, "shards": a.shards, "chains": a.chains, "steps": a.steps, "repeats": a.repeats,
       "shapes": shapes, "isa": json.loads(a.isa) if a.isa else None}
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
print(json.dumps(out), flush=True)
ctx.close()
