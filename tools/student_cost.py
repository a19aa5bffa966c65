#!/usr/bin/env python3
"""Sweep time per step of the Student-t, the linear and the negative-binomial family on the same rows, in one
process (tools/sweep_family_ab.py's method).

The three models hold the same X (host rows); student_t and linear the same double y, the negative binomial the
counts round(|y|) as int32, so the sweeps stream the same X and differ in the residual (and in 4 bytes of y per row
for the count family).  Per arm a fresh adaptive sampler runs --steps state-machine steps with HIP events around
every step's sweeps (stk_ctx_set_profiling); the figure is sweep_ms / sweeps.  Arms alternate, --repeats times;
medians are reported.  --isa: the per-element vector-instruction counts read from the code objects (given by the
caller: they need the build's object files, not a device).  One JSON line on stdout, the same object to --out.
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
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--nu", type=float, default=4.0)
p.add_argument("--hbm-peak-gbs", type=float, default=8000.0, help="HBM peak of the device, GB/s (MI355X: 8 TB/s)")
p.add_argument("--isa", default=None, help="JSON object recorded as is under 'isa'")
p.add_argument("--out", default=None)
a = p.parse_args()

n, d = int(a.rows), a.d
rng = np.random.default_rng(20240)
beta = rng.normal(0, 1 / np.sqrt(d), d)
real, cnt = [], []
for s in range(a.shards):
    X = rng.uniform(-1.7, 1.7, (n, d))
    y = 0.3 + X @ beta + rng.standard_t(4, n)
    real.append({"x": X, "y": y})
    cnt.append({"x": X, "y": np.minimum(np.round(np.abs(y)), 2 ** 31 - 1).astype(np.int32)})
ctx = engine.Context(0, profiling=True)
models = {"student_t": engine.Model(ctx, "student_t", real, nu=a.nu), "linear": engine.Model(ctx, "linear", real),
          "neg_binomial": engine.Model(ctx, "neg_binomial", cnt)}
del real, cnt
launch = engine.sweep_launch(n, d, a.chains if a.chains in (1, 2, 4, 8, 16, 64) else engine.chain_batches(a.chains, d)[0])
ms = {k: [] for k in models}
for r in range(a.repeats):
    for fam in models:
        s = models[fam].sampler(num_warmup=150, num_samples=105, chains=a.chains, seed=20241 + r,
                                shard_ids=list(range(a.shards)))
        s.run(255, max_steps=a.steps)
        info = s.info()
        s.close()
        ms[fam].append(info["sweep_ms"] / max(info["sweeps"], 1))
med = {k: float(np.median(v)) for k, v in ms.items()}
nbytes = {"student_t": a.shards * n * (8 * d + 8), "linear": a.shards * n * (8 * d + 8), "neg_binomial": a.shards * n * (8 * d + 4)}
out = {"what": "sweep time per step (sweep_ms / sweeps, HIP events around every step's sweeps), student_t, linear and "
               "neg_binomial models on the same X in one process, arms alternating; medians over the repeats",
       "rows_per_shard": n, "d": d, "shards": a.shards, "chains": a.chains, "steps": a.steps, "repeats": a.repeats, "nu": a.nu,
       "sweep": launch, "bytes_per_sweep": nbytes, "ms": ms, "median_ms": med,
       "student_t_over_linear": med["student_t"] / med["linear"],
       "student_t_over_neg_binomial": med["student_t"] / med["neg_binomial"],
       "hbm_peak_gbs": a.hbm_peak_gbs,
       "fraction_of_hbm_peak": {k: nbytes[k] / (med[k] * 1e-3) / (a.hbm_peak_gbs * 1e9) for k in med},
       "isa": json.loads(a.isa) if a.isa else None}
line = json.dumps(out)
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
print(line, flush=True)
for m in models.values():
    m.close()
ctx.close()
