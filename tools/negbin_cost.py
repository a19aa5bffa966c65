#!/usr/bin/env python3
"""What the negative binomial's count-table terms cost in the reduce, and that the cost does not grow with n.

The terms are added once per (shard, chain) by k_sweep_reduce_nb's scalar block from the shard's table of tail
counts (entries: min(max y, 1024) + the distinct counts past 1024).  For each row count in --rows, three shards
of the same X with counts that give a table of 1, ~300 and 1024 + 50 entries; per arm a sampler runs --steps
state-machine steps (sweep + reduce + NUTS step per step) and the wall time per step after a synchronise is
taken; arms alternate, --repeats times, medians reported.  The table terms' cost is the difference to the
1-entry arm at the same n.  One JSON line on stdout, the same object to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stark_amd import engine  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--rows", type=int, nargs="+", default=[4096, 65536])
p.add_argument("--d", type=int, default=20)
p.add_argument("--chains", type=int, default=16)
p.add_argument("--steps", type=int, default=400)
p.add_argument("--repeats", type=int, default=5)
p.add_argument("--out", default=None)
a = p.parse_args()

rng = np.random.default_rng(7)
ctx = engine.Context(0)
out = {"what": "wall time per sampler step (sweep + reduce + NUTS step), neg_binomial shards whose count tables have "
               "1, 300 and 1074 entries, at each row count; medians over alternating repeats",
       "d": a.d, "chains": a.chains, "steps": a.steps, "repeats": a.repeats, "rows": {}}
for n in a.rows:
    X = rng.uniform(-1.7, 1.7, (n, a.d))
    i = np.arange(n)
    counts = {"entries_1": (i % 2), "entries_300": (i % 301), "entries_1074": np.where(i < 50, 5000 + 7 * i, i % 1025)}
    models = {k: engine.Model(ctx, "neg_binomial", [{"x": X, "y": y.astype(np.int32)}]) for k, y in counts.items()}
    us = {k: [] for k in counts}
    for r in range(a.repeats):
        for k, m in models.items():
            s = m.sampler(num_warmup=1000, num_samples=10, chains=a.chains, seed=11 + r)
            s.run(1010, max_steps=20)                     # first launches
            ctx.sync()
            t0 = time.perf_counter()
            s.run(1010, max_steps=a.steps)
            ctx.sync()
            us[k].append((time.perf_counter() - t0) / a.steps * 1e6)
            s.close()
    med = {k: float(np.median(v)) for k, v in us.items()}
    out["rows"][str(n)] = {"us_per_step": us, "median_us_per_step": med,
                           "table_terms_us": {k: med[k] - med["entries_1"] for k in med if k != "entries_1"}}
    for m in models.values():
        m.close()
line = json.dumps(out)
if a.out:
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
print(line, flush=True)
ctx.close()
