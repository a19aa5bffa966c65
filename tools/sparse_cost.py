#!/usr/bin/env python
"""Cost of the sparse sweep (k_sweep_sp) against the dense sweep on the same rows, densified.

    python tools/sparse_cost.py [--out profiles/NAME.json] [--shards 8] [--rows 200000] [--reps 5]
                                [--families logistic,neg_binomial] [--shapes 128:8,1024:16]

Per family (logistic and the heaviest residual, neg_binomial) and shape (d = 128 with K = 8 entries per row, d = 1024
with K = 16), at the shape's largest sparse batch size C = engine.chain_batches(., d, sparse=True)[0]: one model of
`shards` sparse shards and one of the same rows as dense doubles, and the lp / gradient of C points per shard through
Model.log_density_grad_shards -- one sweep launch over all the shards plus one reduce launch.  The two models are
called alternately in one process, `reps` times each after a warm-up call; the medians are reported.  A call's wall
time holds the sweep, the reduce and the transfers of the points and results, so the same call on models of one row per
shard (same d, same C) is timed as the call's floor and reported beside it: ms_sweep = ms_call - ms_floor.

Bytes: the sparse sweep's algorithmic traffic (padded rows 12 K n, y, beta in and one partial row out per chunk and
chain) over the 12 K n bytes of the layout, and the dense sweep's n (8 d + y) for comparison.  Needs a GPU and scipy."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(128, 8), (1024, 16)]
FAMILIES = ["logistic", "neg_binomial"]


def make_rows(n, d, K, family, rng):
    import scipy.sparse as sp
    cols = np.sort(np.argsort(rng.random((n, d)), axis=1)[:, :K] if d <= 128 else
                   (rng.integers(0, d // K, (n, K)) + (d // K) * np.arange(K)[None, :]), axis=1)   # K distinct columns per row
    indptr = np.arange(n + 1, dtype=np.int64) * K
    X = sp.csr_matrix((np.ones(n * K), cols.reshape(-1).astype(np.int32), indptr), shape=(n, d))
    beta = rng.normal(0, 1 / np.sqrt(K), d)
    eta = 0.2 + X @ beta
    if family == "logistic":
        y = (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(np.int32)
    else:
        y = rng.poisson(np.exp(np.clip(eta, -5, 4)) * rng.gamma(3.0, 1 / 3.0, n)).astype(np.int32)
    return X, y


def timed(model, q, ctx):
    ctx.sync()
    t = time.perf_counter()
    model.log_density_grad_shards(q)
    return 1e3 * (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--families", default=",".join(FAMILIES))
    ap.add_argument("--shapes", default=",".join(f"{d}:{K}" for d, K in SHAPES), help="d:K pairs")
    a = ap.parse_args()
    families = a.families.split(",")
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    from stark_amd import engine
    ctx = engine.Context(0)
    results = []
    for family in families:
        for d, K in shapes:
            rng = np.random.default_rng(1000 * d + K)
            C = engine.chain_batches(64, d, sparse=True)[0]
            D = d + (1 if family == "logistic" else 2)
            X, y = make_rows(a.rows, d, K, family, rng)
            Xd = np.asarray(X.todense(), np.float64)
            q = rng.normal(0, 0.1, (a.shards, C, D))
            # every shard holds the same rows: the cost does not depend on them being different, the host memory does
            models = {"sparse": engine.Model(ctx, family, [{"x": X, "y": y}] * a.shards),
                      "dense": engine.Model(ctx, family, [{"x": Xd, "y": y}] * a.shards),
                      "sparse_floor": engine.Model(ctx, family, [{"x": X[:1], "y": y[:1]}] * a.shards),
                      "dense_floor": engine.Model(ctx, family, [{"x": Xd[:1], "y": y[:1]}] * a.shards)}
            del Xd
            try:
                lps, _ = models["sparse"].log_density_grad_shards(q)      # warm-up, and the two storages agree
                lpd, _ = models["dense"].log_density_grad_shards(q)
                assert np.allclose(lps, lpd, rtol=1e-9), float(np.abs(lps / lpd - 1).max())
                for k in ("sparse_floor", "dense_floor"):
                    models[k].log_density_grad_shards(q)
                ms = {k: [] for k in models}
                for _ in range(a.reps):
                    for k in models:                                      # alternating
                        ms[k].append(timed(models[k], q, ctx))
                med = {k: float(np.median(v)) for k, v in ms.items()}
                info = models["sparse"].sparse_info(0)
                assert info["bytes"] == 12 * K * a.rows, info               # the layout's bytes, not a measurement
                sl = engine.sparse_launch(a.rows, d, K, C)
                dl = engine.sweep_launch(a.rows, d, C)
                ybytes = 4
                pw = D + 1 + (1 if family == "neg_binomial" else 0)
                sparse_bytes = a.shards * (info["bytes"] + ybytes * a.rows + sl["G"] * C * 8 * (d + 1 + pw))
                dense_bytes = a.shards * a.rows * (8 * d + ybytes)
                rec = {"family": family, "d": d, "K": K, "C": C, "shards": a.shards, "rows_per_shard": a.rows,
                       "ms_call": med, "ms_call_all": ms,
                       "ms_sweep_sparse": med["sparse"] - med["sparse_floor"], "ms_sweep_dense": med["dense"] - med["dense_floor"],
                       "dense_over_sparse": (med["dense"] - med["dense_floor"]) / max(med["sparse"] - med["sparse_floor"], 1e-6),
                       "sparse_launch": sl, "dense_launch": dl, "ell_bytes_per_shard": info["bytes"],
                       "sparse_bytes": sparse_bytes, "sparse_bytes_over_ell": sparse_bytes / (a.shards * info["bytes"]),
                       "dense_bytes": dense_bytes, "dense_bytes_over_sparse_bytes": dense_bytes / sparse_bytes,
                       "sparse_GBps": sparse_bytes / max(med["sparse"] - med["sparse_floor"], 1e-6) / 1e6,
                       "dense_GBps": dense_bytes / max(med["dense"] - med["dense_floor"], 1e-6) / 1e6}
                results.append(rec)
                print(json.dumps({k: rec[k] for k in ("family", "d", "K", "C", "ms_sweep_sparse", "ms_sweep_dense",
                                                       "dense_over_sparse", "sparse_bytes_over_ell", "sparse_GBps",
                                                       "dense_GBps")}), flush=True)
            finally:
                for m in models.values():
                    m.close()
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/sparse_cost.py", "timing": "wall time of Model.log_density_grad_shards, medians of "
                       f"{a.reps} alternating calls; ms_sweep = ms_call - ms_floor (one-row shards)", "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
