#!/usr/bin/env python3
"""What the weighted bootstrap sweep costs at the headline shape, against its unweighted floor.

Workload: BASELINE configs[3]'s model, 8 synthetic logistic shards x 1.25e7 rows x d = 100, on one GPU, at
16 points: the generating point plus N(0, 1e-3) noise.  In one process, alternating:
  boot exponential   stk_log_density_grad_boot(shard = -1, R = 16, kind 1): one 16-replicate weighted sweep
  boot poisson       the same with kind 0              (k_boot16 + k_boot_reduce) over every shard;
  sweep step         stk_log_density_grad_chains at the same 16 points per shard: one 16-chain sweep step
                     (k_sweep16) and its reduce -- the same bytes and the same MFMAs without weights, the
                     natural floor.
Each is timed with a HIP event pair on the context's stream after a warm-up of all three (the entry points
copy their small host arguments inside the window, as a caller pays for them); medians and the spread over
`--repeats` rounds are reported, with the two ratios boot / sweep step.  The ratio has no bar: no earlier
route computes these numbers.
--pipeline also times engine.bootstrap at B = --pipeline-replicates on the same model for both kinds (wall
clock, the Laplace fit apart) and records its iteration counts.  Every GPU step runs under its own time
limit: a step that overruns ends the process.

Writes profiles/<run>_boot_cost.json and prints the same JSON line.
usage: tools/boot_cost.py --run r20a [--rows 1e8 --d 100 --shards 8 --repeats 5 --pipeline]"""
import argparse
import contextlib
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FP64_PEAK_TFS = 78.6    # MI355X fp64 matrix spec, dense (bench.py's figure)


@contextlib.contextmanager
def limit(seconds):
    """The step's own time limit: SIGALRM's default action ends the process."""
    signal.alarm(int(seconds))
    try:
        yield
    finally:
        signal.alarm(0)


def stats(v):
    v = np.asarray(v, float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--run", default="r20a", help="prefix of the profile file")
    p.add_argument("--rows", type=float, default=1e8, help="total rows over all shards")
    p.add_argument("--d", type=int, default=100)
    p.add_argument("--shards", type=int, default=8)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--seed", type=int, default=20240)
    p.add_argument("--step-limit", type=int, default=120, help="seconds every GPU step may take")
    p.add_argument("--pipeline", action="store_true", help="also time engine.bootstrap for both kinds")
    p.add_argument("--pipeline-replicates", type=int, default=256)
    p.add_argument("--out", default=None)
    a = p.parse_args()

    import torch
    from stark_amd import engine, fulldata

    torch.cuda.set_device(0)
    with limit(a.step_limit):
        ctx = fulldata.context_on_torch_stream(0)      # torch events bracket the library's kernels
        n = int(a.rows) // a.shards
        model = engine.Model.synthetic(ctx, "logistic", a.shards, n, a.d, data_seed=a.seed)
        ctx.sync()
    D = a.d + 1
    q = np.concatenate([[0.0], engine.Model.gen_beta(a.seed, a.d)])      # the generating point
    Q = np.ascontiguousarray(q[None, :] + np.random.default_rng(a.seed).normal(0, 1e-3, (16, D)))
    Q16 = np.ascontiguousarray(np.broadcast_to(Q, (a.shards, 16, D)))

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    passes = {"boot_exponential": lambda: model.log_density_grad_boot(Q, None, seed=a.seed, kind="exponential")[0],
              "boot_poisson": lambda: model.log_density_grad_boot(Q, None, seed=a.seed, kind="poisson")[0],
              "sweep": lambda: model.log_density_grad_chains(Q16)[0]}
    with limit(a.step_limit):                          # warm-up of all three
        first = {k: timed(f)[1] for k, f in passes.items()}
    ms = {k: [] for k in passes}
    for _ in range(a.repeats):
        for k, f in passes.items():
            with limit(a.step_limit):
                t, out = timed(f)
                ms[k].append(t)
                assert np.array_equal(out, first[k], equal_nan=True), k   # the same bits every pass
    # a sanity figure, no bar: weights of mean 1 over n rows move lp by about |lp| / sqrt(n) * a few
    rel = {k: float(np.abs(first[k] / first["sweep"] - 1).max()) for k in ("boot_exponential", "boot_poisson")}

    kf, jt = (a.d + 3) // 4, ((a.d + 3) // 4 + 3) // 4
    mfma_flop = a.shards * ((n + 15) // 16) * (kf + 4 * jt) * 2048        # forward + backward tiles, padded
    be, bp, sw = stats(ms["boot_exponential"]), stats(ms["boot_poisson"]), stats(ms["sweep"])
    rec = {"tool": "tools/boot_cost.py", "device": torch.cuda.get_device_name(0),
           "config": {"family": "logistic", "shards": a.shards, "rows_per_shard": n, "d": a.d, "replicates": 16,
                      "repeats": a.repeats},
           "launch": engine.boot_launch(n, a.d), "sweep16_launch": engine.sweep_launch(n, a.d, 16),
           "boot_exponential_ms": be, "boot_poisson_ms": bp, "sweep16_step_ms": sw,
           "ratio_exponential_over_sweep_step": be["median"] / sw["median"],
           "ratio_poisson_over_sweep_step": bp["median"] / sw["median"],
           "bar": "none: the ratio is recorded, not judged",
           "max_relative_shift_of_lp_against_unweighted": rel,
           "mfma_flop": mfma_flop,
           "boot_exponential_mfma_tflops": mfma_flop / (be["median"] * 1e-3) / 1e12,
           "boot_exponential_share_of_fp64_peak": mfma_flop / (be["median"] * 1e-3) / 1e12 / FP64_PEAK_TFS,
           "sweep16_mfma_tflops": mfma_flop / (sw["median"] * 1e-3) / 1e12,
           "x_read_tb_per_s": a.shards * n * a.d * 8 / (be["median"] * 1e-3) / 1e12}

    if a.pipeline:
        with limit(a.step_limit):
            t0 = time.perf_counter()
            fit = engine.laplace(model, q0=q)
            t_fit = time.perf_counter() - t0
        rec["bootstrap_pipeline"] = {"replicates": a.pipeline_replicates, "laplace_fit_s": t_fit}
        for kind in ("exponential", "poisson"):
            with limit(max(a.step_limit, 600)):
                t0 = time.perf_counter()
                res = engine.bootstrap(model, a.pipeline_replicates, kind=kind, seed=a.seed, fit=fit)
                wall = time.perf_counter() - t0
            it = res["iterations"]
            ratio = res["estimates"].var(axis=0, ddof=1) / np.diag(res["cov"])
            rec["bootstrap_pipeline"][kind] = {
                "wall_s": wall, "converged": int(res["converged"].sum()), "iterations_min": int(it.min()),
                "iterations_max": int(it.max()), "sweeps": int(sum(it[t:t + 16].max() + 1 for t in range(0, it.size, 16))),
                "variance_over_laplace_variance_min": float(np.nanmin(ratio)),
                "variance_over_laplace_variance_max": float(np.nanmax(ratio))}

    out = a.out or os.path.join(ROOT, "profiles", f"{a.run}_boot_cost.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))
    model.close()
    ctx.close()


if __name__ == "__main__":
    main()
