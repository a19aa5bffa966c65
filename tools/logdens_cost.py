#!/usr/bin/env python3
"""What the per-draw log-density sweep costs at the headline shape, against the routes that existed before it.

Workload: BASELINE configs[3]'s model, 8 synthetic logistic shards x 1.25e7 rows x d = 100, on one
GPU, at S = 1024 draws: the generating point plus N(0, 1e-3) noise.  In one process, alternating:
  logdens     stk_log_density_draws(shard = -1): lp of every shard at the S draws, one preparation launch,
              one sweep launch and one reduce launch (k_predictive_prep, k_logdens, k_logdens_reduce);
  sweep step  stk_log_density_grad_chains at 16 points per shard: one 16-chain sweep step (k_sweep16) and
              its reduce -- forward AND backward, X read once per 16 draws.  S / 16 of them are the only
              route to the same S numbers without k_logdens;
  predictive  stk_log_predictive(shard = -1, rows = NULL) at the same S: k_predictive, the kernel that
              shares its forward half with k_logdens (draw_forward.h; recorded for comparison, no bar).
Each is timed with a HIP event pair on the context's stream after a warm-up of all three (the entry
points copy their small host arguments inside the window, as a caller pays for them); medians and the
spread over `--repeats` rounds are reported.  The bar is the existing route, not a fixed time: all
shards at S draws must take less than S / 16 sweep steps (ratio < 1, no margin).
--pipeline also times Laplace sampling as concensusWeight(method="laplace") runs it -- per shard a
Laplace fit and engine.laplace_sample at --pipeline-draws draws, then the combine -- on the same model
(wall clock), and sets its smallest importance ESS per second next to the NUTS bench recorded in
--nuts-bench.  Every GPU step runs under its own time limit: a step that overruns ends the process.

Writes profiles/<run>_logdens_cost.json and prints the same JSON line.
usage: tools/logdens_cost.py --run r19a [--rows 1e8 --d 100 --shards 8 --draws 1024 --repeats 5 --pipeline]"""
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
    p.add_argument("--run", default="r19a", help="prefix of the profile file")
    p.add_argument("--rows", type=float, default=1e8, help="total rows over all shards")
    p.add_argument("--d", type=int, default=100)
    p.add_argument("--shards", type=int, default=8)
    p.add_argument("--draws", type=int, default=1024)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--seed", type=int, default=20240)
    p.add_argument("--step-limit", type=int, default=120, help="seconds every GPU step may take")
    p.add_argument("--pipeline", action="store_true", help="also time Laplace sampling of every shard + combine")
    p.add_argument("--pipeline-draws", type=int, default=16000, help="draws per shard (the bench: 16 chains x 1000)")
    p.add_argument("--nuts-bench", default=os.path.join(ROOT, "profiles", "r06ak_bench.json"))
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
    D, S = a.d + 1, a.draws
    q = np.concatenate([[0.0], engine.Model.gen_beta(a.seed, a.d)])      # the generating point
    Q = np.ascontiguousarray(q[None, :] + np.random.default_rng(a.seed).normal(0, 1e-3, (S, D)))
    Q16 = np.ascontiguousarray(np.broadcast_to(Q[:16], (a.shards, 16, D)))

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    passes = {"logdens": lambda: model.log_density(Q),
              "sweep": lambda: model.log_density_grad_chains(Q16)[0],
              "predictive": lambda: model.log_predictive(Q)}
    with limit(a.step_limit):                          # warm-up of all three
        first = {k: timed(f)[1] for k, f in passes.items()}
    ms = {k: [] for k in passes}
    for _ in range(a.repeats):
        for k, f in passes.items():
            with limit(a.step_limit):
                t, out = timed(f)
                ms[k].append(t)
                assert np.array_equal(out, first[k], equal_nan=True), k   # the same bits every pass
    # the two routes give the same numbers: the first 16 draws, in units of the density bar 1e-10 |lp|
    agree = float((np.abs(first["logdens"][:, :16] - first["sweep"]) / (1e-10 * np.abs(first["sweep"]))).max())

    tiles = a.shards * ((n + 15) // 16) * ((S + 15) // 16)
    mfma_flop = tiles * ((a.d + 3) // 4) * 2048                           # issued on the MFMA pipe
    ld, sw, pd = stats(ms["logdens"]), stats(ms["sweep"]), stats(ms["predictive"])
    steps = S / 16
    tfs = mfma_flop / (ld["median"] * 1e-3) / 1e12
    ratio = ld["median"] / (steps * sw["median"])
    rec = {"tool": "tools/logdens_cost.py", "device": torch.cuda.get_device_name(0),
           "config": {"family": "logistic", "shards": a.shards, "rows_per_shard": n, "d": a.d, "draws": S,
                      "repeats": a.repeats},
           "launch": engine.logdens_launch(n, a.d, S),
           "logdens_all_shards_ms": ld, "sweep16_step_ms": sw, "sweep16_steps_compared": steps,
           "sweep16_steps_ms": steps * sw["median"], "predictive_all_shards_ms": pd,
           "ratio_logdens_over_sweep_steps": ratio,
           "ratio_logdens_over_predictive": ld["median"] / pd["median"],
           "bar": "all shards at S draws take less than S / 16 sixteen-chain sweep steps "
                  "(stk_log_density_grad_chains; ratio < 1)",
           "bar_met": bool(ratio < 1.0),
           "logdens_vs_sweep_lp_in_density_bars": agree,
           "mfma_flop": mfma_flop, "logdens_mfma_tflops": tfs, "logdens_share_of_fp64_peak": tfs / FP64_PEAK_TFS,
           "ps_per_row_and_draw": ld["median"] * 1e9 / (a.shards * n * S),
           "x_read_tb_per_s": a.shards * n * a.d * 8 / (ld["median"] * 1e-3) / 1e12}

    if a.pipeline:
        Sp = a.pipeline_draws
        t0 = time.perf_counter()
        draws, khat, ess, t_fit = [], [], [], 0.0
        for s in range(a.shards):
            with limit(a.step_limit):
                tf = time.perf_counter()
                fit = engine.laplace(model, [s], q0=q)
                t_fit += time.perf_counter() - tf
                res = engine.laplace_sample(model, s, Sp, a.seed, stream=s, fit=fit)
            draws.append(np.ascontiguousarray(np.vstack([res["draws"].T, res["lp"][None, :]])))
            khat.append(res["khat"])
            ess.append(res["ess"])
        with limit(a.step_limit):
            out, used = engine.consensus(draws, ctx, separate_lp=True)
        wall = time.perf_counter() - t0
        rec["laplace_pipeline"] = {"draws_per_shard": Sp, "wall_s": wall, "fit_s": t_fit, "khat": khat, "ess": ess,
                                   "min_ess": float(min(ess)), "min_ess_per_s": float(min(ess)) / wall,
                                   "shards_used": int(np.sum(used)), "finite": bool(np.isfinite(out).all()),
                                   "note": "ess is the importance-sampling 1 / sum w^2 of a shard's proposals; wall "
                                           "covers every shard's Newton fit from the generating point, its "
                                           "proposals, weights and resampling, and the combine"}
        if os.path.exists(a.nuts_bench):
            nb = json.load(open(a.nuts_bench))
            nuts_wall = nb["setup_s"]["adaptation"] + nb["setup_s"]["post_warmup_draws"]
            rec["nuts_bench_recorded"] = {"file": os.path.relpath(a.nuts_bench, ROOT), "wall_s": nuts_wall,
                                          "min_ess": nb["min_ess"], "min_ess_per_s": nb["min_ess"] / nuts_wall}
            rec["laplace_over_nuts_min_ess_per_s"] = rec["laplace_pipeline"]["min_ess_per_s"] / (nb["min_ess"] / nuts_wall)

    out = a.out or os.path.join(ROOT, "profiles", f"{a.run}_logdens_cost.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))
    model.close()
    ctx.close()


if __name__ == "__main__":
    main()
