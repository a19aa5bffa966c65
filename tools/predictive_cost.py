#!/usr/bin/env python3
"""What the pointwise log-predictive sweep costs at the headline shape, against the sampler's own sweep.

Workload: BASELINE configs[3]'s model, 8 synthetic logistic shards x 1.25e7 rows x d = 100, on one
GPU, scored against S = 1024 draws: the generating point plus N(0, 1e-3) noise.  In one process,
alternating between the two:
  predictive  stk_log_predictive(shard = -1, rows = NULL): the totals of all shards, one preparation
              launch, one sweep launch and one reduce launch (k_predictive_prep, k_predictive,
              k_draw_totals);
  sweep step  sweep_ms / sweeps of a 16-chain sampler on the same model (k_sweep16), with the
              context's profiling on.  S / 16 of them see as many (row, draw) pairs as the predictive
              sweep does -- forward AND backward, with X read S / 16 times instead of once.
The predictive pass is timed with a HIP event pair on the context's stream after a warm-up of both;
medians and the spread over `--repeats` rounds are reported.  The bar is the existing kernel, not a
fixed time: all shards at S draws must take less than S / 16 sweep steps (ratio < 1, no margin).
Every GPU step (building the model, the warm-up, each timed pass) runs under its own time limit: a
step that overruns ends the process (SIGALRM).

Writes profiles/<run>_predictive_cost.json and prints the same JSON line.
usage: tools/predictive_cost.py --run r16a [--rows 1e8 --d 100 --shards 8 --draws 1024 --repeats 5]"""
import argparse
import contextlib
import json
import os
import signal
import sys

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
    p.add_argument("--run", default="r16a", help="prefix of the profile file")
    p.add_argument("--rows", type=float, default=1e8, help="total rows over all shards")
    p.add_argument("--d", type=int, default=100)
    p.add_argument("--shards", type=int, default=8)
    p.add_argument("--draws", type=int, default=1024)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--steps", type=int, default=4, help="sampler steps per round")
    p.add_argument("--seed", type=int, default=20240)
    p.add_argument("--step-limit", type=int, default=120, help="seconds every GPU step may take")
    p.add_argument("--out", default=None)
    a = p.parse_args()

    import torch
    from stark_amd import _lib, engine, fulldata

    torch.cuda.set_device(0)
    with limit(a.step_limit):
        ctx = fulldata.context_on_torch_stream(0)      # torch events bracket the library's kernels
        n = int(a.rows) // a.shards
        model = engine.Model.synthetic(ctx, "logistic", a.shards, n, a.d, data_seed=a.seed)
        ctx.sync()
    D, S = a.d + 1, a.draws
    q = np.concatenate([[0.0], engine.Model.gen_beta(a.seed, a.d)])      # the generating point
    Q = np.ascontiguousarray(q[None, :] + np.random.default_rng(a.seed).normal(0, 1e-3, (S, D)))
    tot = np.empty((a.shards, 8))
    fn = _lib.load().stk_log_predictive

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def predictive():
        engine.check(fn(model._h, -1, Q.ctypes.data, S, None, tot.ctypes.data))
        return tot.copy()

    sampler = model.sampler(num_warmup=150, num_samples=100000, chains=16, seed=a.seed + 1,
                            stepsize_jitter=0.5, nuts_criterion="stan2.23")

    def sweep_pass():
        ctx.set_profiling(1)
        i0 = sampler.info()
        sampler.run(max_steps=a.steps)
        i1 = sampler.info()
        ctx.set_profiling(0)
        k = i1["sweeps"] - i0["sweeps"]
        return (i1["sweep_ms"] - i0["sweep_ms"]) / k if k else None

    with limit(a.step_limit):                          # warm-up of both
        sampler.run(max_steps=10)
        _, first = timed(predictive)
        sweep_pass()
    pd_ms, sw_ms = [], []
    for _ in range(a.repeats):
        with limit(a.step_limit):
            ms, t = timed(predictive)
            pd_ms.append(ms)
            assert np.array_equal(t, first, equal_nan=True)              # the same bits every pass
        with limit(a.step_limit):
            v = sweep_pass()
            if v is not None:
                sw_ms.append(v)

    tiles = a.shards * ((n + 15) // 16) * ((S + 15) // 16)
    mfma_flop = tiles * ((a.d + 3) // 4) * 2048                           # issued on the MFMA pipe
    pd, sw = stats(pd_ms), stats(sw_ms)
    steps = S / 16
    tfs = mfma_flop / (pd["median"] * 1e-3) / 1e12
    ratio = pd["median"] / (steps * sw["median"])
    w = engine.waic(first)
    rec = {"tool": "tools/predictive_cost.py", "device": torch.cuda.get_device_name(0),
           "config": {"family": "logistic", "shards": a.shards, "rows_per_shard": n, "d": a.d, "draws": S,
                      "repeats": a.repeats, "steps_per_round": a.steps},
           "launch": engine.predictive_launch(n, a.d, S),
           "predictive_all_shards_ms": pd, "sweep16_step_ms": sw, "sweep16_steps_compared": steps,
           "sweep16_steps_ms": steps * sw["median"],
           "ratio_predictive_over_sweep_steps": ratio,
           "bar": "all shards at S draws take less than S / 16 sixteen-chain sweep steps (ratio < 1)",
           "bar_met": bool(ratio < 1.0),
           "mfma_flop": mfma_flop, "predictive_mfma_tflops": tfs, "predictive_share_of_fp64_peak": tfs / FP64_PEAK_TFS,
           "ns_per_row_and_draw": pd["median"] * 1e6 / (a.shards * n * S),
           "x_read_tb_per_s": a.shards * n * a.d * 8 / (pd["median"] * 1e-3) / 1e12,
           "waic": w}
    out = a.out or os.path.join(ROOT, "profiles", f"{a.run}_predictive_cost.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))
    sampler.close()
    model.close()
    ctx.close()


if __name__ == "__main__":
    main()
