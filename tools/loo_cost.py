#!/usr/bin/env python3
"""What the PSIS-LOO sweep costs at the headline shape, against the log-predictive (WAIC) sweep.

Workload: BASELINE configs[3]'s model, 8 synthetic logistic shards x 1.25e7 rows x d = 100, on one
GPU, scored against S draws (1024 and 256 by default): the generating point plus N(0, 1e-3) noise.  In
one process, for every S, alternating between the two:
  loo         stk_loo(shard = -1, rows = NULL): k_predictive_prep, k_loo, k_draw_totals;
  predictive  stk_log_predictive(shard = -1, rows = NULL) at the same S: k_predictive_prep,
              k_predictive, k_draw_totals -- the same forward pass without the sort and the fit.
Each pass is timed with a HIP event pair on the context's stream after a warm-up of both; medians and
the spread over `--repeats` rounds are reported, and their ratio.  There is no bar: no earlier path
computes PSIS-LOO.  Every GPU step (building the model, the warm-up, each timed pass) runs under its
own time limit: a step that overruns ends the process (SIGALRM).

Writes profiles/<run>_loo_cost.json and prints the same JSON line.
usage: tools/loo_cost.py --run r18a [--rows 1e8 --d 100 --shards 8 --draws 1024,256 --repeats 5]"""
import argparse
import contextlib
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    p.add_argument("--run", default="r18a", help="prefix of the profile file")
    p.add_argument("--rows", type=float, default=1e8, help="total rows over all shards")
    p.add_argument("--d", type=int, default=100)
    p.add_argument("--shards", type=int, default=8)
    p.add_argument("--draws", default="1024,256", help="comma-separated S values")
    p.add_argument("--repeats", type=int, default=5)
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
    D = a.d + 1
    q = np.concatenate([[0.0], engine.Model.gen_beta(a.seed, a.d)])      # the generating point
    lib = _lib.load()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    cases = []
    for S in (int(s) for s in a.draws.split(",")):
        Q = np.ascontiguousarray(q[None, :] + np.random.default_rng(a.seed).normal(0, 1e-3, (S, D)))
        tot = np.empty((a.shards, 8))

        def run(fn):
            engine.check(fn(model._h, -1, Q.ctypes.data, S, None, tot.ctypes.data))
            return tot.copy()

        with limit(a.step_limit):                      # warm-up of both
            _, first_loo = timed(lambda: run(lib.stk_loo))
            _, first_pd = timed(lambda: run(lib.stk_log_predictive))
        loo_ms, pd_ms = [], []
        for _ in range(a.repeats):
            with limit(a.step_limit):
                ms, t = timed(lambda: run(lib.stk_loo))
                loo_ms.append(ms)
                assert np.array_equal(t, first_loo, equal_nan=True)      # the same bits every pass
            with limit(a.step_limit):
                ms, t = timed(lambda: run(lib.stk_log_predictive))
                pd_ms.append(ms)
                assert np.array_equal(t, first_pd, equal_nan=True)
        lo, pd = stats(loo_ms), stats(pd_ms)
        cases.append({"draws": S, "launch": engine.loo_launch(n, a.d, S),
                      "predictive_launch": engine.predictive_launch(n, a.d, S),
                      "loo_all_shards_ms": lo, "predictive_all_shards_ms": pd,
                      "ratio_loo_over_predictive": lo["median"] / pd["median"],
                      "loo_ns_per_row_and_draw": lo["median"] * 1e6 / (a.shards * n * S),
                      "loo_us_per_16_row_tile": lo["median"] * 1e3 / (a.shards * ((n + 15) // 16)),
                      "x_read_tb_per_s": a.shards * n * a.d * 8 / (lo["median"] * 1e-3) / 1e12,
                      "loo": engine.loo(first_loo), "waic": engine.waic(first_pd)})
    rec = {"tool": "tools/loo_cost.py", "device": torch.cuda.get_device_name(0),
           "config": {"family": "logistic", "shards": a.shards, "rows_per_shard": n, "d": a.d, "repeats": a.repeats},
           "bar": "none: no earlier path computes PSIS-LOO; the log-predictive sweep at the same S is the yardstick",
           "cases": cases}
    out = a.out or os.path.join(ROOT, "profiles", f"{a.run}_loo_cost.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))
    model.close()
    ctx.close()


if __name__ == "__main__":
    main()
