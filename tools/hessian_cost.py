#!/usr/bin/env python3
"""What the analytic Hessian sweep costs at the headline shape, against what it replaces.

Workload: BASELINE configs[3]'s model, 8 synthetic logistic shards x 1.25e7 rows x d = 100, on one
GPU.  In one process, alternating between the three:
  analytic    stk_log_density_hessian(shard = -1, lp = grad = NULL): the Hessians of all shards, one
              sweep launch and one reduce launch (k_hessian, k_hessian_reduce);
  difference  tools.laplace.hessian over all shards: the central difference of the gradient, 2 D
              points in batches of 16 chains -- the path the sweep supersedes;
  sweep step  sweep_ms / sweeps of a 16-chain sampler on the same model (k_sweep16), with the
              context's profiling on.
Every one is timed with a HIP event pair on the context's stream after a warm-up of all three;
medians and the spread over `--repeats` rounds are reported.  The two Hessians are compared.
Every GPU step (building the model, the warm-up, each timed pass) runs under its own time limit:
a step that overruns ends the process (SIGALRM).

Writes profiles/<run>_hessian_cost.json and prints the same JSON line.
usage: tools/hessian_cost.py --run r15a [--rows 1e8 --d 100 --shards 8 --repeats 10]"""
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
    p.add_argument("--run", default="r15a", help="prefix of the profile file")
    p.add_argument("--rows", type=float, default=1e8, help="total rows over all shards")
    p.add_argument("--d", type=int, default=100)
    p.add_argument("--shards", type=int, default=8)
    p.add_argument("--chains", type=int, default=16)
    p.add_argument("--repeats", type=int, default=10)
    p.add_argument("--steps", type=int, default=4, help="sampler steps per round")
    p.add_argument("--seed", type=int, default=20240)
    p.add_argument("--step-limit", type=int, default=120, help="seconds every GPU step may take")
    p.add_argument("--out", default=None)
    a = p.parse_args()

    import torch
    from stark_amd import _lib, engine, fulldata
    from tools import laplace as L

    torch.cuda.set_device(0)
    with limit(a.step_limit):
        ctx = fulldata.context_on_torch_stream(0)      # torch events bracket the library's kernels
        n = int(a.rows) // a.shards
        model = engine.Model.synthetic(ctx, "logistic", a.shards, n, a.d, data_seed=a.seed)
        ctx.sync()
    D = a.d + 1
    beta = engine.Model.gen_beta(a.seed, a.d)
    q = np.concatenate([[0.0], beta])                  # the generating point: every shard near its mode
    Q = np.ascontiguousarray(np.tile(q, (a.shards, 1)))
    H = np.empty((a.shards, D, D))
    hess_fn = _lib.load().stk_log_density_hessian

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def analytic():
        engine.check(hess_fn(model._h, -1, Q.ctypes.data, None, None, H.ctypes.data))
        return H.sum(axis=0)

    sampler = model.sampler(num_warmup=150, num_samples=100000, chains=a.chains, seed=a.seed + 1,
                            stepsize_jitter=0.5, nuts_criterion="stan2.23")

    def sweep_pass():
        ctx.set_profiling(1)
        i0 = sampler.info()
        sampler.run(max_steps=a.steps)
        i1 = sampler.info()
        ctx.set_profiling(0)
        k = i1["sweeps"] - i0["sweeps"]
        return (i1["sweep_ms"] - i0["sweep_ms"]) / k if k else None

    with limit(a.step_limit):                          # warm-up of all three
        sampler.run(max_steps=10)
        _, Ha = timed(analytic)
        sd = np.sqrt(np.diag(np.linalg.inv(-Ha)))
        _, Hd = timed(lambda: L.hessian(model, range(a.shards), q, 0.1 * sd))
        sweep_pass()
    an_ms, df_ms, sw_ms, full_ms = [], [], [], []
    for _ in range(a.repeats):
        with limit(a.step_limit):
            an_ms.append(timed(analytic)[0])
        with limit(a.step_limit):
            df_ms.append(timed(lambda: L.hessian(model, range(a.shards), q, 0.1 * sd))[0])
        with limit(a.step_limit):
            v = sweep_pass()
            if v is not None:
                sw_ms.append(v)
        with limit(a.step_limit):                      # the Python wrapper: lp and grad too (8 C = 1 sweeps)
            full_ms.append(timed(lambda: model.hessian(None, Q))[0])

    nt = (a.d + 2 + 15) // 16
    mfma_flop = a.shards * ((n + 15) // 16) * (nt * (nt + 1) // 2) * 4 * 2048     # issued on the MFMA pipe
    useful_flop = a.shards * n * D * (D + 1)                                       # the upper triangle's FMAs
    an, df, sw = stats(an_ms), stats(df_ms), stats(sw_ms)
    tfs = mfma_flop / (an["median"] * 1e-3) / 1e12
    rec = {"tool": "tools/hessian_cost.py", "device": torch.cuda.get_device_name(0),
           "config": {"family": "logistic", "shards": a.shards, "rows_per_shard": n, "d": a.d, "chains": a.chains,
                      "repeats": a.repeats, "steps_per_round": a.steps},
           "launch": engine.hessian_launch(n, a.d),
           "analytic_hessian_all_shards_ms": an, "difference_hessian_all_shards_ms": df, "sweep16_step_ms": sw,
           "model_hessian_with_lp_grad_ms": stats(full_ms),
           "mfma_flop": mfma_flop, "useful_flop": useful_flop,
           "analytic_mfma_tflops": tfs, "analytic_share_of_fp64_peak": tfs / FP64_PEAK_TFS,
           "analytic_useful_tflops": useful_flop / (an["median"] * 1e-3) / 1e12,
           "analytic_x_read_tb_per_s": a.shards * n * a.d * 8 / (an["median"] * 1e-3) / 1e12,
           "ratio_analytic_over_difference": an["median"] / df["median"],
           "ratio_analytic_over_sweep_step": an["median"] / sw["median"],
           "bar": "the analytic Hessian is faster than the difference Hessian (ratio < 1)",
           "bar_met": bool(an["median"] < df["median"]),
           "max_abs_difference_over_max_abs_h": float(np.abs(Ha - Hd).max() / np.abs(Ha).max())}
    out = a.out or os.path.join(ROOT, "profiles", f"{a.run}_hessian_cost.json")
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
