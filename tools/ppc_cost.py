#!/usr/bin/env python3
"""What the posterior predictive sweep costs at the headline shape, against the log-predictive sweep.

Workload: BASELINE configs[3]'s model, 8 synthetic logistic shards x 1.25e7 rows x d = 100, on one GPU,
against S = 1024 and S = 256 draws: the generating point plus N(0, 1e-3) noise.  In one process, alternating
between the two at the same S:
  ppc         stk_posterior_predict(shard = -1, stats and obs only): one preparation launch, one sweep launch,
              one launch over y and one reduce launch (k_predictive_prep, k_yrep, k_yobs, k_yrep_reduce);
  predictive  stk_log_predictive(shard = -1, rows = NULL): the totals of all shards (k_predictive_prep,
              k_predictive, k_draw_totals).
Both read X once and form the same eta on the fp64 MFMA; the ppc sweep adds a Philox call and the generator per
(row, draw) where the predictive sweep has a log1p and a streaming logsumexp.  Each pass is timed with a HIP event
pair on the context's stream after a warm-up of both; medians and the spread over `--repeats` rounds are reported.
There is no bar -- no earlier path computes replicates: the numbers to report are the ratio to the log-predictive
sweep at the same S and the time per (row, draw).  Every GPU step (building the model, the warm-up, each timed pass)
runs under its own time limit: a step that overruns ends the process (SIGALRM).

Writes profiles/<run>_ppc_cost.json and prints the same JSON line.
usage: tools/ppc_cost.py --run r23a [--rows 1e8 --d 100 --shards 8 --draws 1024,256 --repeats 5]"""
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
    p.add_argument("--run", default="r23a", help="prefix of the profile file")
    p.add_argument("--rows", type=float, default=1e8, help="total rows over all shards")
    p.add_argument("--d", type=int, default=100)
    p.add_argument("--shards", type=int, default=8)
    p.add_argument("--draws", default="1024,256")
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
    for S in (int(v) for v in a.draws.split(",")):
        Q = np.ascontiguousarray(q[None, :] + np.random.default_rng(a.seed).normal(0, 1e-3, (S, D)))
        st, ob, tot = np.empty((a.shards, S, 8)), np.empty((a.shards, 8)), np.empty((a.shards, 8))

        def ppc():
            engine.check(lib.stk_posterior_predict(model._h, -1, Q.ctypes.data, S, 0, a.seed, None, st.ctypes.data,
                                                   ob.ctypes.data, None, None))
            return st.copy()

        def predictive():
            engine.check(lib.stk_log_predictive(model._h, -1, Q.ctypes.data, S, None, tot.ctypes.data))
            return tot.copy()

        with limit(a.step_limit):                      # warm-up of both
            _, first = timed(ppc)
            _, pfirst = timed(predictive)
        pp_ms, pd_ms = [], []
        for _ in range(a.repeats):
            with limit(a.step_limit):
                ms, t = timed(ppc)
                pp_ms.append(ms)
                assert np.array_equal(t, first, equal_nan=True)          # the same bits every pass
            with limit(a.step_limit):
                ms, t = timed(predictive)
                pd_ms.append(ms)
                assert np.array_equal(t, pfirst, equal_nan=True)
        pp, pd = stats(pp_ms), stats(pd_ms)
        pairs = a.shards * n * S
        chk = engine.ppc(first, ob)
        cases.append({"draws": S, "launch": engine.ppc_launch(n, a.d, S),
                      "ppc_all_shards_ms": pp, "predictive_all_shards_ms": pd,
                      "ratio_ppc_over_predictive": pp["median"] / pd["median"],
                      "ppc_ps_per_row_and_draw": pp["median"] * 1e9 / pairs,
                      "predictive_ps_per_row_and_draw": pd["median"] * 1e9 / pairs,
                      "x_read_tb_per_s": a.shards * n * a.d * 8 / (pp["median"] * 1e-3) / 1e12,
                      "p_values": {k: chk[k]["p"] for k in engine.PPC_STATS + ("chi2",)},
                      "n_non_finite": chk["n_non_finite"]})
    rec = {"tool": "tools/ppc_cost.py", "device": torch.cuda.get_device_name(0),
           "config": {"family": "logistic", "shards": a.shards, "rows_per_shard": n, "d": a.d, "repeats": a.repeats},
           "bar": "none: no earlier path computes replicates; reported against stk_log_predictive at the same S",
           "cases": cases}
    out = a.out or os.path.join(ROOT, "profiles", f"{a.run}_ppc_cost.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))
    model.close()
    ctx.close()


if __name__ == "__main__":
    main()
