#!/usr/bin/env python3
"""k_nuts_step under dense_e next to diag_e, per dispatch, from a kernel trace.

  run      a short adaptive run of one geometry and metric, for `rocprofv3 --kernel-trace`:
             rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- \\
                 python3 tools/dense_step_trace.py run --d 100 --shards 8 --chains 16 --metric dense_e
           Small buffers (warmup 30: windows end after draws 14 and 21) and max_depth 3 keep the step
           count low while every chain still meets two window ends (the Welford update of every
           window draw, the regularisation and the in-place Cholesky).
  summary  per-kernel figures of one or more kernel-trace CSVs as one JSON line each: dispatches,
           median / p99 / max duration.  For k_nuts_step the median is the plain leapfrog step; the
           slowest dispatches are those in which a chain ends a window, so `max` is one chain's
           window-end time (chains sit on different CUs and do not queue behind each other).
             python3 tools/dense_step_trace.py summary DIR/*kernel_trace.csv
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(a):
    from stark_amd import engine
    ctx = engine.Context(0)
    m = engine.Model.synthetic(ctx, "logistic", a.shards, int(a.rows) // a.shards, a.d, data_seed=20240)
    s = m.sampler(num_warmup=30, num_samples=5, chains=a.chains, seed=20241, max_depth=3, adapt_init_buffer=8,
                  adapt_term_buffer=8, adapt_window=7, metric=a.metric)
    s.run()
    info = s.info()
    print(json.dumps({"metric": a.metric, "D": a.d + 1, "chains": a.shards * a.chains, "rows": int(a.rows),
                      "steps": info["steps"], "errors": info["errors"], "done": info["done"]}), flush=True)
    s.close()
    m.close()


def summary(paths):
    for path in paths:
        per = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"].split("(")[0]
                per.setdefault(name, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        for name, ns in sorted(per.items()):
            ns.sort()
            q = lambda p: ns[min(len(ns) - 1, int(p * len(ns)))] / 1e3   # noqa: E731
            print(json.dumps({"file": os.path.basename(path), "kernel": name, "dispatches": len(ns),
                              "median_us": q(0.5), "p99_us": q(0.99), "max_us": ns[-1] / 1e3,
                              "total_ms": sum(ns) / 1e6}))


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = p.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--rows", type=float, default=1e7)
    r.add_argument("--d", type=int, default=100)
    r.add_argument("--shards", type=int, default=8)
    r.add_argument("--chains", type=int, default=16)
    r.add_argument("--metric", default="dense_e", choices=["diag_e", "dense_e", "unit_e"])
    sm = sub.add_parser("summary")
    sm.add_argument("csv", nargs="+")
    a = p.parse_args()
    run(a) if a.cmd == "run" else summary(a.csv)
