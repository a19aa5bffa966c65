#!/usr/bin/env python3
"""What the data fingerprint costs, against the yardstick VERDICT.md sets: the fingerprint of ALL
shards of the headline model takes at most one sweep step of its 16-chain sampler.

Workload: BASELINE configs[3]'s model, 8 synthetic logistic shards x 1.25e7 rows x d = 100, on one
GPU.  In one process, alternating:
  fingerprint  stk_fingerprint_words over the x and y arrays of every shard where the model keeps
               them (Model.device_arrays: the calls stk_model_fingerprint makes, without its
               cache), a HIP event pair around every call, summed over the model;
  sweep step   sweep_ms / sweeps of a 16-chain sampler on the same model with the context's
               profiling on (HIP events around the sweeps of every step).
After a warm-up of both, `--repeats` rounds (>= 20); medians and the spread are reported.  The first,
uncached Model.fingerprint() of the model is timed too (wall clock, with its host round trips).

Writes profiles/<run>_fingerprint_cost.json and prints the same JSON line.
usage: tools/fingerprint_cost.py --run r07a [--rows 1e8 --d 100 --shards 8 --repeats 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_TBS = 8.0      # MI355X HBM3E


def stats(v):
    v = np.asarray(v, float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "n": int(v.size)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--run", default="r07a", help="prefix of the profile file")
    p.add_argument("--rows", type=float, default=1e8, help="total rows over all shards")
    p.add_argument("--d", type=int, default=100)
    p.add_argument("--shards", type=int, default=8)
    p.add_argument("--chains", type=int, default=16)
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--steps", type=int, default=4, help="sampler steps per round")
    p.add_argument("--seed", type=int, default=20240)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.repeats < 20:
        sys.exit("--repeats must be at least 20")

    import ctypes
    import torch
    from stark_amd import _lib, engine, fulldata

    words_fn = _lib.load().stk_fingerprint_words

    torch.cuda.set_device(0)
    ctx = fulldata.context_on_torch_stream(0)      # torch events bracket the library's kernels
    n = int(a.rows) // a.shards
    model = engine.Model.synthetic(ctx, "logistic", a.shards, n, a.d, data_seed=a.seed)
    ctx.sync()
    arrays = [model.device_arrays(s) for s in range(a.shards)]
    nbytes = a.shards * n * (8 * a.d + 4)

    def fingerprint_pass():
        """words() of every array of every shard; the summed event time in ms and the sums."""
        pairs, sums = [], []
        for arr in arrays:
            for key, tag, wb in (("x", 1, 8), ("y", 3, 4)):
                ptr, cnt = arr[key]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                out = ctypes.c_uint64()
                args = (ctx._h, ctypes.c_void_p(ptr), cnt, wb, tag, 0, ctypes.byref(out))
                e0.record()                   # the C call alone lies between the events
                rc = words_fn(*args)
                e1.record()
                engine.check(rc)
                sums.append(out.value)
                pairs.append((e0, e1))
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in pairs), sums

    sampler = model.sampler(num_warmup=150, num_samples=100000, chains=a.chains, seed=a.seed + 1,
                            stepsize_jitter=0.5, nuts_criterion="stan2.23")

    def sweep_pass():
        """ms per sweep step over a.steps steps (None when no step of the batch swept)."""
        ctx.set_profiling(1)
        i0 = sampler.info()
        sampler.run(max_steps=a.steps)
        i1 = sampler.info()
        ctx.set_profiling(0)
        k = i1["sweeps"] - i0["sweeps"]
        if not k:
            return None
        return (i1["sweep_ms"] - i0["sweep_ms"]) / k, (i1["shard_sweeps"] - i0["shard_sweeps"]) / k

    # warm-up of both (code objects, clocks, the sampler past its first steps)
    sampler.run(max_steps=10)
    _, sums0 = fingerprint_pass()
    sweep_pass()
    fp_ms, sw_ms, sw_shards = [], [], []
    for _ in range(a.repeats):
        ms, sums = fingerprint_pass()
        assert sums == sums0, "the fingerprint changed between repeats"
        fp_ms.append(ms)
        v = sweep_pass()
        if v is not None:
            sw_ms.append(v[0])
            sw_shards.append(v[1])
    # the public path, uncached then cached
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    fps = model.fingerprint()
    e1.record()
    first_ms = 1e3 * (time.perf_counter() - t)
    torch.cuda.synchronize()
    first_event_ms = e0.elapsed_time(e1)
    t = time.perf_counter()
    model.fingerprint()
    cached_ms = 1e3 * (time.perf_counter() - t)

    f, s = stats(fp_ms), stats(sw_ms)
    tbs = nbytes / (f["median"] * 1e-3) / 1e12
    ratio = f["median"] / s["median"]
    rec = {"tool": "tools/fingerprint_cost.py", "device": torch.cuda.get_device_name(0),
           "config": {"family": "logistic", "shards": a.shards, "rows_per_shard": n, "d": a.d, "chains": a.chains,
                      "repeats": a.repeats, "steps_per_round": a.steps},
           "algorithmic_bytes": nbytes,
           "fingerprint_all_shards_ms": f, "sweep_step_ms": s,
           "ratio_fingerprint_over_sweep_step": ratio,
           "bar": "fingerprint of all shards <= one sweep step (ratio <= 1)", "bar_met": bool(ratio <= 1.0),
           "fingerprint_tb_per_s": tbs, "fingerprint_share_of_hbm_peak": tbs / HBM_PEAK_TBS,
           "sweep_step_tb_per_s": nbytes / (s["median"] * 1e-3) / 1e12,
           "shard_passes_per_sweep_step": float(np.mean(sw_shards)),
           "model_fingerprint_first_call_event_ms": first_event_ms,
           "model_fingerprint_first_call_wall_ms": first_ms, "model_fingerprint_cached_call_wall_ms": cached_ms,
           "fingerprints": [f"{int(v):016x}" for v in fps]}
    out = a.out or os.path.join(ROOT, "profiles", f"{a.run}_fingerprint_cost.json")
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
