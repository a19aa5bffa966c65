#!/usr/bin/env python3
"""What the semiparametric density-product combiner costs at the headline combine shape, next to the
weighted-average combine of the same draws.

Workload: synthetic Gaussian draws, 8 shards x P = 102 rows (101 parameters + lp__) x S = 16,000 draws on the
device, T = 16,000 output draws, the defaults K = min(T, 1024) chains, burn 200, thin 5 and the annealed
bandwidth.  No shard data is needed.  In one process, alternating:
  prepare     engine.dpe_prepare   the combine's moment stages, the host factorisation, the whitening and
                                   Mahalanobis GEMMs (its output tensors are allocated inside the window)
  sample      engine.dpe_sample    k_dpe_img (one wavefront per chain) and the map back to theta
  consensus   engine.consensus(separate_lp=True)   stk_consensus_blocked on the same device draws
Each is timed with a HIP event pair on the context's stream after a warm-up of all three; medians and the
spread over `--repeats` rounds are reported.  There is no bar: no earlier path computes these draws.  The
record also holds what the chains' time says about the kernel: microseconds per proposal of one chain (every
proposal is a dependent round trip to the image) and the bytes per second the gathers add up to.

Writes profiles/<run>_dpe_cost.json and prints the same JSON line.
usage: tools/dpe_cost.py --run r21a [--shards 8 --rows 102 --draws 16000 --repeats 5]"""
import argparse
import contextlib
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TB_S = 8.0          # MI355X HBM3E spec


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
    p.add_argument("--run", default="r21a", help="prefix of the profile file")
    p.add_argument("--shards", type=int, default=8)
    p.add_argument("--rows", type=int, default=102, help="P: parameter rows + lp__")
    p.add_argument("--draws", type=int, default=16000, help="S per shard; T = S")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--seed", type=int, default=20240)
    p.add_argument("--step-limit", type=int, default=120, help="seconds every GPU step may take")
    p.add_argument("--out", default=None)
    a = p.parse_args()

    import torch
    from stark_amd import engine, fulldata

    torch.cuda.set_device(0)
    ns, P, S = a.shards, a.rows, a.draws
    pp = P - 1
    with limit(a.step_limit):
        ctx = fulldata.context_on_torch_stream(0)      # torch events bracket the library's kernels
        g = torch.Generator(device="cuda:0").manual_seed(a.seed)
        X = torch.randn((ns, P, S), dtype=torch.float64, device="cuda:0", generator=g)
        X[:, :pp] = X[:, :pp] * torch.linspace(0.5, 2.0, pp, dtype=torch.float64, device="cuda:0")[None, :, None]
        X[:, :pp] += 0.05 * torch.randn((ns, pp, 1), dtype=torch.float64, device="cuda:0", generator=g)
        X[:, pp] -= 500.0
        torch.cuda.synchronize()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    state = {}

    def prepare():
        state["prep"] = engine.dpe_prepare(X, ctx=ctx)
        return state["prep"]["Y"]

    passes = {"prepare": prepare,
              "sample": lambda: engine.dpe_sample(state["prep"], seed=a.seed, ctx=ctx),
              "consensus": lambda: engine.consensus(X, ctx=ctx, separate_lp=True)[0]}
    with limit(a.step_limit):                          # warm-up of all three
        first = {k: timed(f)[1] for k, f in passes.items()}
    ms = {k: [] for k in passes}
    info = first["sample"][1]
    for _ in range(a.repeats):
        for k, f in passes.items():
            with limit(a.step_limit):
                t, out = timed(f)
                ms[k].append(t)
                got, ref = (out[0], first[k][0]) if k == "sample" else (out, first[k])
                assert torch.equal(got, ref), k         # the same bits every pass

    T, K, sweeps = S, info["chains"], info["sweeps"]
    launch = engine.dpe_launch(ns, P, S, T, K)
    pr, sa, co = stats(ms["prepare"]), stats(ms["sample"]), stats(ms["consensus"])
    proposals = sweeps * ns                            # of one chain, one after the other
    gathered = K * proposals * 2 * launch["ldp"] * 8   # the old and the new row of every proposal
    dpe = first["sample"][0][:pp].cpu().numpy()
    avg = first["consensus"][:pp].cpu().numpy()
    rec = {"tool": "tools/dpe_cost.py", "device": torch.cuda.get_device_name(0),
           "config": {"shards": ns, "P": P, "S": S, "T": T, "chains": K, "burn": 200, "thin": 5, "sweeps": sweeps,
                      "bandwidth": "annealed", "repeats": a.repeats},
           "launch": launch,
           "prepare_ms": pr, "sample_ms": sa, "consensus_blocked_ms": co,
           "dpe_over_consensus": (pr["median"] + sa["median"]) / co["median"],
           "bar": "none: the times are recorded, not judged",
           "accept_rate": [float(v) for v in info["accept_rate"]],
           "h_range": [info["h_min"], info["h_max"]], "h_last": info["h_last"],
           "sample_us_per_proposal_of_a_chain": sa["median"] * 1e3 / proposals,
           "sample_gather_tb_per_s": gathered / (sa["median"] * 1e-3) / 1e12,
           "sample_gather_share_of_hbm_peak": gathered / (sa["median"] * 1e-3) / 1e12 / HBM_TB_S,
           "image_mb": ns * S * launch["ldp"] * 8 / 1e6,
           "max_abs_mean_difference_from_consensus_in_sd": float(
               np.abs((dpe.mean(axis=1) - avg.mean(axis=1)) / avg.std(axis=1)).max())}

    out = a.out or os.path.join(ROOT, "profiles", f"{a.run}_dpe_cost.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))
    ctx.close()


if __name__ == "__main__":
    main()
