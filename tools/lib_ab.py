#!/usr/bin/env python3
"""A/B of whole library builds on the bench's own workloads: each arm is libstark_hip.so built
from the working tree (or a git revision) with extra compiler flags on chosen source files;
the arms run alternately in fresh processes (STARK_HIP_LIB) so box drift hits every arm, and
each workload reports whether the arms' results are bit-identical.

  workloads  schools   tools/bench_schools.py (configs[1]: 4096 chains, 1000 + 1000): grads/s,
                       identical = posterior means, min ESS, divergences, leapfrogs agree
             sweep16   bench.py --throughput-only (configs[3]: 8 x 1.25e7 rows, d = 100, 16
                       chains): k_sweep16's ms per launch (HIP events), identical = grads agree
             sweep16lin  the same at configs[2]'s shape (linear, 8 x 1.25e6 rows, d = 50)
             fulldata  tools/bench_fulldata.py --steps 6 (configs[4] at 1e7 rows): pass F + B ms

usage: tools/lib_ab.py build NAME [--rev REV] [--flags FILE=FLAGS ...]   (here; -> tools/_bin/ab_NAME, by the
       tree's or the revision's Makefile, FLAGS in place of its own for FILE)
       tools/lib_ab.py run --arms A,B[,C] --work schools|sweep16|fulldata [--rounds R]   (GPU box)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "_bin")


def build(name, rev=None, flags=()):
    out = os.path.join(BIN, f"ab_{name}")
    os.makedirs(out, exist_ok=True)
    csrc = os.path.join(ROOT, "stark_amd", "csrc")
    if rev:
        src = os.path.join(BIN, f"ab_{name}_src")
        subprocess.run(["rm", "-rf", src], check=True)
        os.makedirs(src)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "stark_amd/csrc", "include"], check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", src], input=tar, check=True)
        csrc = os.path.join(src, "stark_amd", "csrc")
    # the one build recipe is the Makefile's: FILE=FLAGS becomes its per-file FLAGS_FILE, for every object built
    # from FILE; where the compiler fails with them make falls back to the default flags and says so, which an
    # arm that asked for flags must not do
    extra = dict(f.split("=", 1) for f in flags)
    p = subprocess.run(["make", "-s", "-j8", "-C", csrc, f"OUT={out}", *[f"FLAGS_{k}={v}" for k, v in extra.items()]],
                       stdout=subprocess.PIPE, text=True)
    if p.returncode or (extra and "failed, default flags" in p.stdout):
        sys.exit("build failed:\n" + "\n".join(ln for ln in p.stdout.splitlines() if "failed" in ln))
    json.dump({"rev": rev or "working tree", "flags": extra or "Makefile"}, open(os.path.join(out, "arm.json"), "w"))
    print("built", os.path.join(out, "libstark_hip.so"), extra or "with the Makefile")


def one(arm, work):
    env = dict(os.environ, STARK_HIP_LIB=os.path.join(BIN, f"ab_{arm}", "libstark_hip.so"))
    if work == "schools":
        cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_schools.py")]
    elif work == "sweep16":
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--throughput-only", "--steps", "200", "--warmup", "10"]
    elif work == "sweep16lin":
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--throughput-only", "--family", "linear", "--rows", "1e7",
               "--d", "50", "--steps", "2000", "--warmup", "50"]
    else:
        cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_fulldata.py"), "--rows-per-gpu", "1e7", "--steps", "6",
               "--warmup", "2"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
    if p.returncode != 0:
        sys.exit(p.stderr[-2000:])
    ln = json.loads(p.stdout.strip().splitlines()[-1])
    if work == "schools":
        return ln["value"] / 1e6, ln["value"], [ln[k] for k in ("posterior_mean_mu_tau", "min_ess", "divergent", "leapfrogs_per_transition")]
    if work in ("sweep16", "sweep16lin"):
        return ln["roofline"]["avg_launch_ms"], ln["value"], [round(ln["value"] * ln["ms_per_step"])]
    return ln["roofline"]["avg_launch_ms"], ln["value"], [ln.get("chains_sha16_per_rank")]


def run(arms, work, rounds):
    res = {a: [] for a in arms}
    rate = {a: [] for a in arms}    # the workload's own headline figure (grads/s)
    ident = {}
    for r in range(rounds):
        for a in (arms if r % 2 == 0 else arms[::-1]):
            v, rt, key = one(a, work)
            res[a].append(v)
            rate[a].append(rt)
            ident.setdefault(a, key)
            print(f"[lib_ab] {work} round {r} {a}: {v:.4f}", file=sys.stderr, flush=True)
    med = {a: sorted(v)[len(v) // 2] for a, v in res.items()}
    out = {"work": work, "unit": "M grads/s" if work == "schools" else "ms per launch",
           "arms": {a: {"values": res[a], "median": med[a], "rate": rate[a],
                        "build": json.load(open(os.path.join(BIN, f"ab_{a}", "arm.json")))} for a in arms},
           "ratio_vs_first": {a: med[a] / med[arms[0]] for a in arms},
           "identical_to_first": {a: ident[a] == ident[arms[0]] for a in arms}}
    print(json.dumps(out))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("cmd", choices=["build", "run"])
    p.add_argument("name", nargs="?")
    p.add_argument("--rev", default=None)
    p.add_argument("--flags", nargs="*", default=[])
    p.add_argument("--arms", default="")
    p.add_argument("--work", default="schools", choices=["schools", "sweep16", "sweep16lin", "fulldata"])
    p.add_argument("--rounds", type=int, default=3)
    a = p.parse_args()
    if a.cmd == "build":
        build(a.name, a.rev, a.flags)
    else:
        run(a.arms.split(","), a.work, a.rounds)


if __name__ == "__main__":
    main()
