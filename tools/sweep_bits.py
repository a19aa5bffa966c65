#!/usr/bin/env python3
"""SHA-256 of what the regression sweeps compute on a fixed seeded list, for comparing two builds
of libstark_hip.so bit for bit (the library is the one STARK_HIP_LIB names, else the tree's):

  shards   log_density_grad_shards over SHAPES x ROWS of tests/test_gpu_sweep_shards.py, both families
  chains   log_density_grad_chains at C in {3, 7, 23, 70} x d in {20, 100, 129, 300}, both families
  single   log_density_grad of shards 1 and 2 at C in {1, 2, 3, 5, 16, 17, 64, 70} x d in {5, 100, 129}
  sample   logistic sampling runs at d = 20, chains = 7, 30 + 30 iterations: 3 shards of 1500, 1500
           and 77 rows, and 8 shards of 77 rows (tiny n: launches dominate) -- draws and stats hashed,
           wall time per sampler step reported as `host_ms_per_step` (a figure, never compared)
  draws    the sweeps over a draw image -- log_predictive(rows=True), loo(rows=True) and log_density --
           for the three regression families at d in {1, 5, 50, 100, 128} (KF = 1, 2, 13, 25, 32) x
           S in {1, 17, 100, 600} (one draw, a partial draw tile, the 4-wave LOO with a fitted tail, the
           8-wave LOO): shards of 1, 65 and 257 rows in one grouped launch, and shard 1 alone
           (shard0 > 0); at d = 5, S = 17 also with one draw whose intercept is NaN and (poisson) one
           whose eta overflows

The sweeps reduce in a fixed order, so two builds that launch the same kernels with the same
arguments give equal hashes; a differing hash is a routing or argument error.

usage: STARK_HIP_LIB=.../libstark_hip.so tools/sweep_bits.py OUT.json;  tools/sweep_bits.py --diff A.json B.json"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return h.hexdigest()


def case(family, d, rows, seed):
    """Shards of `rows` rows from one seeded generator; large-|eta| rows at the head of each."""
    rng = np.random.default_rng(seed)
    shards = []
    beta = rng.normal(0, 1 / np.sqrt(d), d)
    for n in rows:
        X = rng.uniform(-1.7, 1.7, (n, d))
        if family == "logistic":
            eta = X @ beta
            eta[: max(1, n // 50)] *= 80.0
            y = (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.int32)
        else:
            y = 0.3 + X @ beta + rng.normal(size=n)
        shards.append({"x": X, "y": y})
    return shards, beta, rng


def points(rng, family, d, beta, shape):
    q = rng.normal(0, 0.2, shape + (d + 1 if family == "logistic" else d + 2,))
    if family == "logistic":
        q[..., 0, 1:] = beta * 40
    return q


DRAW_ROWS, DRAW_D, DRAW_S = (1, 65, 257), (1, 5, 50, 100, 128), (1, 17, 100, 600)


def draws_section(engine, ctx, H):
    for family in ("logistic", "poisson", "linear"):
        for d in DRAW_D:
            rng = np.random.default_rng(7000 + 10 * d + len(family))
            beta = rng.normal(0, 1 / np.sqrt(d), d)
            shards = []
            for n in DRAW_ROWS:
                X = rng.uniform(-1.7, 1.7, (n, d))
                eta = 0.3 + X @ beta
                y = {"logistic": lambda: (rng.uniform(size=n) < 1 / (1 + np.exp(-eta))).astype(np.int32),
                     "poisson": lambda: rng.poisson(np.exp(eta)).astype(np.int32),
                     "linear": lambda: eta + 0.7 * rng.normal(size=n)}[family]()
                shards.append({"x": X, "y": y})
            truth = np.concatenate([[0.3], beta, [np.log(0.7)] if family == "linear" else []])
            m = engine.Model(ctx, family, shards)
            try:
                cases = [(f"S{S}", truth + rng.normal(0, 0.1, (S, truth.size))) for S in DRAW_S]
                if d == 5:
                    bad = cases[1][1].copy()
                    bad[3, 0] = np.nan
                    cases.append(("S17nan", bad))
                    if family == "poisson":
                        big = cases[1][1].copy()
                        big[7, 1] = 800.0
                        cases.append(("S17overflow", big))
                for tag, Q in cases:
                    for sh in (None, 1):
                        key = f"draws/{family}/d{d}/{tag}/shard{'s' if sh is None else sh}"
                        tot, rows = m.log_predictive(Q, sh, rows=True)
                        H[key + "/predictive"] = sha(tot, *rows.values())
                        tot, rows = m.loo(Q, sh, rows=True)
                        H[key + "/loo"] = sha(tot, *rows.values())
                        H[key + "/logdens"] = sha(m.log_density(Q, sh))
            finally:
                m.close()


def main(out_path):
    from stark_amd import _lib, engine
    from test_gpu_sweep_shards import ROWS, SHAPES
    ctx = engine.default_context(0)
    res = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT), "hashes": {}, "host_ms_per_step": {}}
    H = res["hashes"]
    for family in ("logistic", "linear"):
        for d in sorted({d for d, _ in SHAPES} | {20, 100, 129, 300, 5}):
            shards, beta, rng = case(family, d, ROWS, 1000 * d + (family == "linear"))
            m = engine.Model(ctx, family, shards)
            try:
                for C in sorted(C for dd, C in SHAPES if dd == d):
                    H[f"shards/{family}/d{d}/C{C}"] = sha(*m.log_density_grad_shards(points(rng, family, d, beta, (len(ROWS), C))))
                if d in (20, 100, 129, 300):
                    for C in (3, 7, 23, 70):
                        H[f"chains/{family}/d{d}/C{C}"] = sha(*m.log_density_grad_chains(points(rng, family, d, beta, (len(ROWS), C))))
                if d in (5, 100, 129):
                    for C in (1, 2, 3, 5, 16, 17, 64, 70):
                        for s in (1, 2):
                            H[f"single/{family}/d{d}/C{C}/shard{s}"] = sha(*m.log_density_grad(s, points(rng, family, d, beta, (C,))))
            finally:
                m.close()
    for tag, rows in (("3shards", [1500, 1500, 77]), ("8shards", [77] * 8)):
        shards, _, _ = case("logistic", 20, rows, 20)
        m = engine.Model(ctx, "logistic", shards)
        try:
            r = m.sample(num_warmup=30, num_samples=30, chains=7, seed=11)
            t0 = time.perf_counter()     # timed on the repeat: the kernels are loaded
            r2 = m.sample(num_warmup=30, num_samples=30, chains=7, seed=11)
            dt = time.perf_counter() - t0
        finally:
            m.close()
        H[f"sample/{tag}"] = sha(*r.draws, *r.stats)
        H[f"sample/{tag}/repeat"] = sha(*r2.draws, *r2.stats)
        res["host_ms_per_step"][tag] = {"steps": int(r.info["steps"]), "ms_per_step": 1e3 * dt / r.info["steps"]}
    draws_section(engine, ctx, H)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(H)} hashes -> {out_path}; host ms per step {res['host_ms_per_step']}")


def diff(a, b):
    A, B = (json.load(open(p))["hashes"] for p in (a, b))
    bad = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
    print(f"{len(A)} / {len(B)} hashes, {len(bad)} differ" + "".join(f"\n  {k}" for k in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(diff(*sys.argv[2:4]) if sys.argv[1] == "--diff" else main(sys.argv[1]))
