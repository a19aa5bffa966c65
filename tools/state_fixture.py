#!/usr/bin/env python3
"""Record the version-2 sampler state fixtures that tests/test_gpu_state_fixture.py replays.

For each case: create the model and a sampler, run to iteration STOP (mid-warmup, so the
adaptation state is live in the blob), save the blob, then resume to the end.  Written to
tests/golden/state_v2_<case>.npz: the blob bytes, the final draws and the final sampler stats of
every shard.

Record with the library build the fixtures are to pin -- the one BEFORE a change to the host
layer -- never with the code under test:

    STARK_HIP_LIB=path/to/libstark_hip.so python tools/state_fixture.py [case ...]

A later change that deliberately alters the sampler's bits regenerates the fixtures with this
tool.  A change to the header part of the blob (StateHeader, the fingerprint table, the segment
order or sizes) is a format change and needs a new version number, not new fixtures."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STOP = 12
CFG = dict(num_warmup=20, num_samples=10, max_depth=5)
SCHOOLS_Y = [28, 8, -3, 7, -1, 1, 18, 12]          # examples/stark_ex.py
SCHOOLS_SIGMA = [15, 10, 16, 11, 9, 11, 10, 18]
# the smallest cases that reach every branch of the sampler's buffer table
CASES = {
    # the fused kernel and the tree stack
    "schools": dict(model=lambda e, ctx: e.Model(ctx, "schools", [{"y": SCHOOLS_Y, "sigma": SCHOOLS_SIGMA}]),
                    cfg=dict(chains=2)),
    # the chain batches 2 + 1 and two shards' fingerprints
    "logistic": dict(model=lambda e, ctx: e.Model.synthetic(ctx, "logistic", 2, 256, 3), cfg=dict(chains=3)),
    # the three dense_e segments
    "linear": dict(model=lambda e, ctx: e.Model.synthetic(ctx, "linear", 1, 128, 2), cfg=dict(chains=2, metric="dense_e")),
}


def fixture_path(case):
    return os.path.join(GOLDEN, f"state_v2_{case}.npz")


def sampler(engine, ctx, case):
    """The case's model and a fresh sampler on it."""
    m = CASES[case]["model"](engine, ctx)
    return m, m.sampler(**CFG, **CASES[case]["cfg"])


def final(s):
    """Draws and stats of every shard, stacked."""
    out = [s.draws(sh) for sh in range(s.model.nshards)]
    return np.stack([d for d, _ in out]), np.stack([st for _, st in out])


def main():
    sys.path.insert(0, ROOT)
    from stark_amd import _lib, engine
    ctx = engine.Context(0)
    for case in sys.argv[1:] or CASES:
        m, s = sampler(engine, ctx, case)
        blob = s.run(STOP).save_state()
        draws, stats = final(s.run())
        np.savez(fixture_path(case), blob=blob, draws=draws, stats=stats)
        print(f"{case}: blob {blob.size} bytes, file {os.path.getsize(fixture_path(case))} bytes ({_lib.LIB_PATH})")
        s.close()
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
