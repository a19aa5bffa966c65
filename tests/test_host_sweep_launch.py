"""Which sweep kernel runs at (rows, covariates, chains), and with what launch shape: the planner's
decision (stk_sweep_plan, seen through stk_sweep_launch_info / engine.sweep_launch), held to the
table recorded before the planner existed, and to what the GPU tests say about their own shapes.
Host only: no device."""
import json
import os

import pytest

import test_gpu_sweep_widths as SW
from conftest import GOLDEN
from test_gpu_sweep16w import WIDTHS, _shape
from test_gpu_sweep_shards import ROWS, SHAPES

V1, V2, V3, S16, GEMM64, S16W = 1, 2, 3, 4, 5, 6
KEYS = ("kind", "T", "LD", "G", "lds_bytes", "ws_bytes_per_shard")


def _table():
    with open(os.path.join(GOLDEN, "sweep_launch.json")) as f:
        return json.load(f)["rows"]


def test_every_golden_row():
    """All 630 grid points of tools/sweep_launch_dump.hip: the recorded launch, or a refusal."""
    from stark_amd import engine
    rows = _table()
    assert len(rows) == 630
    kinds = [0] * 7
    for n, d, C, kind, *rest in rows:
        kinds[kind] += 1
        if kind == 0:
            assert rest == []
            with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
                engine.sweep_launch(n, d, C)
        else:
            assert engine.sweep_launch(n, d, C) == dict(zip(KEYS, [kind] + rest)), (n, d, C)
    assert kinds == [20, 196, 128, 96, 70, 96, 24]


def test_refuses_what_is_no_batch():
    from stark_amd import engine
    for n, d, C in ((0, 100, 4), (100, 0, 4), (100, 100, 3), (100, 100, 32), (100, 1025, 8), (100, 1025, 16)):
        with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
            engine.sweep_launch(n, d, C)


# What the comments on SHAPES in test_gpu_sweep_shards.py say each (d, C) reaches, at every n of
# ROWS: (kind, T) and, for k_sweep3, the ring depth that selects its instance (d = 100 with 3 slots:
# k_sweep3<.., 50, 3>; d = 50 with 5: k_sweep3<.., 25, 5>; anything else: the generic one).
EXPECT = {
    (4, 8): (V2, 64), (5, 8): (V1, 64), (100, 8): (V2, 64), (128, 8): (V2, 64),
    (129, 8): (V1, 32), (300, 8): (V1, 16), (700, 8): (V1, 8), (1024, 8): (V1, 8),
    (20, 4): (V3, 64, 5), (50, 4): (V3, 64, 5), (100, 4): (V3, 64, 3), (120, 4): (V2, 64), (33, 4): (V1, 64),
    (100, 1): (V3, 64, 3), (100, 2): (V3, 64, 3),
    (4, 16): (S16, 64), (33, 16): (S16, 64), (100, 16): (S16, 64), (113, 16): (S16, 64), (128, 16): (S16, 64),
    (5, 64): (GEMM64, 64), (17, 64): (GEMM64, 64), (100, 64): (GEMM64, 64), (300, 64): (GEMM64, 64),
}


def test_grouped_sweep_shapes_reach_their_kernels():
    from stark_amd import engine
    assert set(SHAPES) == set(EXPECT)
    for (d, C), want in EXPECT.items():
        for n in ROWS:
            got = engine.sweep_launch(n, d, C)
            assert (got["kind"], got["T"]) == want[:2], (n, d, C, got)
            if got["kind"] == V3:
                assert got["LD"] == want[2], (n, d, C, got)
    reached = {(k, t) for k, t, *_ in EXPECT.values()}
    assert {k for k, _ in reached} == {V1, V2, V3, S16, GEMM64}
    assert {t for k, t in reached if k == V1} == {64, 32, 16, 8}
    assert EXPECT[(100, 4)][2] == 3 and EXPECT[(50, 4)][2] == 5


def test_grouped_sweep_chunks_are_what_the_comment_says():
    """G = 3, 1, 3, 1, 2 over the five groups for v1 at T = 64, v2, v3 and k_sweep16; 6, 1, 6, 1, 3
    for the 64-chain passes: groups whose own G is below the partial-sum stride."""
    from stark_amd import engine
    groups = [ROWS[0], ROWS[2], ROWS[3], ROWS[4], ROWS[5]]
    for (d, C), want in EXPECT.items():
        G = [engine.sweep_launch(n, d, C)["G"] for n in groups]
        if want[0] == GEMM64:
            assert G == [6, 1, 6, 1, 3], (d, C, G)
        elif want[:2] != (V1, 32) and want[:2] != (V1, 16) and want[:2] != (V1, 8):
            assert G == [3, 1, 3, 1, 2], (d, C, G)
        else:
            assert G[0] > 3 and min(G) < max(G), (d, C, G)


# ---------------------------------------------------------------- test_gpu_sweep_widths.py
def _launch_class(d, C):
    """What picks a sweep's code at (d, C) on the long shard of test_gpu_sweep_widths.py: the kernel, C,
    rows per tile, the parity of d (16-B or 8-B rows) and the LD handed to the kernel (v1, v2: the LDS row
    stride; v3: the ring depth; k_sweep16w: waves per block); v3's DMA count per sub-tile; k_sweep16's
    KF and d mod 4; the 64-chain passes' column tile, k_gemm_bwd<256>'s column blocks and whether pass F
    has 8 or more 16-column steps."""
    from stark_amd import engine
    p = engine.sweep_launch(SW.ROWS[0], d, C)
    cls = (p["kind"], C, p["T"], d % 2, p["LD"])
    if p["kind"] == V3:
        cls += (-(-d // 16),)
    elif p["kind"] == S16:
        cls += ((d + 3) // 4, d % 4)
    elif p["kind"] == GEMM64:
        cls += (64 if d <= 64 else (128 if d <= 128 else 256), -(-d // 256), -(-d // 16) >= 8)
    return cls


def test_sweep_widths_hold_both_ends_of_every_launch_class():
    """d = 1 .. 1024 x every batch size: the first and the last d of every class are cases of
    test_gpu_sweep_widths.py; k_sweep3 shows every ring depth and every DMA count there; and no refusal
    hides a width (every batch size is one launch at every d)."""
    first, last = {}, {}
    for C in SW.PLAN:
        for d in range(1, 1025):
            cls = _launch_class(d, C)
            first.setdefault(cls, d)
            last[cls] = d
    assert len(set(SW.WIDTHS)) == len(SW.WIDTHS) and SW.WIDTHS[:128] == list(range(1, 129))
    missing = sorted({d for cls in first for d in (first[cls], last[cls])} - set(SW.WIDTHS))
    assert not missing, missing
    assert {cls[0] for cls in first} == {V1, V2, V3, S16, GEMM64, S16W}
    v3 = [cls for cls in first if cls[0] == V3]
    assert {cls[1] for cls in v3} == {1, 2, 4}
    for C in (1, 2, 4):
        assert {cls[4] for cls in v3 if cls[1] == C} == {3, 4, 5}                  # ring depths
        assert {cls[5] for cls in v3 if cls[1] == C} == set(range(1, 8))           # DMAs of X per sub-tile
    assert {cls[5] for cls in first if cls[0] == S16} == set(range(1, 33))         # every KF
    assert {cls[2] for cls in first if cls[0] == V1} == {64, 32, 16, 8}


def test_sweep_widths_rows_are_what_the_planner_makes_of_them():
    """Why 1483 and 77 rows (the docstring of test_gpu_sweep_widths.py), at every width of the file."""
    from stark_amd import engine
    n, short = SW.ROWS
    assert -(-n // 64) == 24 and n % 64 == 11                      # 24 tiles of 64 rows, 11 rows in the last
    for d in SW.WIDTHS:
        assert engine.chain_batches(SW.POINTS, d) == SW.PLAN
        for C in SW.PLAN:
            p, ps = engine.sweep_launch(n, d, C), engine.sweep_launch(short, d, C)
            assert ps["kind"] == p["kind"] and ps["G"] < p["G"], (d, C, p, ps)     # grouped; Gs above the short shard's G
            if p["kind"] in (V2, V3, S16) or (p["kind"] == V1 and p["T"] == 64):
                assert p["G"] == 3, (d, C, p)                      # 3 chunks of 8 tiles: 32 sub-tiles of 16 rows, 8 per
                if p["kind"] == V3:                                # wave of k_sweep16
                    assert 3 <= p["LD"] <= 5, (d, C, p)            # a chunk's 8 tiles wrap every ring depth
            elif p["kind"] == GEMM64:
                assert p["G"] == 6, (d, C, p)
            elif p["kind"] == V1:
                assert p["G"] == -(-n // (8 * p["T"])) > 3, (d, C, p)
            else:
                assert p["kind"] == S16W and p["G"] == 2, (d, C, p)


def test_wide_sixteen_widths_reach_k_sweep16w():
    from stark_amd import engine
    for d in WIDTHS:
        for n in ROWS:
            got = engine.sweep_launch(n, d, 16)
            assert (got["kind"], got["T"], got["LD"]) == (S16W, 64, _shape(d)[0]), (n, d, got)
