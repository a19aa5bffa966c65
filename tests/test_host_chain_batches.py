"""The chain-batch plan of the regression sampler (stk_chain_batches / engine.chain_batches): a pure
host function of (chains, covariates), callable with no device."""
import numpy as np
import pytest

SIZES = (64, 16, 8, 4, 2, 1)
WIDTHS = (1, 100, 128, 129, 1023)


def _single_launch_before(C, d):
    """The (chains, d) pairs the sampler took before it batched chains: one sweep launch each."""
    if C == 64:
        return 1 <= d <= 4096
    if C == 16:
        return 1 <= d <= 128
    return C in (1, 2, 4, 8) and 1 <= d <= 1024


@pytest.mark.parametrize("d", WIDTHS)
def test_plan_covers_every_count(d):
    from stark_amd import engine
    for C in range(1, 131):
        plan = engine.chain_batches(C, d)
        assert sum(plan) == C, (C, d, plan)
        assert all(a >= b for a, b in zip(plan, plan[1:])), (C, d, plan)
        assert set(plan) <= set(SIZES), (C, d, plan)
        assert engine.chain_batches(C, d) == plan
        if _single_launch_before(C, d):
            assert plan == [C], (C, d, plan)


def test_plan_examples_at_d_100():
    from stark_amd import engine
    want = {3: [2, 1], 17: [16, 1], 32: [16, 16], 63: [16, 16, 16, 8, 4, 2, 1], 70: [64, 4, 2], 130: [64, 64, 2]}
    for C, plan in want.items():
        assert engine.chain_batches(C, 100) == plan


def test_plan_refuses_no_chains():
    import ctypes
    from stark_amd import _lib, engine
    lib = _lib.load()
    sizes = np.zeros(8, np.int32)
    for C in (0, -1, -64):
        assert lib.stk_chain_batches(C, 100, sizes.ctypes.data, 8) == -1          # STK_E_ARG
        with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
            engine.chain_batches(C, 100)
    # the count alone: no output array
    assert lib.stk_chain_batches(63, 100, ctypes.c_void_p(), 0) == 7
    # a short array takes the first sizes, the count is still returned
    assert lib.stk_chain_batches(63, 100, sizes.ctypes.data, 2) == 7 and list(sizes[:3]) == [16, 16, 0]
