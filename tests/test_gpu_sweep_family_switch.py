"""The sweeps' dispatch on the runtime family, once per family: a chain count that is no batch size is refused
with STK_E_ARG before anything is launched, and the same model then runs a valid sweep -- one shard of n = 77
rows, d = 5, C = 2 through Model.log_density_grad_shards -- to the family's own reference at the family's own
bars (the oracle and _check_against_oracle for logistic and linear; the longdouble restatements and check_bars of
test_gpu_poisson.py, test_gpu_negbin.py and test_gpu_student.py for the other three)."""
import numpy as np
import pytest

import negbin_ref
import student_ref
import test_gpu_negbin as nb
import test_gpu_poisson as pois
import test_gpu_student as st
from test_gpu_sweep_shards import _check_against_oracle, _grouped_case

pytestmark = pytest.mark.gpu

N, D, C = 77, 5, 2
NU = 4.0


def _case(orc, family):
    """(shards, model keywords, q [1, C, D], check(lp, g)) by the family's own recipe."""
    if family in ("logistic", "linear"):
        shards, oms, q = _grouped_case(orc, family, D, C, rows=[N])
        return shards, {}, q, lambda lp, g: _check_against_oracle(oms, q, lp, g, f"switch[{family}]")
    if family == "poisson":
        rng, X, y, beta = pois.make_data(N, D)
        q = rng.normal(0, 0.2, (C, D + 1))
        q[0] = np.concatenate([[0.3], 3 * beta])
        q[1, 1:] = 12 * beta
        olp, og = pois.ref_lpgrad(X, y, q)
        check = pois.check_bars
    elif family == "neg_binomial":
        rng, X, y, beta = nb.make_data(N, D)
        q = nb.points(rng, beta, C, D)
        olp, og = negbin_ref.ref_lpgrad(X, y, q)
        check = nb.check_bars
    else:
        rng, X, y, beta = st.make_data(N, D)
        q = st.points(rng, beta, C, D)
        olp, og = student_ref.ref_lpgrad(X, y, q, NU)
        check = st.check_bars
    assert np.all(np.isfinite(olp.astype(np.float64)))
    return [{"x": X, "y": y}], ({"nu": NU} if family == "student_t" else {}), q[None], \
        lambda lp, g: check(lp[0], g[0], olp, og, family)


@pytest.mark.parametrize("family", ["logistic", "linear", "poisson", "neg_binomial", "student_t"])
def test_refused_chain_count_then_a_valid_sweep(ctx, orc, family):
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    shards, kw, q, check = _case(orc, family)
    m = engine.Model(ctx, family, shards, **kw)
    try:
        assert engine.chain_batches(3, D) == [2, 1]          # three chains are no single batch
        with pytest.raises(StarkHipError) as e:
            m.log_density_grad_shards(np.concatenate([q, q[:, :1]], axis=1))
        assert e.value.code == -1                            # STK_E_ARG
        lp, g = m.log_density_grad_shards(q)
        assert lp.shape == (1, C) and np.isfinite(lp).all() and np.isfinite(g).all()
        check(lp, g)
    finally:
        m.close()
