"""Host-side pieces of the Laplace-weighted consensus: the safeguarded Newton driver (engine.laplace)
on mock models, the argument checks of engine.consensus(weights=...) and the Hessian sweep's launch
shape (stk_hessian_launch_info).  No GPU."""
import numpy as np
import pytest


class Quad:
    """Two "shards" of an exactly quadratic log density, half the precision each (the Quad pattern of
    tests/test_host.py with a hessian method)."""

    def __init__(self, mu, prec):
        self.mu, self.part = mu, prec / 2.0
        self.hessians = 0

    def log_density_grad(self, s, Q):
        r = np.atleast_2d(Q) - self.mu
        return -0.5 * np.einsum("ij,jk,ik->i", r, self.part, r), -(r @ self.part)

    def hessian(self, s, q):
        self.hessians += 1
        lp, g = self.log_density_grad(s, q)
        return lp[0], g[0], -self.part


class LinearMock:
    """Stan's linear regression density in numpy, (alpha, beta, u = log sigma), flat priors: -H is
    indefinite at q = 0 when the residuals are large against sigma = 1."""

    def __init__(self, X, y):
        self.Xt = np.concatenate([np.ones((len(y), 1)), X], axis=1)
        self.y = y
        self.nshards, self.D = 1, [self.Xt.shape[1] + 1]

    def _parts(self, q):
        r = self.y - self.Xt @ q[:-1]
        return r, np.exp(-2.0 * q[-1])

    def log_density_grad(self, s, Q):
        lp, g = [], []
        for q in np.atleast_2d(Q):
            r, e = self._parts(q)
            lp.append(-(len(r) - 1) * q[-1] - 0.5 * e * (r @ r))
            g.append(np.concatenate([e * (self.Xt.T @ r), [-(len(r) - 1) + e * (r @ r)]]))
        return np.array(lp), np.array(g)

    def hessian(self, s, q):
        r, e = self._parts(q)
        D = q.size
        H = np.empty((D, D))
        H[:-1, :-1] = -e * (self.Xt.T @ self.Xt)
        H[:-1, -1] = H[-1, :-1] = -2.0 * e * (self.Xt.T @ r)
        H[-1, -1] = -2.0 * e * (r @ r)
        lp, g = self.log_density_grad(s, q)
        return lp[0], g[0], H


def test_newton_on_a_quadratic_density_takes_one_step():
    from stark_amd import engine
    rng = np.random.default_rng(8)
    D = 7
    A = rng.normal(size=(D, D))
    prec = A @ A.T + D * np.eye(D)
    mu = rng.normal(size=D)
    model = Quad(mu, prec)
    mode, cov, info = engine.laplace(model, [0, 1], q0=mu + 0.3)
    np.testing.assert_allclose(mode, mu, rtol=0, atol=1e-12)
    np.testing.assert_allclose(cov, np.linalg.inv(prec), rtol=1e-12, atol=1e-14)
    assert info["kinds"] == ["newton", "newton"] and info["halvings"] == [0, 0]
    assert info["steps_in_sd"][0] > 0.1 and info["steps_in_sd"][1] < 1e-10      # one step, then the check
    assert info["hessians"] == 2 and model.hessians == 4


def test_reduce_sums_the_ranks_parts():
    """Two "ranks" of one shard each, emulated by a reduce that doubles: the mode of twice the density
    is the same, the covariance halves."""
    from stark_amd import engine
    rng = np.random.default_rng(9)
    D = 4
    A = rng.normal(size=(D, D))
    prec = A @ A.T + D * np.eye(D)
    mu = rng.normal(size=D)

    def reduce(v):
        v *= 2.0

    mode, cov, _ = engine.laplace(Quad(mu, prec), [0], q0=np.zeros(D), reduce=reduce)
    np.testing.assert_allclose(mode, mu, rtol=0, atol=1e-12)
    np.testing.assert_allclose(cov, np.linalg.inv(prec), rtol=1e-12, atol=1e-14)   # 2 x half the precision


def test_indefinite_start_takes_the_block_step():
    from stark_amd import engine
    rng = np.random.default_rng(10)
    n, d = 200, 5
    X = rng.normal(size=(n, d))
    y = 3.0 + X @ rng.normal(size=d) * 2.0 + 0.5 * rng.normal(size=n)
    model = LinearMock(X, y)
    _, _, H0 = model.hessian(0, np.zeros(d + 2))
    assert np.linalg.eigvalsh(-H0).min() < 0                     # plain Newton has no descent direction here
    mode, cov, info = engine.laplace(model)                      # every shard, q0 = 0
    assert info["kinds"][0] == "block" and info["kinds"][-1] == "newton"
    ols, *_ = np.linalg.lstsq(model.Xt, y, rcond=None)
    np.testing.assert_allclose(mode[:-1], ols, rtol=1e-9, atol=1e-12)
    r = y - model.Xt @ ols
    np.testing.assert_allclose(np.exp(2 * mode[-1]), r @ r / (n - 1), rtol=1e-10)
    _, _, H = model.hessian(0, mode)
    np.testing.assert_allclose(cov, np.linalg.inv(-H), rtol=1e-6, atol=1e-12)


def test_non_finite_hessian_and_no_convergence_raise():
    from stark_amd import engine

    class Bad(Quad):
        def hessian(self, s, q):
            lp, g, H = super().hessian(s, q)
            H = H.copy()
            H[0, 0] = np.nan
            return lp, g, H

    with pytest.raises(ValueError, match="shard 1"):
        engine.laplace(Bad(np.zeros(3), np.eye(3)), [1], q0=np.ones(3))
    model = LinearMock(np.random.default_rng(1).normal(size=(50, 2)), np.arange(50.0))
    with pytest.raises(ValueError, match="no convergence"):
        engine.laplace(model, max_iter=1)


def test_consensus_weights_argument_checks():
    """Refused before a context (a device) is needed."""
    from stark_amd import engine
    draws = [np.random.default_rng(s).normal(size=(4, 30)) for s in range(3)]
    with pytest.raises(ValueError, match="3 shards"):
        engine.consensus(draws, weights=[np.eye(3)] * 2)
    with pytest.raises(ValueError, match=r"weights\[1\]"):
        engine.consensus(draws, weights=[np.eye(3), np.eye(4), np.eye(3)])
    with pytest.raises(ValueError, match=r"weights\[0\]"):
        engine.consensus(draws, weights=[np.ones(3)] * 3)


def _expected_launch(n, d):
    nt = (d + 2 + 15) // 16                                      # column tiles: x, the ones column, linear's r
    ld = 16 * nt if nt % 2 else 16 * nt + 16
    G = min(256, max(1, -(-(-(-n // 16)) // 32)))
    return {"T": 16, "G": G, "waves": 4, "lds_bytes": 8 * (4 * 16 * ld + ld + 32),
            "ws_bytes_per_shard": 8 * 256 * (nt * (nt + 1) // 2) * G}


@pytest.mark.parametrize("n,d,G,lds,ws", [(1, 1, 1, 8576, 2048), (65, 128, 1, 75136, 92160),
                                          (12_500_000, 100, 256, 58496, 14_680_064), (1027, 17, 3, 25216, 18432)])
def test_hessian_launch_info(n, d, G, lds, ws):
    from stark_amd import engine
    got = engine.hessian_launch(n, d)
    assert got == _expected_launch(n, d)
    assert (got["G"], got["lds_bytes"], got["ws_bytes_per_shard"]) == (G, lds, ws)
    assert got["lds_bytes"] <= 80 * 1024                         # two blocks per CU


def test_hessian_launch_info_refuses_wide_shards():
    from stark_amd import engine
    from stark_amd._lib import StarkHipError
    with pytest.raises(StarkHipError, match="128") as e:
        engine.hessian_launch(1000, 129)
    assert e.value.code == -1
    with pytest.raises(StarkHipError):
        engine.hessian_launch(0, 10)
