"""The categorical (softmax regression) family's log density and gradient in np.longdouble, straight from the formulas
of include/stark_hip.h (STK_CATEGORICAL): the reference of tests/test_gpu_categorical.py and
tests/test_host_categorical.py.  The oracle has no softmax.

K = ncat classes, G = K - 1, q = [alpha_1 .. alpha_G, beta_1[0 .. d), ..., beta_G[0 .. d)], y in 1 .. K, class K the
reference.  With eta_ig = alpha_g + x_i . beta_g, eta_iK = 0, m_i = max_g eta_ig over all K and s_i = sum_g e^{eta_ig - m_i},
  lp              = sum_i (eta_{i, y_i} - m_i - log s_i)  - (pa |alpha|^2 + pb |beta|^2) / 2
  d lp / d eta_ig = 1[y_i = g] - e^{eta_ig - m_i} / s_i
np.exp, np.log and plain sums on longdouble: no table, no clamp, no running product.
"""
import numpy as np

L = np.longdouble


def split_q(q, ncat, d):
    """alpha (C, G) and beta (C, G, d) of the rows of q."""
    q = np.asarray(q)
    G = ncat - 1
    return q[:, :G], q[:, G:].reshape(q.shape[0], G, d)


def eta(X, q, ncat):
    """eta (n, C, K) in longdouble, the reference class's zeros included."""
    Xl = np.asarray(X).astype(L)
    a, b = split_q(np.asarray(q).astype(L), ncat, Xl.shape[1])
    with np.errstate(over="ignore", invalid="ignore"):
        e = a[None, :, :] + np.einsum("nd,cgd->ncg", Xl, b)
    return np.concatenate([e, np.zeros(e.shape[:2] + (1,), L)], axis=2)


def ref_lpgrad(X, y, q, ncat, prior=(0.0, 0.0)):
    """lp (C,) and gradient (C, G (d + 1)) at the rows of q, in np.longdouble."""
    Xl, ql = np.asarray(X).astype(L), np.asarray(q).astype(L)
    n, d = Xl.shape
    G = ncat - 1
    y = np.asarray(y).astype(np.int64)
    assert y.shape == (n,) and y.min() >= 1 and y.max() <= ncat
    pa, pb = (L(0) if s in (0.0, None) else 1 / (L(s) * L(s)) for s in prior)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = eta(X, q, ncat)                                   # (n, C, K)
        m = e.max(axis=2, keepdims=True)
        p = np.exp(e - m)
        s = p.sum(axis=2, keepdims=True)
        ey = np.take_along_axis(e, (y - 1)[:, None, None].repeat(e.shape[1], 1), axis=2)
        lp = (ey - m - np.log(s))[:, :, 0].sum(0)
        ind = (np.arange(1, ncat + 1)[None, :] == y[:, None]).astype(L)          # (n, K)
        de = (ind[:, None, :] - p / s)[:, :, :G]              # (n, C, G)
        ga = de.sum(0)                                        # (C, G)
        gb = np.einsum("ncg,nd->cgd", de, Xl)                 # (C, G, d)
        a, b = split_q(ql, ncat, d)
        lp = lp - (pa * (a ** 2).sum(1) + pb * (b ** 2).sum((1, 2))) / 2
        g = np.concatenate([ga - pa * a, (gb - pb * b).reshape(ql.shape[0], G * d)], axis=1)
    return lp, g


def swap_classes(q, y, ncat, d, g1, g2):
    """The same model with the non-reference classes g1 and g2 (1-based) relabelled: y and the (alpha, beta) blocks."""
    q = np.array(q, copy=True)
    G = ncat - 1
    a, b = q[:, :G].copy(), q[:, G:].reshape(q.shape[0], G, d).copy()
    a[:, [g1 - 1, g2 - 1]] = a[:, [g2 - 1, g1 - 1]]
    b[:, [g1 - 1, g2 - 1]] = b[:, [g2 - 1, g1 - 1]]
    y2 = np.array(y, copy=True)
    y2[np.asarray(y) == g1] = g2
    y2[np.asarray(y) == g2] = g1
    return np.concatenate([a, b.reshape(q.shape[0], G * d)], axis=1), y2
