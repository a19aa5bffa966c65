"""numpy restatement of the semiparametric density-product combiner, in np.longdouble (no library code).

With M usable shards of S draws theta^m_s in R^p, mu_m / Sigma_m the sample mean and covariance (np.cov's),
  Sigma_M = inv(sum_m inv(Sigma_m)) = L L^T,  mu_M = Sigma_M sum_m inv(Sigma_m) mu_m,
  y^m_s = inv(L)(theta^m_s - mu_M) / sqrt(M),  n^m_s = |y^m_s|^2,
  g^m_s = (theta^m_s - mu_m)^T inv(Sigma_m) (theta^m_s - mu_m) / 2,
and for an index tuple t with s_t, N_t, G_t the sums of y, n, g at the chosen draws
  log W_t(h) = -(N_t - |s_t|^2 / M) / (2 h^2) - |s_t|^2 / (2 M (1 + h^2)) + G_t
  component:   y ~ N(s_t / (M (1 + h^2)), h^2 / (M (1 + h^2)) I),  theta = mu_M + sqrt(M) L y.
Random numbers: Philox4x32-10 (engine.philox_words, itself checked against the library elsewhere) at
  {chain, m >> 2, 0, stream << 8 | 0x23}   initial index of coordinate m: 32-bit word m & 3, index = (word * S) >> 32
  {chain, sweep, m, stream << 8 | 0x24}    proposal: index from the first output's low word, u = u53(second output)
  {chain, draw, i >> 1, stream << 8 | 0x25} Box-Muller normals of coordinates i (cos for even i, sin for odd)
"""
import itertools

import numpy as np

LD = np.longdouble
TAG_INIT, TAG_PROP, TAG_NORM = 0x23, 0x24, 0x25


# ---------------------------------------------------------------- longdouble linear algebra
def inv_ld(A):
    """Gauss-Jordan inverse of a symmetric positive definite matrix in longdouble (diagonal pivots)."""
    A = np.array(A, LD)
    n = A.shape[0]
    B = np.eye(n, dtype=LD)
    for k in range(n):
        piv = A[k, k]
        A[k] = A[k] / piv
        B[k] = B[k] / piv
        col = A[:, k].copy()
        col[k] = 0
        A -= np.outer(col, A[k])
        B -= np.outer(col, B[k])
    return B


def chol_ld(A):
    A = np.array(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_lower_ld(L, B):
    """inv(L) B by forward substitution."""
    L = np.asarray(L, LD)
    X = np.array(B, LD)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


# ---------------------------------------------------------------- prepare
def prepare(draws, lp_row=True):
    """draws: [nshards, P, S].  The prepared arrays as engine.dpe_prepare names them, in longdouble; shards with a
    NaN draw are left out."""
    X = np.asarray(draws, np.float64)
    ns, P, S = X.shape
    p = P - 1 if lp_row else P
    used = ~np.isnan(X).any(axis=(1, 2))
    Xu = X[used].astype(LD)
    M = Xu.shape[0]
    th = Xu[:, :p, :]
    mu_m = th.mean(axis=2)
    cen = th - mu_m[:, :, None]
    cov = np.einsum("mis,mjs->mij", cen, cen) / LD(S - 1)
    W = np.stack([inv_ld(c) for c in cov])
    Sig = inv_ld(W.sum(axis=0))
    mu = Sig @ np.einsum("mij,mj->i", W, mu_m)
    L = chol_ld(Sig)
    ldp = (p + 7) // 8 * 8
    Y = np.zeros((M, S, ldp), LD)
    n = np.zeros((M, S), LD)
    g = np.zeros((M, S), LD)
    for m in range(M):
        y = solve_lower_ld(L, th[m] - mu[:, None]) / np.sqrt(LD(M))
        Y[m, :, :p] = y.T
        n[m] = (y * y).sum(axis=0)
        g[m] = LD(0.5) * np.einsum("is,ij,js->s", cen[m], W[m], cen[m])
    out = {"M": M, "p": p, "S": S, "ldp": ldp, "lp_row": bool(lp_row), "shard_used": used, "mu": mu, "L": L, "Y": Y,
           "n": n, "g": g, "lpv": None, "lp_w": None, "mu_m": mu_m, "W": W, "Sigma": Sig}
    if lp_row:
        lp = Xu[:, p, :]
        w = 1 / lp.var(axis=1, ddof=1)
        out["lpv"] = lp
        out["lp_w"] = w / w.sum()
    return out


def as_float64(prep):
    """The prepared arrays rounded to fp64: what the library's samplers take."""
    out = dict(prep)
    for k in ("mu", "L", "Y", "n", "g", "lpv", "lp_w"):
        if prep[k] is not None:
            out[k] = np.ascontiguousarray(np.asarray(prep[k], np.float64))
    return out


def synthetic_prep(rng, M, S, p, lp_row=True):
    """Prepared arrays that no draws were whitened for (S may be <= p): random rows y, n = |y|^2, random g, a random
    lower factor.  The sampler's arithmetic does not care where its arrays came from."""
    ldp = (p + 7) // 8 * 8
    Y = np.zeros((M, S, ldp))
    Y[:, :, :p] = rng.standard_normal((M, S, p)) / np.sqrt(M)
    L = np.tril(rng.standard_normal((p, p))) * 0.3 + np.eye(p)
    out = {"M": M, "p": p, "S": S, "ldp": ldp, "lp_row": bool(lp_row), "shard_used": np.ones(M, bool),
           "mu": rng.standard_normal(p), "L": L, "Y": Y, "n": (Y * Y).sum(axis=2),
           "g": 0.5 * rng.chisquare(max(p, 1), (M, S)) / max(p, 1) * 3, "lpv": None, "lp_w": None}
    if lp_row:
        out["lpv"] = rng.standard_normal((M, S)) - 50.0
        w = rng.uniform(0.5, 2.0, M)
        out["lp_w"] = w / w.sum()
    return out


# ---------------------------------------------------------------- the mixture
def state(prep, t):
    """(s_t, N_t, G_t) of the index tuple t, longdouble, from scratch."""
    Y, n, g = (np.asarray(prep[k], LD) for k in ("Y", "n", "g"))
    m = np.arange(prep["M"])
    return Y[m, t, :prep["p"]].sum(axis=0), n[m, t].sum(), g[m, t].sum()


def logw(prep, t, h):
    s, N, G = state(prep, t)
    M, h2 = LD(prep["M"]), LD(h) * LD(h)
    q = s @ s
    return -(N - q / M) / (2 * h2) - q / (2 * M * (1 + h2)) + G


def emit(prep, t, h, z):
    """theta of the tuple t's component at the normals z [p] (and the lp__ row)."""
    s, _, _ = state(prep, t)
    M, h2 = LD(prep["M"]), LD(h) * LD(h)
    y = s / (M * (1 + h2)) + np.sqrt(h2 / (M * (1 + h2))) * np.asarray(z, LD)
    theta = np.asarray(prep["mu"], LD) + np.sqrt(M) * (np.asarray(prep["L"], LD) @ y)
    if prep["lp_row"]:
        lp = (np.asarray(prep["lp_w"], LD) * np.asarray(prep["lpv"], LD)[np.arange(prep["M"]), t]).sum()
        theta = np.append(theta, lp)
    return theta


def mixture_moments(prep, h):
    """Mean and covariance of theta under the whole mixture, by enumerating the S^M index tuples (tiny cases)."""
    M, S, p = prep["M"], prep["S"], prep["p"]
    Md, h2 = LD(M), LD(h) * LD(h)
    tuples = [np.array(t) for t in itertools.product(range(S), repeat=M)]
    lw = np.array([logw(prep, t, h) for t in tuples], LD)
    w = np.exp(lw - lw.max())
    w /= w.sum()
    L, mu = np.asarray(prep["L"], LD), np.asarray(prep["mu"], LD)
    means = np.stack([mu + np.sqrt(Md) * (L @ (state(prep, t)[0] / (Md * (1 + h2)))) for t in tuples])
    mean = w @ means
    within = (h2 / (1 + h2)) * (L @ L.T)            # M L (h^2 / (M (1 + h^2)) I) L^T
    d = means - mean
    return mean, within + np.einsum("t,ti,tj->ij", w, d, d)


def _trap(y, x):
    return ((y[1:] + y[:-1]) * (x[1:] - x[:-1])).sum() / 2


def quadrature_1d(draws, h, grid=None):
    """Mean and sd of prod_m p_m(theta) for one-dimensional shards, p_m straight from its definition
    p_m = N(. | mu_m, v_m) (1/S) sum_s N(. | theta_s, h^2 M v_M) / N(theta_s | mu_m, v_m), by the trapezoid rule."""
    X = np.asarray(draws, LD)                         # [M, S]
    M, S = X.shape
    mu_m, v_m = X.mean(axis=1), X.var(axis=1, ddof=1)
    vM = 1 / (1 / v_m).sum()
    if grid is None:
        muM = vM * (mu_m / v_m).sum()
        grid = np.linspace(float(muM - 12 * np.sqrt(vM)), float(muM + 12 * np.sqrt(vM)), 4001)
    x = np.asarray(grid, LD)
    kv = LD(h) * LD(h) * M * vM
    logp = np.zeros_like(x)
    for m in range(M):
        par = -(x - mu_m[m]) ** 2 / (2 * v_m[m])
        lw = (X[m] - mu_m[m]) ** 2 / (2 * v_m[m])     # 1 / N(theta_s | mu_m, v_m) up to a constant
        e = -(x[:, None] - X[m][None, :]) ** 2 / (2 * kv) + lw[None, :]
        mx = e.max(axis=1)
        logp += par + mx + np.log(np.exp(e - mx[:, None]).sum(axis=1))
    dens = np.exp(logp - logp.max())
    z = _trap(dens, x)
    mean = _trap(dens * x, x) / z
    var = _trap(dens * (x - mean) ** 2, x) / z
    return float(mean), float(np.sqrt(var))


# ---------------------------------------------------------------- random numbers
def _c3(tag, stream):
    return (int(stream) << 8) | tag


def _u53(x):
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def init_indices(seed, stream, K, M, S):
    """[K, M] starting indices."""
    from stark_amd import engine
    k, m = np.meshgrid(np.arange(K), np.arange(M), indexing="ij")
    a, b = engine.philox_words(seed, k, m >> 2, 0, _c3(TAG_INIT, stream))
    w64 = np.where(m & 2, b, a)
    word = np.where(m & 1, w64 >> np.uint64(32), w64 & np.uint64(0xFFFFFFFF))
    return ((word * np.uint64(S)) >> np.uint64(32)).astype(np.int64)


def proposals(seed, stream, K, sweeps, M, S):
    """([K, sweeps, M] proposed indices, [K, sweeps, M] log u in longdouble)."""
    from stark_amd import engine
    k, r, m = np.meshgrid(np.arange(K), np.arange(sweeps), np.arange(M), indexing="ij")
    a, b = engine.philox_words(seed, k, r, m, _c3(TAG_PROP, stream))
    c = (((a & np.uint64(0xFFFFFFFF)) * np.uint64(S)) >> np.uint64(32)).astype(np.int64)
    return c, np.log(_u53(b).astype(LD))


def normals(seed, stream, chain, draw, p):
    from stark_amd import engine
    i = np.arange(p)
    a, b = engine.philox_words(seed, chain, draw, i >> 1, _c3(TAG_NORM, stream))
    rad = np.sqrt(-2 * np.log(_u53(a).astype(LD)))
    th = 2 * np.pi * _u53(b).astype(LD)
    return np.where(i & 1, rad * np.sin(th), rad * np.cos(th))


# ---------------------------------------------------------------- replay
def replay(prep, h, seed, stream, T, K, burn, thin, trace_idx):
    """Follow a run's index trace in longdouble.  Returns
    logw [K, sweeps]: log W of the traced state at the end of every sweep, recomputed from scratch;
    wrong: proposals whose traced decision contradicts the recomputed margin log W' - log W - log u;
    min_margin: the smallest |margin| over proposals with c != the current index;
    out [P, T]: the draws of the traced states at this module's normals;
    rows p (+ 1) x T; columns no chain emits stay NaN."""
    M, S, p = prep["M"], prep["S"], prep["p"]
    sweeps = burn + thin * (-(-T // K))
    h = np.broadcast_to(np.asarray(h, np.float64), (sweeps,))
    init = init_indices(seed, stream, K, M, S)
    prop, logu = proposals(seed, stream, K, sweeps, M, S)
    lw_out = np.zeros((K, sweeps), LD)
    out = np.full((p + (1 if prep["lp_row"] else 0), T), np.nan, LD)
    wrong, min_margin = 0, np.inf
    for k in range(K):
        t = init[k].copy()
        for r in range(sweeps):
            lw = logw(prep, t, h[r])
            for m in range(M):
                c, after = prop[k, r, m], trace_idx[k, r, m]
                t2 = t.copy()
                t2[m] = c
                lw2 = logw(prep, t2, h[r])
                margin = (lw2 - lw) - logu[k, r, m]
                if c != t[m]:
                    min_margin = min(min_margin, abs(float(margin)))
                    took = after == c
                    wrong += int(took != (margin > 0))
                    if after not in (c, t[m]):
                        wrong += 1
                if after == c and c != t[m]:
                    t, lw = t2, lw2
            lw_out[k, r] = lw
            e = r + 1 - burn
            if e > 0 and e % thin == 0:
                col = (e // thin - 1) * K + k
                if col < T:
                    out[:, col] = emit(prep, t, h[r], normals(seed, stream, k, e // thin - 1, p))
    return {"logw": lw_out, "wrong": wrong, "min_margin": min_margin, "out": out}
