"""numpy restatement of the quantitative-genetics analyses (geonomics_amd/sim/quantgen.py,
csrc/gnx_grm.hip) for the tests: dense fp64 brute force that shares no code with the package.

  table_direct / grm_from_dosages   the standardised relationship matrix from its definition
  reml_logl_dense / reml_brute      the restricted likelihood with slogdet and solve, maximised
                                    over log10(delta) with scipy's bounded scalar minimiser
  se_h2_numeric                     delta-method s.e. from a numeric Hessian of the dense logL
  blup_dense / blup_marker          BLUP from V^-1, and from the equivalent ridge regression
  grm_bound                         the error bound of gnx_grm's sums
"""
import numpy as np


def table_direct(c1, n, kind='additive', method='gcta', alpha=-1.0, min_maf=0.01):
    """(val float64 [L][3], used bool [L]) locus by locus from the definitions"""
    c1 = np.asarray(c1, dtype=np.int64)
    L = c1.size
    used = np.zeros(L, bool)
    for l in range(L):
        p = c1[l] / (2.0 * n)
        used[l] = 0 < c1[l] < 2 * n and min(p, 1 - p) >= min_maf
    m = int(used.sum())
    h = np.array([2.0 * (c / (2.0 * n)) * (1 - c / (2.0 * n)) for c in c1])
    val = np.zeros((L, 3))
    for l in np.flatnonzero(used):
        p = c1[l] / (2.0 * n)
        for d in range(3):
            if kind == 'dominance':
                num = (0.0, 2 * p, 4 * p - 2)[d] - 2 * p * p
                val[l, d] = num / (h[l] * np.sqrt(m))
            elif method == 'gcta':
                val[l, d] = (d - 2 * p) / np.sqrt(h[l] * m)
            elif method == 'vanraden':
                val[l, d] = (d - 2 * p) / np.sqrt(h[used].sum())
            else:
                val[l, d] = (d - 2 * p) * h[l] ** (alpha / 2) / np.sqrt((h[used] ** (1 + alpha)).sum())
    return val, used


def expand(val, D):
    """Z [n][L]: Z[i][l] = val[l][D[i][l]]"""
    D = np.asarray(D, dtype=np.int64)
    return np.take_along_axis(np.asarray(val)[None, :, :], D[:, :, None], axis=2)[:, :, 0]


def grm_from_dosages(D, kind='additive', method='gcta', alpha=-1.0, min_maf=0.01, fp32=True):
    """(G float64 [n][n], used, Z) of dosages D [n][L]; fp32: the table rounded to float32 as the
    device reads it, the sums in fp64"""
    D = np.asarray(D, dtype=np.int64)
    val, used = table_direct(D.sum(0), D.shape[0], kind, method, alpha, min_maf)
    if fp32:
        val = val.astype(np.float32).astype(np.float64)
    Z = expand(val, D)
    return Z @ Z.T, used, Z


def grm_bound(Zabs, n_loci):
    """|G_ij - exact| <= (1.01 * 1024 * 2^-24 + L * 2^-53) * S_ij with S = |Z| |Z|^T: an fp32 fma
    chain of at most 1024 products (first-order bound 1024 u S, u = 2^-24, with 1 % for the
    higher orders), then an fp64 sum of the chains"""
    S = Zabs @ Zabs.T
    return (1.01 * 1024 * 2.0 ** -24 + n_loci * 2.0 ** -53) * S


def reml_logl_dense(G, y, X, sg2, se2):
    """-1/2 [(n - c) log 2 pi + log|V| + log|X^T V^-1 X| + y^T P y], V = sg2 G + se2 I"""
    n, c = X.shape
    V = sg2 * G + se2 * np.eye(n)
    ViX = np.linalg.solve(V, X)
    Viy = np.linalg.solve(V, y)
    A = X.T @ ViX
    yPy = y @ Viy - (X.T @ Viy) @ np.linalg.solve(A, X.T @ Viy)
    return -0.5 * ((n - c) * np.log(2 * np.pi) + np.linalg.slogdet(V)[1]
                   + np.linalg.slogdet(A)[1] + yPy)


def _profile(G, y, X, x):
    """(logL, sg2) at delta = 10^x with sg2 at its maximiser y^T P_H y / (n - c), H = G + delta I"""
    n, c = X.shape
    H = G + 10.0 ** x * np.eye(n)
    HiX = np.linalg.solve(H, X)
    Hiy = np.linalg.solve(H, y)
    R = y @ Hiy - (X.T @ Hiy) @ np.linalg.solve(X.T @ HiX, X.T @ Hiy)
    sg2 = R / (n - c)
    return reml_logl_dense(G, y, X, sg2, sg2 * 10.0 ** x), sg2


def reml_brute(G, y, X):
    """the maximum over log10(delta) in [-10, 10]: a grid of step 0.25, then scipy's bounded
    minimiser around the best node -> dict(h2, Vg, Ve, logL, logL0, delta, x, at_boundary)"""
    from scipy.optimize import minimize_scalar
    n, c = X.shape
    grid = np.linspace(-10, 10, 81)
    ll = np.array([_profile(G, y, X, x)[0] for x in grid])
    k = int(np.argmax(ll))
    a, b = grid[max(k - 1, 0)], grid[min(k + 1, 80)]
    res = minimize_scalar(lambda x: -_profile(G, y, X, x)[0], bounds=(a, b), method='bounded',
                          options=dict(xatol=1e-13, maxiter=500))
    x = float(res.x)
    # the bounded minimiser never returns an end.  Where the best node lies within a decade of an
    # end, that end is the maximum if the likelihood there is no lower than what the minimiser
    # found, rounding aside (the dense solves carry about 1e-10 of relative noise where delta is
    # 1e-10, more than the likelihood changes over that decade)
    for end in (0, 80):
        if abs(k - end) <= 4 and ll[end] >= -res.fun - 1e-9 * abs(res.fun):
            x = float(grid[end])
    logL, sg2 = _profile(G, y, X, x)
    r = y - X @ np.linalg.lstsq(X, y, rcond=None)[0]
    s0 = r @ r / (n - c)
    logL0 = -0.5 * ((n - c) * np.log(2 * np.pi) + (n - c) * np.log(s0)
                    + np.linalg.slogdet(X.T @ X)[1] + (n - c))
    return dict(h2=1 / (1 + 10.0 ** x), Vg=sg2, Ve=sg2 * 10.0 ** x, logL=logL, logL0=logL0,
                delta=10.0 ** x, x=x, at_boundary=abs(x) == 10.0)


def se_h2_numeric(G, y, X, sg2, se2, rel=1e-3):
    """delta-method s.e. of h2 = sg2 / (sg2 + se2) from the central-difference Hessian of the
    dense restricted likelihood in (sg2, se2)"""
    t0 = np.array([sg2, se2])
    h = rel * t0

    def f(t):
        return reml_logl_dense(G, y, X, t[0], t[1])

    Hm = np.empty((2, 2))
    for i in range(2):
        for j in range(2):
            ei, ej = np.eye(2)[i] * h[i], np.eye(2)[j] * h[j]
            Hm[i, j] = (f(t0 + ei + ej) - f(t0 + ei - ej) - f(t0 - ei + ej) + f(t0 - ei - ej)) \
                / (4 * h[i] * h[j])
    cov = np.linalg.inv(-Hm)
    g = np.array([se2, -sg2]) / (sg2 + se2) ** 2
    return float(np.sqrt(g @ cov @ g))


def he_dense(G, y, X):
    """Haseman-Elston: slope of r_i r_j on G_ij over i < j, r the unit-variance OLS residual"""
    n, c = X.shape
    r = y - X @ np.linalg.lstsq(X, y, rcond=None)[0]
    r = r / np.sqrt(r @ r / (n - c))
    g, z = [], []
    for i in range(n):
        g.append(G[i, i + 1:])
        z.append(r[i] * r[i + 1:])
    return float(np.polyfit(np.concatenate(g), np.concatenate(z), 1)[0])


def blup_dense(G, y, X, delta, train=None):
    """(g_hat [n], beta): G[:, t] V_tt^-1 (y_t - X_t beta), V_tt = G_tt + delta I, beta by GLS"""
    t = np.arange(G.shape[0]) if train is None else np.asarray(train)
    V = G[np.ix_(t, t)] + delta * np.eye(t.size)
    ViX = np.linalg.solve(V, X[t])
    beta = np.linalg.solve(X[t].T @ ViX, ViX.T @ y[t])
    return G[:, t] @ np.linalg.solve(V, y[t] - X[t] @ beta), beta


def blup_marker(Z, y, X, delta, beta):
    """the same prediction in its marker-effect form: Z (Z^T Z + delta I)^-1 Z^T (y - X beta)
    with Z Z^T = G (ridge regression on the standardised genotypes)"""
    m = Z.shape[1]
    return Z @ np.linalg.solve(Z.T @ Z + delta * np.eye(m), Z.T @ (y - X @ beta))
