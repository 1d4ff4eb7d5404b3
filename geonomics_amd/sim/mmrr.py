"""Isolation by distance and by environment: MMRR and (partial) Mantel tests (reference
demos/_IBD_IBE.py:195-330 -> data/IBD_IBE_demo/MMRR.py:7-74, a port of Wang's MMRR that refits
statsmodels' OLS on the n (n - 1) / 2 unfolded pairs once per permutation, and
data/IBD_IBE_demo/run_mantel.R: vegan's mantel.partial(gen, env, geo)) from cross-sums.

Y is the genetic distance matrix, X_1 .. X_K the predictor distance matrices, all unfolded to
their m = n (n - 1) / 2 pairs i > j.  Both tests permute the rows and columns of Y only, and
under a permutation just the cross-sums S_k = sum_{i>j} Y[r_i][r_j] X_k[i][j] change: m,
sum y, sum y^2, sum x_k and sum x_k x_l do not.  Nothing here sees a matrix: from
(sums [n_perm][K], moments) - gnx_dist_perm_sums - follow, by centred fp64 algebra,
    the OLS fit of every permutation: coefficients, t-values, F and R^2 (MMRR), and
    Pearson's r between Y and X_k, and the partial r given another predictor (Mantel).
Pure functions, fp64.
"""
from collections import OrderedDict

import numpy as np


# ------------------------------------------------------------------ permutations
def draw_row_shuffles(n, nperm, seed=None, rng=None):
    """the reference's permutations (MMRR.py:48-53): the list of row numbers shuffled again and
    again, permutation p being the state after p + 1 shuffles -> int64 [nperm][n].  seed: a
    fresh np.random.RandomState(seed), which replays np.random.seed(seed) followed by
    np.random.shuffle; else rng (e.g. the Model's), else numpy's global state"""
    if nperm < 1:
        raise ValueError('nperm: at least 1 permutation (got %r)' % (nperm,))
    if seed is not None:
        rng = np.random.RandomState(seed)
    elif rng is None:
        rng = np.random
    rows = np.arange(int(n))
    out = np.empty((int(nperm), int(n)), np.int64)
    for p in range(int(nperm)):
        rng.shuffle(rows)
        out[p] = rows
    return out


def invert_rows(rows):
    """the library's convention from the reference's: Yperm = Y[r][:, r] pairs individual
    r[i] of Y with the predictors of individual i, so individual a takes the columns of
    perm[a] = r^-1[a]"""
    rows = np.asarray(rows, np.int64)
    perm = np.empty(rows.shape, np.int32)
    np.put_along_axis(perm, rows, np.arange(rows.shape[1], dtype=np.int32)[None, :], axis=1)
    return perm


# ------------------------------------------------------------------ the moments
def _centred(mom):
    """m, mean y, mean x [K], cyy, cxx [K][K] of the centred pairs, and sy, sx"""
    m = float(mom['m'])
    sx = np.asarray(mom['sx'], np.float64)
    sxx = np.asarray(mom['sxx'], np.float64)
    sy, syy = float(mom['sy']), float(mom['syy'])
    return m, sy / m, sx / m, syy - sy * sy / m, sxx - np.outer(sx, sx) / m


def _cxy(S, mom):
    """centred cross-products [..., K] of cross-sums S [..., K]"""
    sx = np.asarray(mom['sx'], np.float64)
    return np.asarray(S, np.float64) - sx * (float(mom['sy']) / float(mom['m']))


# ------------------------------------------------------------------ MMRR
def ols_from_sums(S, mom):
    """the OLS fit y ~ 1 + x_1 + .. + x_K of every row of S [..., K] (one permutation each)
    -> dict(coef [..., K + 1] (intercept first), t [..., K + 1], F [...], r2 [...])"""
    m, ybar, xbar, cyy, cxx = _centred(mom)
    K = xbar.size
    dof = m - K - 1
    if dof < 1:
        raise ValueError('MMRR: %d pairs leave no residual degrees of freedom for %d '
                         'predictors and an intercept' % (m, K))
    cxy = _cxy(S, mom)
    cinv = np.linalg.inv(cxx)
    slopes = cxy @ cinv                                   # cinv is symmetric
    icpt = ybar - slopes @ xbar
    ess = np.einsum('...k,...k->...', slopes, cxy)        # explained sum of squares
    rss = cyy - ess
    s2 = rss / dof
    var = np.concatenate([[1.0 / m + xbar @ cinv @ xbar], np.diag(cinv)])
    coef = np.concatenate([icpt[..., None], slopes], axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = coef / np.sqrt(s2[..., None] * var)
        F = (ess / K) / s2
        r2 = 1.0 - rss / cyy
    return dict(coef=coef, t=t, F=F, r2=r2)


def mmrr(sums, mom, names=None):
    """MMRR.py's MMRR(Y, X, Xnames, nperm) from the permuted cross-sums [nperm][K] and the
    moments (the observed fit is that of mom['sxy']) -> OrderedDict with the reference's keys
    in its order: 'R^2', 'Intercept', names, '<name>(t)', '<name>(p)', 'F-statistic',
    'F p-value'"""
    sums = np.asarray(sums, np.float64)
    if sums.ndim != 2 or sums.shape[0] < 1:
        raise ValueError('sums: [nperm][K] with nperm >= 1')
    nperm, K = sums.shape
    if names is None:
        names = ['X%i' % i for i in range(1, K + 1)]
    if len(names) != K:
        raise ValueError('%d names for %d predictors' % (len(names), K))
    obs = ols_from_sums(np.asarray(mom['sxy'], np.float64), mom)
    per = ols_from_sums(sums, mom)
    tp = (1.0 + (np.abs(per['t']) >= np.abs(obs['t'])).sum(axis=0)) / (nperm + 1)
    Fp = (1.0 + (per['F'] >= obs['F']).sum()) / (nperm + 1)
    cn = ['Intercept'] + list(names)
    out = OrderedDict()
    out['R^2'] = float(obs['r2'])
    out.update({c: float(v) for c, v in zip(cn, obs['coef'])})
    out.update({c + '(t)': float(v) for c, v in zip(cn, obs['t'])})
    out.update({c + '(p)': float(v) for c, v in zip(cn, tp)})
    out['F-statistic'] = float(obs['F'])
    out['F p-value'] = float(Fp)
    return out


# ------------------------------------------------------------------ Mantel
def mantel_r(S, mom, x=0, given=None):
    """Pearson's r between the pairs of Y and of predictor x for every row of S [..., K];
    given: the partial r_{Y x . given} = (r_Yx - r_Yg r_xg) / sqrt((1 - r_Yg^2)(1 - r_xg^2))
    (vegan's mantel / mantel.partial with Y the permuted matrix)"""
    m, ybar, xbar, cyy, cxx = _centred(mom)
    cxy = _cxy(S, mom)
    r = cxy[..., x] / np.sqrt(cyy * cxx[x, x])
    if given is None:
        return r
    ryg = cxy[..., given] / np.sqrt(cyy * cxx[given, given])
    rxg = cxx[x, given] / np.sqrt(cxx[x, x] * cxx[given, given])
    return (r - ryg * rxg) / np.sqrt((1.0 - ryg * ryg) * (1.0 - rxg * rxg))


def mantel(sums, mom, x=0, given=None):
    """the (partial) Mantel test -> dict(r, p = (1 + #{r_perm >= r}) / (nperm + 1), nperm,
    perm_r [nperm])"""
    sums = np.asarray(sums, np.float64)
    if sums.ndim != 2 or sums.shape[0] < 1:
        raise ValueError('sums: [nperm][K] with nperm >= 1')
    if float(mom['m']) < 3:
        raise ValueError('Mantel: at least 3 individuals (got %d pairs)' % mom['m'])
    r = float(mantel_r(np.asarray(mom['sxy'], np.float64), mom, x, given))
    perm_r = mantel_r(sums, mom, x, given)
    nperm = sums.shape[0]
    return dict(r=r, p=(1.0 + (perm_r >= r).sum()) / (nperm + 1), nperm=nperm, perm_r=perm_r)


# ------------------------------------------------------------------ the host restatement
def unfold_tril(A):
    """the pairs i > j of a matrix, row by row (MMRR.py's _unfold_tril)"""
    A = np.asarray(A)
    return A[np.tril_indices(A.shape[0], k=-1)]


def euclid(f):
    """pairwise Euclidean distances [n][n] of the rows of f [n][d] (or [n]), fp64"""
    f = np.asarray(f, np.float64)
    f = f[:, None] if f.ndim == 1 else f
    d = f[:, None, :] - f[None, :, :]
    return np.sqrt((d * d).sum(axis=2))


def genetic_distances(D):
    """0.5 sqrt(G_aa + G_bb - 2 G_ab), G = D D^T, of integer dosages D [n][L]
    (Species._calc_genetic_distances)"""
    Di = np.asarray(D).astype(np.int64)
    G = Di @ Di.T
    g = np.diag(G)
    return 0.5 * np.sqrt((g[:, None] + g[None, :] - 2 * G).astype(np.float64))


def numpy_moments(Y, Xs):
    """the moments gnx_dist_perm_sums returns, in numpy, of matrices Y and Xs [K]"""
    y = unfold_tril(Y).astype(np.float64)
    x = np.stack([unfold_tril(X).astype(np.float64) for X in Xs])
    return dict(m=float(y.size), sy=y.sum(), syy=y @ y, sx=x.sum(axis=1), sxy=x @ y,
                sxx=x @ x.T)


def numpy_perm_sums(Y, Xs, rows):
    """S [nperm][K] of the reference's row shuffles `rows`: sum_{i>j} Y[r_i][r_j] X_k[i][j]"""
    Y = np.asarray(Y, np.float64)
    x = np.stack([unfold_tril(X).astype(np.float64) for X in Xs])
    out = np.empty((len(rows), x.shape[0]))
    for p, r in enumerate(rows):
        out[p] = x @ unfold_tril(Y[r][:, r])
    return out
