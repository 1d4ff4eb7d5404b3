"""Quantitative genetics on a genomic relationship matrix (GRM): the host arithmetic behind
Model.calc_grm, calc_heritability and predict_breeding_values (an extension: the reference
has no such analyses).

The device computes G_ij = sum_l val[l][d_il] val[l][d_jl] from the packed genomes (gnx_grm,
csrc/gnx_grm.hip: f32 MFMA with fp64 sums); this module writes the table `val` (grm_values)
and works on the n x n matrix that comes back:

  reml           the one-component mixed model y = X b + g + e, g ~ N(0, sg2 G), e ~ N(0, se2 I),
                 fitted by restricted maximum likelihood in the eigenbasis of G (EMMA, Kang et al.
                 2008; GEMMA, Zhou & Stephens 2012): with G = U diag(s) U^T and delta = se2 / sg2,
                 V = sg2 U diag(s + delta) U^T, so every quantity is a sum over n terms
  he_regression  Haseman-Elston regression, a non-iterative check of reml's h2
  gblup          the best linear unbiased prediction of the breeding values g

Pure numpy/scipy, fp64; nothing here needs a device.
"""
import numpy as np

KINDS = ('additive', 'dominance')
METHODS = ('gcta', 'vanraden', 'alpha')
GRM_MAX = 8192              # individuals per relationship matrix (the matrix is n x n)
LOG10_DELTA = (-10.0, 10.0)


def check_request(who, kind='additive', method='gcta', alpha=-1.0, min_maf=0.01):
    """ValueError unless the kind, the weighting and its parameters are known"""
    if kind not in KINDS:
        raise ValueError("%s: kind: 'additive' or 'dominance', not %r" % (who, kind))
    if method not in METHODS:
        raise ValueError("%s: method: 'gcta', 'vanraden' or 'alpha', not %r" % (who, method))
    if isinstance(alpha, bool) or not np.isfinite(alpha):
        raise ValueError('%s: alpha: a finite exponent of 2pq (got %r)' % (who, alpha))
    if isinstance(min_maf, bool) or not 0 <= min_maf < 0.5:
        raise ValueError('%s: min_maf: in [0, 0.5) (got %r)' % (who, min_maf))


def grm_values(c1, n, kind='additive', method='gcta', alpha=-1.0, min_maf=0.01, subset=None,
               weights=None):
    """the table of gnx_grm and the loci it uses, from the sample's exact 1-allele counts c1 [L]
    of n individuals.  With p = c1 / 2n, q = 1 - p and m the number of used loci, the value of a
    locus at dosage d is
      additive, 'gcta'      (d - 2p) / sqrt(2pq m)                    (Yang et al. 2011)
      additive, 'vanraden'  (d - 2p) / sqrt(sum_l 2pq)                (VanRaden 2008, method 1)
      additive, 'alpha'     (d - 2p) (2pq)^(alpha/2) / sqrt(sum_l (2pq)^(1 + alpha))
                            (Speed et al. 2012; alpha = -1 is 'gcta', alpha = 0 'vanraden')
      dominance             {-2p^2, 2p - 2p^2, (4p - 2) - 2p^2}[d] / (2pq sqrt(m))
                            (Zhu et al. 2015; `method` does not apply)
    so that the mean of the diagonal of G is about 1.  Loci that are monomorphic in the sample,
    whose minor allele frequency is below min_maf, or outside `subset` (bool [L]) are not used:
    their rows are zero.  weights [L] multiplies the rows (LD-weighted GRMs).
    -> (val float32 [L][3], used bool [L])"""
    check_request('grm_values', kind, method, alpha, min_maf)
    c1 = np.asarray(c1, dtype=np.int64).ravel()
    if isinstance(n, bool) or int(n) != n or n < 1:
        raise ValueError('grm_values: n: a positive number of individuals (got %r)' % (n,))
    if c1.size and (c1.min() < 0 or c1.max() > 2 * n):
        raise ValueError('grm_values: counts outside 0..2n')
    p = c1 / (2.0 * n)
    q = 1.0 - p
    used = (c1 > 0) & (c1 < 2 * n) & (np.minimum(p, q) >= min_maf)
    if subset is not None:
        subset = np.asarray(subset, dtype=bool).ravel()
        if subset.size != c1.size:
            raise ValueError('grm_values: subset: %d entries for %d loci' % (subset.size, c1.size))
        used &= subset
    if weights is not None:
        weights = np.asarray(weights, dtype=np.float64).ravel()
        if weights.size != c1.size or not np.isfinite(weights).all():
            raise ValueError('grm_values: weights: finite values [L = %d] (got %s)'
                             % (c1.size, weights.shape))
    val = np.zeros((c1.size, 3), np.float64)
    m = int(used.sum())
    if m:
        pu, h = p[used], 2.0 * p[used] * q[used]
        d = np.arange(3.0)
        if kind == 'dominance':
            num = np.stack([-2 * pu ** 2, 2 * pu - 2 * pu ** 2, (4 * pu - 2) - 2 * pu ** 2], 1)
            v = num / (h * np.sqrt(m))[:, None]
        else:
            a = {'gcta': -1.0, 'vanraden': 0.0, 'alpha': float(alpha)}[method]
            scale = h ** (a / 2.0) / np.sqrt(np.sum(h ** (1.0 + a)))
            v = (d[None, :] - 2 * pu[:, None]) * scale[:, None]
        if weights is not None:
            v = v * weights[used][:, None]
        val[used] = v
    return val.astype(np.float32), used


def eig_grm(G):
    """(evals ascending, U) of the symmetric G, fp64"""
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1]:
        raise ValueError('eig_grm: a square matrix (got %s)' % (G.shape,))
    return np.linalg.eigh(G)


def _design(y, X, n=None):
    y = np.asarray(y, dtype=np.float64).ravel()
    n = y.size if n is None else n
    X = np.ones((n, 1)) if X is None else np.asarray(X, dtype=np.float64)
    X = X[:, None] if X.ndim == 1 else X
    if X.ndim != 2 or X.shape[0] != n or y.size != n:
        raise ValueError('y [n] and X [n][c] of one n (got %s and %s)' % (y.shape, X.shape))
    if X.shape[1] >= n or np.linalg.matrix_rank(X) < X.shape[1]:
        raise ValueError('X: %d columns of full rank for %d individuals' % (X.shape[1], n))
    return y, X


class _Rotated:
    """y and X in the eigenbasis of G, and the restricted likelihood as a function of
    x = log10(delta)"""

    def __init__(self, evals, U, y, X):
        self.s = np.maximum(np.asarray(evals, dtype=np.float64).ravel(), 0.0)
        U = np.asarray(U, dtype=np.float64)
        self.n, self.c = X.shape
        if U.shape != (self.n, self.n) or self.s.size != self.n:
            raise ValueError('evals [n] and U [n][n] for n = %d (got %s and %s)'
                             % (self.n, self.s.shape, U.shape))
        self.yt = U.T @ y
        self.Xt = U.T @ X
        self.df = self.n - self.c

    def parts(self, delta):
        """d = 1 / (s + delta), A = X^T D X, beta, the residual r and R = r^T D r"""
        d = 1.0 / (self.s + delta)
        XD = self.Xt * d[:, None]
        A = self.Xt.T @ XD
        beta = np.linalg.solve(A, XD.T @ self.yt)
        r = self.yt - self.Xt @ beta
        return d, XD, A, beta, r, float(np.sum(d * r * r))

    def logl(self, x):
        """-1/2 [(n - c) log 2 pi + log|V| + log|X^T V^-1 X| + y^T P y] at sg2 = R / (n - c)"""
        delta = 10.0 ** x
        d, _, A, _, _, R = self.parts(delta)
        df = self.df
        return -0.5 * (df * np.log(2 * np.pi) + df * np.log(R / df) - np.sum(np.log(d))
                       + np.linalg.slogdet(A)[1] + df)

    def dlogl(self, x):
        """d logl / d ln(delta)"""
        delta = 10.0 ** x
        d, XD, A, _, r, R = self.parts(delta)
        tr = np.trace(np.linalg.solve(A, XD.T @ XD))
        return -0.5 * delta * (-self.df * np.sum(d * d * r * r) / R + np.sum(d) - tr)

    def information(self, sg2, se2):
        """the observed information of (sg2, se2): I_ij = y^T P V_i P V_j P y - tr(P V_i P V_j) / 2
        with V_g = diag(s), V_e = I in the eigenbasis, P = W - Z A^-1 Z^T, W = 1 / (sg2 s + se2),
        Z = W X"""
        w = 1.0 / (sg2 * self.s + se2)
        Z = self.Xt * w[:, None]
        Ai = np.linalg.inv(self.Xt.T @ Z)
        q = w * self.yt - Z @ (Ai @ (Z.T @ self.yt))           # P y
        S = (self.s, np.ones(self.n))
        info = np.empty((2, 2))
        for i in range(2):
            for j in range(i, 2):
                ui, uj = S[i] * q, S[j] * q
                quad = np.sum(ui * w * uj) - (Z.T @ ui) @ Ai @ (Z.T @ uj)
                Bi = Ai @ (Z.T @ (Z * S[i][:, None]))
                Bj = Ai @ (Z.T @ (Z * S[j][:, None]))
                tr = (np.sum(w * w * S[i] * S[j])
                      - 2.0 * np.trace(Ai @ (Z.T @ (Z * (S[i] * w * S[j])[:, None])))
                      + np.trace(Bi @ Bj))
                info[i, j] = info[j, i] = quad - 0.5 * tr
        return info


def reml(evals, U, y, X=None):
    """restricted maximum likelihood of y = X b + g + e, g ~ N(0, sg2 G), e ~ N(0, se2 I), with
    G = U diag(evals) U^T (eigenvalues clamped at 0) and X [n][c] (None: an intercept).  A
    bounded search over x = log10(delta), delta = se2 / sg2, in [-10, 10]: a grid of step 0.1,
    then the root of the analytic derivative in the bracket around the best node (Brent).
    -> dict: h2 = sg2 / (sg2 + se2), se_h2 (delta method from the observed information of
    (sg2, se2); NaN where that is singular), Vg, Ve, beta [c], logL, logL0 (the fit with
    sg2 = 0), lrt_p (1/2 chi2_1 sf of 2 (logL - logL0)), delta, at_boundary (the maximum lies at
    an end of the interval: h2 is then 1 / (1 + 10^-+10))"""
    from scipy.optimize import brentq, minimize_scalar
    from scipy.stats import chi2
    y, X = _design(y, X)
    rot = _Rotated(evals, U, y, X)
    lo, hi = LOG10_DELTA
    grid = np.linspace(lo, hi, 201)
    ll = np.array([rot.logl(x) for x in grid])
    k = int(np.argmax(ll))
    at_boundary = False
    if k == 0 and rot.dlogl(lo) <= 0:
        x, at_boundary = lo, True
    elif k == grid.size - 1 and rot.dlogl(hi) >= 0:
        x, at_boundary = hi, True
    else:
        a, b = grid[max(k - 1, 0)], grid[min(k + 1, grid.size - 1)]
        if rot.dlogl(a) > 0 > rot.dlogl(b):
            x = brentq(rot.dlogl, a, b, xtol=1e-14, rtol=8.9e-16, maxiter=200)
        else:
            x = minimize_scalar(lambda t: -rot.logl(t), bounds=(a, b), method='bounded',
                                options=dict(xatol=1e-12)).x
    delta = 10.0 ** x
    _, _, _, beta, _, R = rot.parts(delta)
    Vg = R / rot.df
    Ve = delta * Vg
    logL = float(rot.logl(x))
    # sg2 = 0: ordinary least squares
    b0 = np.linalg.lstsq(X, y, rcond=None)[0]
    rss = float(np.sum((y - X @ b0) ** 2))
    logL0 = -0.5 * (rot.df * np.log(2 * np.pi) + rot.df * np.log(rss / rot.df)
                    + np.linalg.slogdet(X.T @ X)[1] + rot.df)
    h2 = Vg / (Vg + Ve)
    se_h2 = np.nan
    try:
        cov = np.linalg.inv(rot.information(Vg, Ve))
        grad = np.array([Ve, -Vg]) / (Vg + Ve) ** 2
        var = float(grad @ cov @ grad)
        if np.isfinite(var) and var >= 0:
            se_h2 = float(np.sqrt(var))
    except np.linalg.LinAlgError:
        pass
    return dict(h2=float(h2), se_h2=se_h2, Vg=float(Vg), Ve=float(Ve), beta=beta, logL=logL,
                logL0=float(logL0), lrt_p=float(0.5 * chi2.sf(max(2.0 * (logL - logL0), 0.0), 1)),
                delta=float(delta), at_boundary=bool(at_boundary))


def he_regression(G, y, X=None):
    """Haseman-Elston regression: the response is residualised on X (None: an intercept) and
    scaled to unit variance (residual sum of squares / (n - c)); the slope of the ordinary
    regression of the products r_i r_j on G_ij over the pairs i < j estimates h2 without
    iteration (it may fall outside [0, 1]).  NaN when the off-diagonal of G does not vary"""
    G = np.asarray(G, dtype=np.float64)
    y, X = _design(y, X, G.shape[0])
    r = y - X @ np.linalg.lstsq(X, y, rcond=None)[0]
    r = r / np.sqrt(np.sum(r * r) / (X.shape[0] - X.shape[1]))
    iu = np.triu_indices(G.shape[0], 1)
    g = G[iu]
    z = r[iu[0]] * r[iu[1]]
    gc = g - g.mean()
    den = float(np.sum(gc * gc))
    return float(np.sum(gc * (z - z.mean())) / den) if den > 0 else float('nan')


def gblup(evals, U, y, X=None, delta=None, train=None):
    """best linear unbiased prediction of the breeding values of every individual of
    G = U diag(evals) U^T: g_hat = G[:, train] V_tt^-1 (y_t - X_t beta) with V_tt = G_tt + delta I
    and beta the generalised least squares estimate on the training individuals.  train: their
    indices (None: everybody; then y of the others is not read).  delta = se2 / sg2 (None: fitted
    by reml on the training individuals' sub-matrix)
    -> dict: g_hat [n], y_hat = X beta + g_hat [n], beta [c], delta, fit (reml's dict when delta
    was fitted, else None)"""
    s = np.maximum(np.asarray(evals, dtype=np.float64).ravel(), 0.0)
    U = np.asarray(U, dtype=np.float64)
    n = s.size
    y = np.asarray(y, dtype=np.float64).ravel()
    X = np.ones((n, 1)) if X is None else np.asarray(X, dtype=np.float64)
    X = X[:, None] if X.ndim == 1 else X
    if U.shape != (n, n) or y.size != n or X.shape[0] != n:
        raise ValueError('gblup: evals [n], U [n][n], y [n], X [n][c] of one n')
    fit = None
    if train is None:
        st, Ut, yt, Xt, cross = s, U, y, X, None
    else:
        train = np.asarray(train, dtype=np.int64).ravel()
        if train.size < 2 or train.min() < 0 or train.max() >= n or \
                np.unique(train).size != train.size:
            raise ValueError('gblup: train: distinct indices in 0..%d' % (n - 1))
        cross = (U * s) @ U[train].T                       # G[:, train]
        st, Ut = np.linalg.eigh(cross[train])
        st = np.maximum(st, 0.0)
        yt, Xt = y[train], X[train]
    yt, Xt = _design(yt, Xt)
    if delta is None:
        fit = reml(st, Ut, yt, Xt)
        delta = fit['delta']
    if not delta > 0:
        raise ValueError('gblup: delta: a positive ratio se2 / sg2 (got %r)' % (delta,))
    rot = _Rotated(st, Ut, yt, Xt)
    d, _, _, beta, r, _ = rot.parts(float(delta))
    if cross is None:
        g_hat = Ut @ (st * d * r)
    else:
        g_hat = cross @ (Ut @ (d * r))
    return dict(g_hat=g_hat, y_hat=X @ beta + g_hat, beta=beta, delta=float(delta), fit=fit)
