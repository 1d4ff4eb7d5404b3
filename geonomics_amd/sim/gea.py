"""Genotype-environment association by canonical correlation (reference sim/model.py:2717-2780,
Model.run_gea -> structs/species.py:2269-2355, Species._run_cca: sklearn's
CCA(n_components=3).fit(genotypes, [env, lat, long]), i.e. NIPALS with mode B and canonical
deflation on the centred, unit-variance columns) from cross-products with the dosage matrix.

D is the N x n_loci matrix of dosages d = a + b in {0, 1, 2}; the mean genotypes are X = D / 2
and the predictors are Z = [env, lat, long].  Nothing here sees D: the fit needs only
    C = D^T D (exact integers), s = D^T 1, D^T Z, Z^T Z, Z^T 1
(gnx_geno_locus_gram, gnx_geno_locus_cross), from which Sxx = X^T X, Sxy = X^T Y and
Syy = Y^T Y of the centred and scaled blocks follow; every quantity sklearn computes from the
N-row blocks (pseudo-inverses, scores' inner products, loadings, deflation) is a function of
these three.  The individuals' scores are one N x 3 product with D (gnx_geno_matmul), passed
in as a callable so that the CPU tests can hand in a numpy one.  Pure functions, fp64.
"""
import warnings

import numpy as np

N_COMPONENTS = 3        # the reference fits 3 components to its 3 predictors
MAX_ITER = 500          # sklearn's CCA(max_iter=500)
TOL = 1e-6              # sklearn's CCA(tol=1e-06), on |xw - xw_prev|^2
EPS = np.finfo(np.float64).eps


class DegenerateGEAWarning(UserWarning):
    """N <= n_loci + 3: every canonical correlation is 1 and the answer is a matter of the
    pseudo-inverse's cutoff (sklearn's own, too)"""


class GEAConvergenceWarning(UserWarning):
    """the power iteration of a component stopped at MAX_ITER (sklearn: ConvergenceWarning)"""


# Eigenvalues of a cross-product matrix at or below PINV_CUTOFF x the largest are treated as
# zero by sym_pinv.  sklearn drops singular values of the N-row block at or below 1e6 eps x the
# largest, which catches the exactly dependent columns (a monomorphic locus, two identical
# loci) because the SVD leaves them at ~eps.  In the squared (Gram) domain those directions
# come out of eigh at ~eps x the largest EIGENvalue, so the same number is used on the
# eigenvalues: 1e6 eps ~ 2.2e-10, six decades above eigh's noise.  A direction whose
# eigenvalue ratio lies between (1e6 eps)^2 and 1e6 eps is kept by sklearn and dropped here;
# `min_kept_ratio` in the result says how far the data are from that band.
PINV_CUTOFF = 1e6 * EPS


def sym_pinv(S):
    """pseudo-inverse of a symmetric positive semi-definite matrix by eigh
    -> (S^+, smallest kept eigenvalue / largest eigenvalue)"""
    lam, U = np.linalg.eigh((S + S.T) * 0.5)
    top = lam[-1]
    if not top > 0:
        return np.zeros_like(S), np.inf
    keep = lam > PINV_CUTOFF * top
    Uk = U[:, keep]
    return (Uk / lam[keep]) @ Uk.T, float(lam[keep].min() / top)


def scaled_cross_products(C, s, DtZ, ZtZ, Zt1, N):
    """Sxx, Sxy, Syy of the centred, unit-variance (ddof=1) blocks X = D / 2 and Y = Z, with
    sklearn's rule that a zero standard deviation is replaced by 1 (_center_scale_xy).
    The integer part N C - s s^T is exact in int64 (entries below 4 N^2).
    -> Sxx, Sxy, Syy, x_mean, x_sd, y_mean, y_sd"""
    C = np.asarray(C, np.int64)
    s = np.asarray(s, np.int64)
    N = int(N)
    if N < 2:
        raise ValueError('a CCA needs at least 2 individuals (got %d)' % N)
    if N > 1 << 30:
        raise ValueError('N above 2^30: N C - s s^T would leave int64')
    DtZ = np.asarray(DtZ, np.float64)
    ZtZ = np.asarray(ZtZ, np.float64)
    Zt1 = np.asarray(Zt1, np.float64)
    cxx = (C * N - np.outer(s, s)).astype(np.float64) / (4.0 * N)       # X_c^T X_c
    cxy = 0.5 * (DtZ - np.outer(s.astype(np.float64), Zt1) / N)          # X_c^T Z_c
    cyy = ZtZ - np.outer(Zt1, Zt1) / N                                   # Z_c^T Z_c
    x_sd = np.sqrt(np.maximum(np.diag(cxx), 0.0) / (N - 1))
    y_sd = np.sqrt(np.maximum(np.diag(cyy), 0.0) / (N - 1))
    x_sd[x_sd == 0.0] = 1.0
    y_sd[y_sd == 0.0] = 1.0
    return (cxx / np.outer(x_sd, x_sd), cxy / np.outer(x_sd, y_sd), cyy / np.outer(y_sd, y_sd),
            s / (2.0 * N), x_sd, Zt1 / N, y_sd)


def cca_from_cross_products(C, s, DtZ, ZtZ, Zt1, N, matmul):
    """sklearn's CCA(n_components=3).fit(X, Z) and .transform(X), X = D / 2, from the
    cross-products of D (n_loci columns) and Z (3 columns) over N individuals.

    matmul(M [n_loci][3] fp64) -> D M [N][3] supplies the scores.  Warns
    (DegenerateGEAWarning) when N <= n_loci + 3 and (GEAConvergenceWarning) when a
    component's iteration hits MAX_ITER.
    -> dict(ind_df [N][3] = x scores, loci_df [n_loci][3] = x_loadings_, var_df [3][3] =
       y_loadings_, n_iter [3], min_kept_ratio = the smallest eigenvalue ratio any
       pseudo-inverse kept)"""
    Sxx, Sxy, Syy, x_mean, x_sd, _, _ = scaled_cross_products(C, s, DtZ, ZtZ, Zt1, N)
    p, q = Sxy.shape
    if q != N_COMPONENTS:
        raise ValueError('Z must have %d columns, got %d' % (N_COMPONENTS, q))
    if int(N) <= p + q:
        warnings.warn('GEA: %d individuals for %d loci + %d predictors: the CCA is degenerate '
                      '(every canonical correlation is 1; the loadings depend on the '
                      'pseudo-inverse cutoff).  Use fewer loci (loci=...)' % (N, p, q),
                      DegenerateGEAWarning, stacklevel=2)
    W = np.zeros((p, q))
    P = np.zeros((p, q))
    Q = np.zeros((q, q))
    n_iter = np.zeros(q, np.int64)
    min_kept = np.inf
    for k in range(q):
        Sxx_pinv, r1 = sym_pinv(Sxx)
        Syy_pinv, r2 = sym_pinv(Syy)
        min_kept = min(min_kept, r1, r2)
        # y_score = Y c: the first Y column that is not constant (|entry| > eps somewhere;
        # its squared norm is Syy's diagonal)
        live = np.flatnonzero(np.diag(Syy) > EPS)
        if live.size == 0:
            raise ValueError('GEA: the predictors are constant after %d components' % k)
        c = np.zeros(q)
        c[live[0]] = 1.0
        xw_old = None
        for it in range(MAX_ITER):
            xw = Sxx_pinv @ (Sxy @ c)
            xw /= np.sqrt(xw @ xw) + EPS
            yw = Syy_pinv @ (Sxy.T @ xw)
            yw /= np.sqrt(yw @ yw) + EPS
            c = yw / (yw @ yw + EPS)
            if xw_old is not None and (xw - xw_old) @ (xw - xw_old) < TOL:
                break
            xw_old = xw
        n_iter[k] = it + 1
        if it + 1 == MAX_ITER:
            warnings.warn('GEA: component %d: maximum number of iterations reached' % k,
                          GEAConvergenceWarning, stacklevel=2)
        sign = np.sign(xw[np.argmax(np.abs(xw))])       # sklearn's _svd_flip_1d
        xw = xw * sign
        yw = yw * sign
        tt = xw @ Sxx @ xw
        uu = yw @ Syy @ yw
        tu = xw @ Sxy @ yw
        pk = Sxx @ xw / tt
        qk = Syy @ yw / uu
        # X -= t p^T, Y -= u q^T (t = X xw, u = Y yw), in cross-product form
        Sxy = Sxy - np.outer(pk, Sxy.T @ xw) - np.outer(Sxy @ yw, qk) + tu * np.outer(pk, qk)
        Sxx = Sxx - tt * np.outer(pk, pk)
        Syy = Syy - uu * np.outer(qk, qk)
        W[:, k], P[:, k], Q[:, k] = xw, pk, qk
    R = W @ np.linalg.pinv(P.T @ W)                     # x_rotations_
    M = R / (2.0 * x_sd[:, None])
    ind = np.asarray(matmul(M), np.float64) - (x_mean / x_sd) @ R
    return dict(ind_df=ind, loci_df=P, var_df=Q, n_iter=n_iter, min_kept_ratio=min_kept)


def numpy_cross_products(D, Z):
    """the five cross-products of dosages D [N][n_loci] and predictors Z [N][3] in numpy
    -> C int64, s int64, DtZ, ZtZ, Zt1 (fp64)"""
    Di = np.asarray(D).astype(np.int64)
    Df = Di.astype(np.float64)
    Z = np.asarray(Z, np.float64)
    C = np.rint(Df.T @ Df).astype(np.int64)          # integer entries below 2^53: exact
    return C, Di.sum(axis=0), Df.T @ Z, Z.T @ Z, Z.sum(axis=0)
