"""Per-locus association scans (an extension: the reference has no such analysis): for every
locus one regression of a phenotype on the dosage (GWAS) or of the dosage on an environmental
variable (GEA), with covariates, genetic PCs or the latent factors of LFMM2 (Caye et al. 2019,
Mol. Biol. Evol. 36:852; `lfmm2` of the R package LEA) against population structure.

Nothing here sees the n x L dosage matrix D.  By the Frisch-Waugh theorem the coefficient of one
variable in a regression with covariates is the simple regression of the two residuals, so a
scan needs, per locus l with dosage column g,
    s1 = sum g, s2 = sum g^2 (exact integers)  and  g . y for a few columns y,
which is one call of gnx_assoc_cross (csrc/gnx_assoc.hip) with Y = [Q | x~_1 .. x~_r]:
    Q    an orthonormal basis of the centred covariates (the intercept is never sent: the centred
         sum of squares of g is the exact integer (n s2 - s1^2) / n),
    x~_k the tested variable k, centred and residualised on Q.
Then g~.g~ = (n s2 - s1^2) / n - sum (Q^T g)^2, the partial correlation r = g.x~ / sqrt(g~.g~
x~.x~), t = r sqrt(df / (1 - r^2)) with df = n - q - 2, and a two-sided p from the t distribution.
Pure numpy/scipy, fp64; `cross` is a callable so that the CPU tests can hand in a numpy one.
"""
import warnings

import numpy as np

M_MAX = 32              # columns of Y one device call takes
GRAM_MAX = 8192         # individuals of the exact Gram matrix behind the latent factors
TILE = 64               # the unit of a stretch (csrc/gnx_assoc.hip, AS_TI)


def stretch_rule(n, L):
    """the summation order of gnx_assoc_cross (include/gnx_hip.h): the individuals are cut into
    stretches of `stretch` consecutive ones, the last one ragged -> (stretch, stretches)"""
    n, L = int(n), int(L)
    lines = (L + 1023) // 1024
    tiles = max(1, -(-n // TILE))
    want = min(tiles, 32, max(1, 2048 // lines))
    per_tiles = -(-tiles // want)
    return TILE * per_tiles, -(-tiles // per_tiles)


def ordered_cross(D, Y):
    """gnx_assoc_cross restated bit for bit: within a stretch the rounded acc + d y over
    ascending individuals from +0 (d y is exact), then the stretches left to right
    -> dict(DtY fp64 [L][m], s1, s2 int64 [L], stretch, stretches)"""
    Di = np.asarray(D).astype(np.int64)
    Y = np.asarray(Y, np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    n, L = Di.shape
    per, cnt = stretch_rule(n, L)
    Df = Di.astype(np.float64)
    tot = None
    for c in range(cnt):
        acc = np.zeros((L, Y.shape[1]))
        for i in range(c * per, min(n, (c + 1) * per)):
            acc += Df[i][:, None] * Y[i][None, :]
        tot = acc if tot is None else tot + acc
    return dict(DtY=tot, s1=Di.sum(axis=0), s2=(Di * Di).sum(axis=0), stretch=per,
                stretches=cnt)


def brute_cross(D, Y):
    """the restatement in extended precision: DtY = D^T Y summed in np.longdouble (where that
    is the x87 format its own error, n 2^-64 abs_sums, is 2^-11 of the fp64 bound
    (n - 1) 2^-53 abs_sums), s1 = sum d, s2 = sum d^2 (int64) and abs_sums = D^T |Y|
    -> (DtY longdouble [L][m], s1, s2, abs_sums longdouble [L][m])"""
    Di = np.asarray(D).astype(np.int64)
    Y = np.asarray(Y, np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    Dl = Di.astype(np.longdouble)
    Yl = Y.astype(np.longdouble)
    DtY = np.zeros((Di.shape[1], Y.shape[1]), np.longdouble)
    ab = np.zeros_like(DtY)
    for j in range(Y.shape[1]):
        DtY[:, j] = (Dl * Yl[:, j][:, None]).sum(axis=0)
        ab[:, j] = (Dl * np.abs(Yl[:, j])[:, None]).sum(axis=0)
    return DtY, Di.sum(axis=0), (Di * Di).sum(axis=0), ab


def numpy_cross(D):
    """cross(Y) of the dosages D [n][L] in plain fp64 numpy, for the host tests"""
    Di = np.asarray(D).astype(np.int64)
    Df = Di.astype(np.float64)
    s1, s2 = Di.sum(axis=0), (Di * Di).sum(axis=0)
    return lambda Y: dict(DtY=Df.T @ np.asarray(Y, np.float64), s1=s1, s2=s2, kernel_ms=0.0)


def check_columns(n_cols, who='assoc'):
    """refuse more columns (covariates and tested variables) than one device call takes"""
    if n_cols > M_MAX:
        raise ValueError('%s: %d covariates and tested variables together; one scan takes at '
                         'most %d columns' % (who, n_cols, M_MAX))


def _orthonormal(A):
    """an orthonormal basis of the columns of A (the directions whose singular value is above
    max(shape) eps x the largest)"""
    if A.shape[1] == 0:
        return A
    U, s, _ = np.linalg.svd(A, full_matrices=False)
    if not s[0] > 0:
        return A[:, :0]
    return U[:, s > max(A.shape) * np.finfo(np.float64).eps * s[0]]


def design(X, C=None, mutual=False):
    """the columns one scan sends: X [n][r] the tested variables, C [n][c] the covariates (None:
    none).  Both are centred; Q is an orthonormal basis of C (of [C | X] with mutual) and x~_k is
    x_k residualised on the covariates of its test: on C, or with mutual on C and the other
    tested variables (LFMM: every layer given the others and the factors)
    -> dict(Y [n][q + r] = [Q | x~], q, xx [r] = x~.x~, n_cov = the covariates' rank, the same
    for every test)"""
    X = np.asarray(X, np.float64)
    if X.ndim == 1:
        X = X[:, None]
    n, r = X.shape
    if r < 1:
        raise ValueError('no variable to test')
    C = np.zeros((n, 0)) if C is None else np.asarray(C, np.float64).reshape(n, -1)
    if not (np.isfinite(X).all() and np.isfinite(C).all()):
        raise ValueError('the tested variables and the covariates must be finite')
    Xc = X - X.mean(axis=0)
    Cc = C - C.mean(axis=0)
    Xt = np.empty_like(Xc)
    if not mutual:
        Q = _orthonormal(Cc)
        n_cov = Q.shape[1]
        for _ in range(2):                       # twice: the second pass removes what rounding left
            Xc = Xc - Q @ (Q.T @ Xc)
        Xt = Xc
    else:
        Q = _orthonormal(np.column_stack([Cc, Xc]))
        n_cov = Q.shape[1] - 1                   # x~_k is not zero (checked below): rank(B) + 1
        for k in range(r):
            B = _orthonormal(np.column_stack([Cc, np.delete(Xc, k, axis=1)]))
            x = Xc[:, k]
            for _ in range(2):
                x = x - B @ (B.T @ x)
            Xt[:, k] = x
    xx = (Xt * Xt).sum(axis=0)
    if not (xx > 0).all():
        raise ValueError('a tested variable is constant or a combination of its covariates')
    return dict(Y=np.ascontiguousarray(np.column_stack([Q, Xt])), q=Q.shape[1], xx=xx,
                n_cov=n_cov, mutual=bool(mutual))


def genomic_inflation(t):
    """the genomic inflation factor: the median of t^2 over the tested loci (the entries that
    are not NaN; per column of a 2-d t) over the median of chi-square with 1 df"""
    from scipy.stats import chi2
    t2 = np.asarray(t, np.float64) ** 2
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)      # a column without a tested locus
        med = np.nanmedian(t2, axis=0)
    return med / chi2.ppf(0.5, 1)


def calibrated_p(t, gif):
    """p of t^2 / GIF against chi-square with 1 df (NaN where t is)"""
    from scipy.stats import chi2
    t = np.asarray(t, np.float64)
    return chi2.sf(t * t / gif, 1)


def bh_qvalues(p):
    """Benjamini-Hochberg q-values of the finite entries of p (NaN stays NaN and does not count
    as a test); a 2-d p is treated column by column"""
    p = np.asarray(p, np.float64)
    if p.ndim == 2:
        return np.column_stack([bh_qvalues(p[:, k]) for k in range(p.shape[1])]) \
            if p.shape[1] else p.copy()
    q = np.full(p.shape, np.nan)
    idx = np.flatnonzero(np.isfinite(p))
    if idx.size == 0:
        return q
    order = idx[np.argsort(p[idx], kind='stable')]
    m = order.size
    adj = p[order] * m / np.arange(1, m + 1)
    q[order] = np.minimum(np.minimum.accumulate(adj[::-1])[::-1], 1.0)
    return q


def scan_stats(DtY, s1, s2, n, dsn, kind='gwas', min_maf=0.01, collinear_tol=1e-8,
               calibrate=False):
    """the statistics of one scan from the device's sums (module docstring): DtY [L][q + r]
    against dsn['Y'], s1, s2 [L].  kind 'gwas': beta = g.x~ / g~.g~ (the tested variable on the
    dosage); 'gea': beta = g.x~ / x~.x~ (the dosage on the tested variable); se = beta / t,
    written as sqrt((1 - r^2) x~.x~ / (df g~.g~)) and its mirror so that t = 0 gives no 0 / 0.
    Not tested (NaN in beta, se, t, p, q; left out of gif and q): monomorphic loci, decided on
    the integers n s2 == s1^2; maf < min_maf; loci collinear with the covariates,
    g~.g~ <= collinear_tol (n s2 - s1^2) / n (a definition, not a measurement).  calibrate:
    p from t^2 / gif against chi-square with 1 df instead of the t distribution
    -> dict(beta, se, t, p, q [L][r], maf [L], tested bool [L], gif [r], df)"""
    from scipy.stats import t as t_dist
    if kind not in ('gwas', 'gea'):
        raise ValueError("kind: 'gwas' or 'gea', not %r" % (kind,))
    n = int(n)
    s1 = np.asarray(s1, np.int64)
    s2 = np.asarray(s2, np.int64)
    if n > 1 << 30:
        raise ValueError('n above 2^30: n s2 - s1^2 would leave int64')
    q, xx = int(dsn['q']), np.asarray(dsn['xx'], np.float64)
    r = xx.size
    df = n - int(dsn['n_cov']) - 2
    if df < 1:
        raise ValueError('%d individuals leave no degrees of freedom beside %d covariates'
                         % (n, dsn['n_cov']))
    DtY = np.asarray(DtY, np.float64)
    # the columns are centred up to rounding; what their sums leave is taken off with the mean
    gy = DtY - np.outer(s1 / float(n), dsn['Y'].sum(axis=0))
    num = n * s2 - s1 * s1                                   # exact
    ssg = num / float(n)
    gx = gy[:, q:]
    proj = (gy[:, :q] ** 2).sum(axis=1)[:, None]
    if dsn['mutual']:
        proj = proj - gx * gx / xx                           # the basis without x~_k
    gg = ssg[:, None] - proj
    frq = s1 / (2.0 * n)
    maf = np.minimum(frq, 1.0 - frq)
    tested = (num != 0) & (maf >= min_maf) & (gg > collinear_tol * ssg[:, None]).all(axis=1)
    with np.errstate(all='ignore'):
        rho = gx / np.sqrt(gg * xx)
        rho = np.clip(rho, -1.0, 1.0)
        t = rho * np.sqrt(df / (1.0 - rho * rho))
        if kind == 'gwas':
            beta = gx / gg
            se = np.sqrt((1.0 - rho * rho) * xx / (df * gg))
        else:
            beta = gx / xx
            se = np.sqrt((1.0 - rho * rho) * gg / (df * xx))
    for a in (beta, se, t):
        a[~tested] = np.nan
    gif = genomic_inflation(t) if tested.any() else np.full(r, np.nan)
    p = calibrated_p(t, gif) if calibrate else 2.0 * t_dist.sf(np.abs(t), df)
    p[~tested] = np.nan
    return dict(beta=beta, se=se, t=t, p=p, q=bh_qvalues(p), maf=maf, tested=tested,
                gif=np.asarray(gif, np.float64).reshape(r), df=df)


def scan(cross, n, X, C=None, kind='gwas', mutual=False, min_maf=0.01, collinear_tol=1e-8,
         calibrate=False):
    """one association scan over every locus: cross(Y [n][m]) -> dict(DtY, s1, s2, kernel_ms)
    is the device call (Device.assoc_cross bound to the sample) or numpy_cross(D)
    -> scan_stats' dict and kernel_ms"""
    dsn = design(X, C, mutual)
    check_columns(dsn['Y'].shape[1])
    got = cross(dsn['Y'])
    out = scan_stats(got['DtY'], got['s1'], got['s2'], n, dsn, kind, min_maf, collinear_tol,
                     calibrate)
    out['kernel_ms'] = float(got.get('kernel_ms', 0.0))
    return out


def lfmm_weights(X, lam=1e-5):
    """the ridge weights of LFMM2: X centred, its full SVD X = Q_x S R^T, and
    d_i = sqrt(lam / (lam + S_i^2)) for the first rank(X) entries, 1 elsewhere -> (Q_x [n][n], d)"""
    X = np.asarray(X, np.float64)
    if X.ndim == 1:
        X = X[:, None]
    if not lam > 0:
        raise ValueError('lam: a positive ridge penalty (got %r)' % (lam,))
    Xc = X - X.mean(axis=0)
    Qx, S, _ = np.linalg.svd(Xc, full_matrices=True)
    rank = int((S > max(Xc.shape) * np.finfo(np.float64).eps * S[0]).sum()) if S.size and \
        S[0] > 0 else 0
    d = np.ones(Xc.shape[0])
    d[:rank] = np.sqrt(lam / (lam + S[:rank] ** 2))
    return Qx, d


def latent_factors(G, X, K, lam=1e-5):
    """the K latent factors of the LFMM2 ridge estimate from the exact Gram matrix G = D D^T
    (gnx_geno_gram): with H the centring matrix, the top-K eigenvectors u of
    diag(d) Q_x^T (H G H) Q_x diag(d) and U = Q_x diag(1 / d) u (lfmm_weights) -> U [n][K]"""
    G = np.asarray(G, np.float64)
    n = G.shape[0]
    K = int(K)
    if K < 0 or K >= n:
        raise ValueError('K: 0..n-1 latent factors (got %d for %d individuals)' % (K, n))
    if K == 0:
        return np.zeros((n, 0))
    Qx, d = lfmm_weights(X, lam)
    Gc = G - G.mean(axis=0)[None, :]
    Gc = Gc - Gc.mean(axis=1)[:, None]                       # H G H
    P = Qx * d[None, :]                                      # Q_x diag(d)
    M = P.T @ Gc @ P
    w, V = np.linalg.eigh((M + M.T) * 0.5)
    u = V[:, ::-1][:, :K]
    return (Qx / d[None, :]) @ u


# ---- the mixed-model scan (csrc/gnx_quad.hip) ---------------------------------------------------
# y = X b + g beta + u + e, u ~ N(0, sg2 G), e ~ N(0, se2 I): with G = U diag(lambda) U^T and
# delta = se2 / sg2 the rotation M = diag((lambda + delta)^-1/2) U^T whitens the model
# (M^T M = (G + delta I)^-1), and the scan is the Frisch-Waugh scan above on M y, M X and M g.
# The n x L matrix M D is never formed: per locus the test needs ||M z||^2, z the centred dosage
# (the whitened intercept M 1 is a covariate, so centring changes nothing but the size of the
# numbers), which is gnx_assoc_quad, and z . (M^T c) for a few whitened columns c, which is
# gnx_assoc_cross.  delta is fixed at the null model's REML estimate and sigma^2 is re-estimated
# per locus in closed form: the test of EMMAX (Kang et al. 2010, Nat. Genet. 42:348), P3D (Zhang
# et al. 2010) and FaST-LMM with a fixed delta (Lippert et al. 2011).  delta is not refitted per
# locus (exact GEMMA).

def numpy_quad(D):
    """quad(val [L][3], M [m][n], use bool [L]) of the dosages D [n][L] in plain fp64 numpy, for
    the host tests: q[l] = sum_k (sum_i M[k][i] val[l][d_il])^2 at the loci in use, 0 elsewhere"""
    Di = np.asarray(D).astype(np.int64)

    def quad(val, M, use=None):
        val = np.asarray(val, np.float64)
        Z = np.take_along_axis(val.T, Di, axis=0)
        q = ((np.asarray(M, np.float64) @ Z) ** 2).sum(axis=0)
        if use is not None:
            q[~np.asarray(use, bool)] = 0.0
        return dict(q=q, kernel_ms=0.0)
    return quad


def lmm_rotation(evals, U, delta):
    """M fp64 [n][n] = diag((max(lambda, 0) + delta)^-1/2) U^T of G = U diag(lambda) U^T:
    M^T M = (G + delta I)^-1"""
    delta = float(delta)
    if not (np.isfinite(delta) and delta > 0):
        raise ValueError('delta: a positive, finite ratio se2 / sg2 (got %r)' % (delta,))
    lam = np.maximum(np.asarray(evals, np.float64).ravel(), 0.0)
    U = np.asarray(U, np.float64)
    if U.shape != (lam.size, lam.size):
        raise ValueError('evals [n] and U [n][n] (got %s and %s)' % (lam.shape, U.shape))
    # (in C order: U.T / ... would come back in U.T's Fortran order, and the device call would
    # then copy all of it again, strided)
    M = np.empty_like(U)
    np.divide(U.T, np.sqrt(lam + delta)[:, None], out=M)
    return M


def lmm_design(y, X, M):
    """the columns one mixed-model scan sends to gnx_assoc_cross: y [n] the response, X [n][c]
    the covariates WITH the intercept column (the whitened intercept M 1 is not constant, so it
    travels as a covariate), M [n][n] the rotation.  y* = M y, Q* an orthonormal basis of M X,
    y~* = y* residualised on Q* (twice, as design), and A = M^T [Q* | y~*], so that for a dosage
    column g  (M g) . Q*_j = g . A_j
    -> dict(A [n][rank + 1], rank = the rank of M X, xx = y~* . y~*)"""
    y = np.asarray(y, np.float64)
    M = np.asarray(M, np.float64)
    n = M.shape[1]
    if y.shape != (n,):
        raise ValueError('lmm_design: one response y [n = %d] (got %s)' % (n, y.shape))
    X = np.asarray(X, np.float64).reshape(n, -1)
    if not (np.isfinite(y).all() and np.isfinite(X).all()):
        raise ValueError('the response and the covariates must be finite')
    ys = M @ y
    Q = _orthonormal(M @ X)
    yt = ys
    for _ in range(2):
        yt = yt - Q @ (Q.T @ yt)
    xx = float(yt @ yt)
    # what two passes leave of a response inside the span is rounding: (n eps)^2 of y* . y*
    if not xx > (n * np.finfo(np.float64).eps) ** 2 * float(ys @ ys):
        raise ValueError('the response is constant or a combination of the covariates')
    return dict(A=np.ascontiguousarray(M.T @ np.column_stack([Q, yt])), rank=int(Q.shape[1]),
                xx=xx)


def lmm_centre(s1, n):
    """the centre of a locus' dosages: the mean s1 / n rounded to a multiple of 2^-20, so that
    {0, 1, 2} - centre is exact in fp32 (21 bits) and the table of gnx_assoc_quad and the fp64
    terms of lmm_scan_stats speak of the same z.  Any centre gives the same test (the whitened
    intercept is a covariate); the mean keeps the numbers, and so the fp32 error of q, small"""
    return np.rint(np.asarray(s1, np.float64) / float(n) * 2.0 ** 20) / 2.0 ** 20


def lmm_table(s1, n, use=None):
    """the centred table of gnx_assoc_quad: val[l] = {0, 1, 2} - lmm_centre(s1_l, n) in fp32,
    without rounding; zero for the loci that are not to be tested (use bool [L]; None: all)"""
    val = (np.arange(3.0)[None, :] - lmm_centre(s1, n)[:, None]).astype(np.float32)
    if use is not None:
        val[~np.asarray(use, bool)] = 0.0
    return val


def lmm_testable(s1, s2, n, min_maf=0.01):
    """what the integers decide: polymorphic (n s2 != s1^2) and maf >= min_maf -> (bool [L], maf)"""
    s1 = np.asarray(s1, np.int64)
    s2 = np.asarray(s2, np.int64)
    frq = s1 / (2.0 * int(n))
    maf = np.minimum(frq, 1.0 - frq)
    return (int(n) * s2 - s1 * s1 != 0) & (maf >= min_maf), maf


def lmm_scan_stats(q, DtY, s1, s2, n, dsn, min_maf=0.01, collinear_tol=1e-8, calibrate=False):
    """the statistics of one mixed-model scan at a fixed delta from the device's sums: q [L] =
    ||M z||^2 of the centred dosages z = g - lmm_centre(s1, n) (gnx_assoc_quad), DtY [L][rank + 1]
    = D^T A against dsn = lmm_design's dict, s1, s2 [L].  z . A_j = DtY_lj - centre_l sum A_j;
    gg = q - sum over the covariate columns of (z . A_j)^2; gx = z . A_y; the partial correlation
    rho = gx / sqrt(gg xx), t = rho sqrt(df / (1 - rho^2)) with df = n - rank - 1,
    beta = gx / gg (the response on the dosage; sigma^2 is re-estimated per locus in closed form,
    delta is not: EMMAX / P3D / FaST-LMM with a fixed delta), se = sqrt((1 - rho^2) xx /
    (df gg)), p from the t distribution (calibrate: from t^2 / gif against chi-square with 1 df)
    and Benjamini-Hochberg q.  Not tested (NaN; left out of gif and q), as scan_stats:
    monomorphic loci, decided on the integers; maf < min_maf; gg <= collinear_tol q
    -> dict(beta, se, t, p, q [L][1], maf, tested [L], gif [1], df)"""
    from scipy.stats import t as t_dist
    n = int(n)
    if n > 1 << 30:
        raise ValueError('n above 2^30: n s2 - s1^2 would leave int64')
    rank, xx = int(dsn['rank']), float(dsn['xx'])
    df = n - rank - 1
    if df < 1:
        raise ValueError('%d individuals leave no degrees of freedom beside %d covariates'
                         % (n, rank))
    qf = np.asarray(q, np.float64)
    ok, maf = lmm_testable(s1, s2, n, min_maf)
    zA = np.asarray(DtY, np.float64) - np.outer(lmm_centre(s1, n), dsn['A'].sum(axis=0))
    gg = qf - (zA[:, :rank] ** 2).sum(axis=1)
    gx = zA[:, rank]
    tested = ok & (gg > collinear_tol * qf)
    with np.errstate(all='ignore'):
        rho = np.clip(gx / np.sqrt(gg * xx), -1.0, 1.0)
        t = rho * np.sqrt(df / (1.0 - rho * rho))
        beta = gx / gg
        se = np.sqrt((1.0 - rho * rho) * xx / (df * gg))
    beta, se, t = beta[:, None], se[:, None], t[:, None]
    for a in (beta, se, t):
        a[~tested] = np.nan
    gif = genomic_inflation(t) if tested.any() else np.full(1, np.nan)
    p = calibrated_p(t, gif) if calibrate else 2.0 * t_dist.sf(np.abs(t), df)
    p[~tested] = np.nan
    return dict(beta=beta, se=se, t=t, p=p, q=bh_qvalues(p), maf=maf, tested=tested,
                gif=np.asarray(gif, np.float64).reshape(1), df=df)


def lmm_scan(cross, quad, n, y, X, M, min_maf=0.01, collinear_tol=1e-8, calibrate=False):
    """one mixed-model scan over every locus at the rotation M (lmm_rotation; rounded to fp32
    by the caller where quad is the device's): cross(Y) as scan's; quad(val, M, use) ->
    dict(q, kernel_ms) is Device.assoc_quad bound to the sample or numpy_quad(D).  The cross
    call runs first: its exact s1, s2 decide the loci quad is asked for and write its table
    -> lmm_scan_stats' dict, kernel_ms (both calls) and seconds (cross, quad)"""
    import time
    dsn = lmm_design(y, X, M)
    check_columns(dsn['A'].shape[1], 'lmm')
    t0 = time.perf_counter()
    got = cross(dsn['A'])
    t1 = time.perf_counter()
    use, _ = lmm_testable(got['s1'], got['s2'], n, min_maf)
    qd = quad(lmm_table(got['s1'], n, use), M, use)
    t2 = time.perf_counter()
    out = lmm_scan_stats(qd['q'], got['DtY'], got['s1'], got['s2'], n, dsn, min_maf,
                         collinear_tol, calibrate)
    out['kernel_ms'] = float(got.get('kernel_ms', 0.0)) + float(qd.get('kernel_ms', 0.0))
    out['seconds'] = dict(cross=t1 - t0, quad=t2 - t1)
    return out
