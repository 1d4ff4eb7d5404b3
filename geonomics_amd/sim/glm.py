"""Per-locus logistic fits (an extension: the reference has no such analysis): L independent
binomial GLMs d_il ~ Binomial(trials = 2, mu_il), logit mu_il = x_i . beta_l, over one small
design X [n][p].  This is the logistic genotype-environment association of Sambada (Joost et al.
2007, Mol. Ecol. 16:3955; Stucki et al. 2017, Mol. Ecol. Resour. 17:1072) - a likelihood-ratio
("G") test and a Wald test per locus, the effect a log-odds per unit of environment - and, with
one covariate x, the sigmoid cline p(x) = 1 / (1 + exp(-4 (x - c) / w)) with centre
c = -beta0 / beta1 and width w = 4 / |beta1|.

Nothing here sees the n x L dosage matrix D.  The log-likelihood of locus l is
    l(beta) = beta . (X^T d_l) - trials * sum_i log(1 + exp(x_i . beta))       (+ a constant),
so the genotypes enter only through X^T D: one call of gnx_assoc_cross (csrc/gnx_assoc.hip) with
Y = X, which also counts s1 = sum d and s2 = sum d^2 for the MAF filter.  What a Newton step
needs beside it,
    s = sum_i log(1 + e^eta_i),   A = sum_i mu_i x_i,   I = sum_i mu_i (1 - mu_i) x_i x_i^T,
is a function of (X, beta_l) alone: gnx_glm_sweep (csrc/gnx_glm.hip) for the fits that are still
active, or numpy_sweep below.  The score is U = X^T d - trials A, the information trials I.
Pure numpy/scipy, fp64; `cross` and `sweep` are callables so that the CPU tests can hand in
numpy ones, and the same driver serves the device and the restatement.
"""
import numpy as np

from . import assoc as _as

TILE = 64               # the unit of a stretch (csrc/gnx_glm.hip, GLM_TI)
P_MAX = 8               # columns of the design one device call takes, the intercept among them


def n_cols(p):
    """the sums per fit: s, A [p] and the upper triangle of I"""
    return 1 + p + p * (p + 1) // 2


def stretch_rule(n):
    """the summation order of gnx_glm_sweep (include/gnx_glm.h): the individuals are cut into
    at most 64 stretches of `stretch` consecutive ones, the last one ragged
    -> (stretch, stretches)"""
    n = int(n)
    tiles = max(1, -(-n // TILE))
    per = -(-tiles // min(tiles, 64))
    return TILE * per, -(-n // (TILE * per))


def numpy_sweep(X, B, dtype=np.float64):
    """gnx_glm_sweep's formulas, vectorised (include/gnx_glm.h): per fit k the sums over the
    individuals of [s, A, I] at the coefficients B[k] over the design X, in `dtype`
    (np.longdouble: the tests' reference).  Every number of a fit is computed elementwise and
    summed along its own row, so it depends neither on the other fits nor on m
    -> (sums dtype [m][n_cols(p)], 0.0: the kernel time of a device sweep)"""
    X = np.asarray(X, np.float64).astype(dtype)
    B = np.asarray(B, np.float64).astype(dtype)
    if X.ndim != 2 or B.ndim != 2 or X.shape[1] != B.shape[1]:
        raise ValueError('X [n][p] and B [m][p] (got %s and %s)' % (X.shape, B.shape))
    (n, p), m = X.shape, B.shape[0]
    out = np.zeros((m, n_cols(p)), dtype)
    step = max(1, (1 << 21) // max(n, 1))                    # rows of B at a time: bounded memory
    zero = np.zeros((), dtype)
    for k0 in range(0, m, step):
        b = B[k0:k0 + step]
        eta = np.zeros((b.shape[0], n), dtype)
        for j in range(p):
            eta = eta + X[None, :, j] * b[:, j, None]
        t = np.exp(-np.abs(eta))
        r = 1 / (1 + t)
        mu = np.where(eta >= 0, r, t * r)
        w = t * r * r
        o = out[k0:k0 + step]
        o[:, 0] = (np.maximum(eta, zero) + np.log1p(t)).sum(axis=1)
        q = 1 + p
        for j in range(p):
            o[:, 1 + j] = (mu * X[None, :, j]).sum(axis=1)
            wx = w * X[None, :, j]
            for c in range(j, p):
                o[:, q] = (wx * X[None, :, c]).sum(axis=1)
                q += 1
    return out, 0.0


def unpack(sums, p):
    """the sums of a sweep as (s [m], A [m][p], I [m][p][p] symmetric)"""
    sums = np.asarray(sums)
    if sums.ndim != 2 or sums.shape[1] != n_cols(p):
        raise ValueError('sums: %s, not [m][%d] for p = %d' % (sums.shape, n_cols(p), p))
    I = np.zeros((sums.shape[0], p, p), sums.dtype)
    iu = np.triu_indices(p)
    I[:, iu[0], iu[1]] = sums[:, 1 + p:]
    I[:, iu[1], iu[0]] = sums[:, 1 + p:]
    return sums[:, 0], sums[:, 1:1 + p], I


def _positive_definite(I):
    """which of the symmetric matrices I [m][p][p] are finite and positive definite to working
    precision: the smallest eigenvalue above p eps x the largest"""
    ok = np.isfinite(I).all(axis=(1, 2))
    if ok.any():
        ev = np.linalg.eigvalsh(I[ok])
        ok[ok] = ev[:, 0] > I.shape[1] * np.finfo(np.float64).eps * ev[:, -1]
    return ok


def fit(sweep, X, XtD, trials=2, tol=1e-8, max_iter=25, max_halvings=10):
    """m binomial GLMs with the logit link by Newton's method, batched over the active fits:
    X [n][p] the design, XtD [m][p] = X^T d_k per fit, sweep(X, B) -> (sums, kernel_ms) is
    Device.glm_sweep or numpy_sweep.  Every fit starts at beta = 0; a step is I^-1 U with
    U = XtD - trials A; the log-likelihood is l = beta . XtD - trials s.  A step that lowers l
    (by more than 64 eps max(1, |l|): the rounding of l itself is no descent) is halved, at most
    max_halvings times, and a fit whose step still lowers l then stops where it was.  A fit has
    converged when max |step| <= tol max(1, max |beta|) and leaves the batch; one whose
    information matrix is singular or not positive definite at any step stops there.  A fit that
    has not converged after max_iter steps (separation: its maximum is at infinity) is reported
    as such, never raised
    -> dict(beta [m][p], cov [m][p][p] = (trials I)^-1 at the last beta (NaN where that is not
    positive definite), loglik [m], converged bool [m], n_iter [m], n_sweeps, kernel_ms)"""
    X = np.ascontiguousarray(X, np.float64)
    XtD = np.ascontiguousarray(XtD, np.float64)
    if X.ndim != 2 or XtD.ndim != 2 or XtD.shape[1] != X.shape[1]:
        raise ValueError('X [n][p] and XtD [m][p] (got %s and %s)' % (X.shape, XtD.shape))
    m, p = XtD.shape
    trials = float(trials)
    eps = np.finfo(np.float64).eps
    beta = np.zeros((m, p))
    info = np.full((m, p, p), np.nan)
    A = np.zeros((m, p))
    ll = np.full(m, np.nan)
    converged = np.zeros(m, bool)
    n_iter = np.zeros(m, np.int64)
    count = dict(n_sweeps=0, kernel_ms=0.0)

    def lowered(l_new, l_old):
        """the step lowered the log-likelihood (a NaN counts as lower)"""
        return ~(l_new >= l_old - 64 * eps * np.maximum(1.0, np.abs(l_old)))

    def evaluate(idx, B):
        """(l, A, I) of the fits idx at the coefficients B"""
        sums, ms = sweep(X, B)
        count['n_sweeps'] += 1
        count['kernel_ms'] += float(ms)
        s, a, i = unpack(np.asarray(sums, np.float64), p)
        return (B * XtD[idx]).sum(axis=1) - trials * s, a, i

    active = np.arange(m)
    if m:
        ll[:], A[:], info[:] = evaluate(active, beta)
    for _ in range(int(max_iter)):
        if active.size == 0:
            break
        ok = _positive_definite(info[active])
        active = active[ok]                                  # the others stop where they are
        if active.size == 0:
            break
        step = np.linalg.solve(trials * info[active],
                               (XtD[active] - trials * A[active])[:, :, None])[:, :, 0]
        # the candidates; the fits whose log-likelihood fell are tried again at half the step
        new_b = beta[active] + step
        new_l, new_a, new_i = evaluate(active, new_b)
        low = np.flatnonzero(lowered(new_l, ll[active]))
        for _h in range(int(max_halvings)):
            if low.size == 0:
                break
            step[low] *= 0.5
            new_b[low] = beta[active[low]] + step[low]
            new_l[low], new_a[low], new_i[low] = evaluate(active[low], new_b[low])
            low = low[lowered(new_l[low], ll[active[low]])]
        keep = np.ones(active.size, bool)
        keep[low] = False                                    # still lower: stays at its old beta
        act, step = active[keep], step[keep]
        beta[act], ll[act], A[act], info[act] = new_b[keep], new_l[keep], new_a[keep], new_i[keep]
        n_iter[act] += 1
        done = np.abs(step).max(axis=1) <= tol * np.maximum(1.0, np.abs(beta[act]).max(axis=1))
        converged[act[done]] = True
        active = act[~done]
    cov = np.full((m, p, p), np.nan)
    ok = _positive_definite(info)
    if ok.any():
        cov[ok] = np.linalg.inv(trials * info[ok])
    return dict(beta=beta, cov=cov, loglik=ll, converged=converged, n_iter=n_iter,
                n_sweeps=count['n_sweeps'], kernel_ms=count['kernel_ms'])


def check_columns(n_beside, who='logistic scan'):
    """refuse more columns beside the intercept than one device sweep takes"""
    if n_beside + 1 > P_MAX:
        raise ValueError('%s: %d covariates and tested variables together; a logistic fit takes '
                         'at most %d columns beside the intercept' % (who, n_beside, P_MAX - 1))


def design(X_test, C=None, who='logistic scan'):
    """the design [1 | C | X_test] of a scan with every column but the intercept centred and
    scaled to unit variance (conditioning; the fit is invariant), and the map back: with
    z_j = (x_j - mean_j) / sd_j the caller's coefficients are beta = T b, T upper triangular.
    A column that is constant, or a combination of the intercept and the columns before it, is
    refused by name
    -> dict(Z [n][p], T [p][p], c = the covariates' number, r = the tested variables')"""
    X_test = np.asarray(X_test, np.float64)
    if X_test.ndim == 1:
        X_test = X_test[:, None]
    n, r = X_test.shape
    if r < 1:
        raise ValueError('%s: no variable to test' % who)
    C = np.zeros((n, 0)) if C is None else np.asarray(C, np.float64).reshape(n, -1)
    c = C.shape[1]
    check_columns(c + r, who)
    if not (np.isfinite(X_test).all() and np.isfinite(C).all()):
        raise ValueError('%s: the tested variables and the covariates must be finite' % who)
    raw = np.column_stack([C, X_test])
    names = ['covariate %d' % k for k in range(c)] + ['tested variable %d' % k for k in range(r)]
    mean, sd = raw.mean(axis=0), raw.std(axis=0)
    Q = np.ones((n, 1)) / np.sqrt(n)                         # an orthonormal basis so far
    Z = np.ones((n, 1 + c + r))
    for j in range(c + r):
        col = raw[:, j] - mean[j]
        # constant: what centring leaves is rounding, n eps of the column's size
        if not sd[j] > n * np.finfo(np.float64).eps * max(abs(mean[j]), np.abs(raw[:, j]).max()):
            raise ValueError('%s: the design is rank-deficient: %s is constant' % (who, names[j]))
        z = col / sd[j]
        rest = z
        for _ in range(2):                                   # twice: what rounding left
            rest = rest - Q @ (Q.T @ rest)
        if not rest @ rest > 1e-10 * (z @ z):
            raise ValueError('%s: the design is rank-deficient: %s is a combination of the '
                             'intercept and the columns before it' % (who, names[j]))
        Q = np.column_stack([Q, rest / np.sqrt(rest @ rest)])
        Z[:, 1 + j] = z
    T = np.eye(1 + c + r)
    T[0, 1:] = -mean / sd
    T[np.arange(1, 1 + c + r), np.arange(1, 1 + c + r)] = 1.0 / sd
    return dict(Z=np.ascontiguousarray(Z), T=T, c=c, r=r)


def testable(s1, s2, n, min_maf=0.01):
    """what the integers decide, as scan_stats does: polymorphic (n s2 != s1^2) and
    maf >= min_maf -> (bool [L], maf)"""
    return _as.lmm_testable(s1, s2, n, min_maf)


def scan(cross, sweep, n, X_test, C=None, min_maf=0.01, tol=1e-8, max_iter=25, calibrate=False,
         who='logistic scan'):
    """one logistic scan over every locus: cross(Y [n][p]) -> dict(DtY, s1, s2, kernel_ms) as
    sim/assoc.scan's (Device.assoc_cross bound to the sample, or assoc.numpy_cross(D)), sweep as
    fit's.  X_test [n][r] the tested variables, C [n][c] the covariates (None: none); the full
    model [1, C, X_test] is tested against the null model [1, C] per locus by the likelihood
    ratio lrt = 2 (l_full - l_null) on r degrees of freedom, each tested column by Wald.  Loci
    that are monomorphic or below min_maf (decided on the integers s1, s2) are not fitted and
    come back NaN.  calibrate: p from lrt / gif.  Coefficients, standard errors and covariances
    are in the caller's units
    -> dict(beta, se, z, p_wald [L][r]; lrt, p, q, maf, tested, converged, n_iter [L]; gif (the
    median of lrt over the median of chi-square with r df), df = r; coef [L][p], cov [L][p][p]
    of the full model in the design's order [1, C, X_test], loglik, loglik_null [L]; kernel_ms
    (cross and sweeps), n_sweeps)"""
    from scipy.stats import chi2, norm
    n = int(n)
    if n > 1 << 30:
        raise ValueError('n above 2^30: n s2 - s1^2 would leave int64')
    dsn = design(X_test, C, who)
    Z, T, c, r = dsn['Z'], dsn['T'], dsn['c'], dsn['r']
    if Z.shape[0] != n:
        raise ValueError('%s: the design has %d rows, not n = %d' % (who, Z.shape[0], n))
    p = 1 + c + r
    got = cross(Z)
    XtD = np.asarray(got['DtY'], np.float64)
    L = XtD.shape[0]
    tested, maf = testable(got['s1'], got['s2'], n, min_maf)
    idx = np.flatnonzero(tested)
    full = fit(sweep, Z, XtD[idx], 2, tol, max_iter)
    null = fit(sweep, Z[:, :1 + c], XtD[idx][:, :1 + c], 2, tol, max_iter)

    def spread(a, fill=np.nan, dtype=np.float64):
        out = np.full((L,) + a.shape[1:], fill, dtype)
        out[idx] = a
        return out

    coef = full['beta'] @ T.T
    cov = T[None, :, :] @ full['cov'] @ T.T[None, :, :]
    beta = coef[:, 1 + c:]
    with np.errstate(all='ignore'):
        se = np.sqrt(np.diagonal(cov, axis1=1, axis2=2)[:, 1 + c:])
        z = beta / se
        lrt = 2.0 * (full['loglik'] - null['loglik'])
    lrt_all = spread(lrt)
    gif = float('nan')
    if np.isfinite(lrt_all).any():
        # assoc.genomic_inflation squares its argument and divides by the median of chi2_1
        gif = float(_as.genomic_inflation(np.sqrt(np.maximum(lrt_all, 0.0)))
                    * chi2.ppf(0.5, 1) / chi2.ppf(0.5, r))
    pv = chi2.sf(np.maximum(lrt_all, 0.0) / (gif if calibrate else 1.0), r)
    return dict(beta=spread(beta), se=spread(se), z=spread(z),
                p_wald=spread(2.0 * norm.sf(np.abs(z))), lrt=lrt_all, p=pv,
                q=_as.bh_qvalues(pv), maf=maf, tested=tested,
                converged=spread(full['converged'] & null['converged'], False, bool),
                n_iter=spread(full['n_iter'], 0, np.int64), gif=gif, df=r,
                coef=spread(coef), cov=spread(cov), loglik=spread(full['loglik']),
                loglik_null=spread(null['loglik']),
                kernel_ms=float(got.get('kernel_ms', 0.0)) + full['kernel_ms'] + null['kernel_ms'],
                n_sweeps=full['n_sweeps'] + null['n_sweeps'])


def cline_stats(beta, cov, lo, hi):
    """the sigmoid cline p(x) = 1 / (1 + exp(-(beta0 + beta1 x))) of each locus: beta [L][2] =
    (beta0, beta1), cov [L][2][2] their covariance, [lo, hi] the range of x that was sampled
    -> dict(centre = -beta0 / beta1, width = 4 / |beta1| (the inverse of the steepest slope),
    se_centre, se_width (delta method: the gradients (-1 / beta1, beta0 / beta1^2) and
    4 / beta1^2), in_range = lo <= centre <= hi, delta_p = p(hi) - p(lo), slope_sign)"""
    beta = np.asarray(beta, np.float64)
    cov = np.asarray(cov, np.float64)
    b0, b1 = beta[:, 0], beta[:, 1]
    with np.errstate(all='ignore'):
        centre = -b0 / b1
        width = 4.0 / np.abs(b1)
        g0, g1 = -1.0 / b1, b0 / (b1 * b1)
        var_c = g0 * g0 * cov[:, 0, 0] + 2.0 * g0 * g1 * cov[:, 0, 1] + g1 * g1 * cov[:, 1, 1]
        se_centre = np.sqrt(var_c)
        se_width = 4.0 / (b1 * b1) * np.sqrt(cov[:, 1, 1])
        delta_p = _expit(b0 + b1 * hi) - _expit(b0 + b1 * lo)
        in_range = (centre >= lo) & (centre <= hi)
    return dict(centre=centre, width=width, se_centre=se_centre, se_width=se_width,
                in_range=in_range, delta_p=delta_p, slope_sign=np.sign(b1))


def _expit(eta):
    t = np.exp(-np.abs(eta))
    return np.where(eta >= 0, 1.0 / (1.0 + t), t / (1.0 + t))


def concordance(centre, width, use):
    """the summary of the concordance question: the median and the median absolute deviation
    of centre and width over the loci in `use` (NaN when there are none), and their number"""
    use = np.asarray(use, bool)
    out = dict(n_loci=int(use.sum()))
    for name, a in (('centre', centre), ('width', width)):
        a = np.asarray(a, np.float64)[use]
        med = float(np.median(a)) if a.size else float('nan')
        out['median_' + name] = med
        out['mad_' + name] = float(np.median(np.abs(a - med))) if a.size else float('nan')
    return out
