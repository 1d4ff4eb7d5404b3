"""Fine-scale spatial genetic structure from sums over pairs (csrc/gnx_sgs.hip, gnx_sgs_sums):
mean kinship per distance class, the slope of kinship on ln(distance), the Sp statistic
(Vekemans & Hardy 2004) and Wright's neighbourhood size.  The reference has no such analysis
(its IBD demo, demos/_IBD_IBE.py, ends at MMRR on a sample).

d_al is the dosage (0, 1, 2) of individual a at locus l, n the sample size, s_l = sum_a d_al,
    pbar_l = s_l / 2n,   den = sum_l pbar_l (1 - pbar_l),   c0 = sum_l pbar_l^2.
Loiselle's kinship (Loiselle et al. 1995) as a ratio of sums over the loci is
    F_ab = sum_l (d_al / 2 - pbar_l)(d_bl / 2 - pbar_l) / den + 1 / (2n - 1)
         = (dot_ab / 4 - (w_a + w_b) / 2 + c0) / den + 1 / (2n - 1),
dot_ab = sum_l d_al d_bl and w_a = sum_l pbar_l d_al, so every sum of F, and of F ln r, over the
pairs of a distance class is a combination of the ten sums the device returns per class:
    isums [K][3] = pairs, sum dot, sum (self_a + self_b)           (self_a = sum_l d_al^2)
    fsums [K][7] = sum r, sum ln r, sum ln^2 r, sum dot ln r, sum (self_a + self_b) ln r,
                   sum (w_a + w_b), sum (w_a + w_b) ln r
with locus_weight = pbar.  Nothing here sees a pair.  Pure functions, fp64.
"""
import warnings

import numpy as np


def default_edges(lo, hi, n_classes=10):
    """n_classes distance classes of equal width in ln r from lo to hi -> [n_classes + 1]"""
    if isinstance(n_classes, bool) or int(n_classes) != n_classes or not 1 <= n_classes <= 32:
        raise ValueError('n_classes: 1..32 distance classes (got %r)' % (n_classes,))
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0 < lo < hi):
        raise ValueError('distance classes from %r to %r: need 0 < lo < hi' % (lo, hi))
    e = np.exp(np.linspace(np.log(lo), np.log(hi), int(n_classes) + 1))
    e[0], e[-1] = lo, hi
    return e


def check_edges(edges):
    """edges as the library takes them: float64, 2..33 of them, finite, ascending, >= 0"""
    e = np.asarray(edges, dtype=np.float64).ravel()
    if not 2 <= e.size <= 33:
        raise ValueError('edges: 1..32 distance classes (got %d edges)' % e.size)
    if not np.isfinite(e).all() or e[0] < 0 or (np.diff(e) <= 0).any():
        raise ValueError('edges: finite, ascending distances starting at or above 0')
    return e


def locus_terms(s_l, n):
    """pbar [L'], den, c0 of the sample's locus counts s_l (1-alleles over 2n chromosomes)"""
    pbar = np.asarray(s_l, np.float64) / (2.0 * n)
    return pbar, float((pbar * (1.0 - pbar)).sum()), float((pbar * pbar).sum())


def _kin_sums(isums, fsums, den, c0, n):
    """per class: sum F and sum F ln r over the pairs"""
    I = np.asarray(isums, np.float64)
    S = np.asarray(fsums, np.float64)
    m, corr = I[..., 0], 1.0 / (2.0 * n - 1.0)
    sF = (I[..., 1] / 4.0 - S[..., 5] / 2.0 + c0 * m) / den + corr * m
    sFl = (S[..., 3] / 4.0 - S[..., 6] / 2.0 + c0 * S[..., 1]) / den + corr * S[..., 1]
    return sF, sFl


def _fit_slice(fit_range, K):
    if fit_range is None:
        return slice(0, K)
    try:
        k0, k1 = (int(v) for v in fit_range)
    except (TypeError, ValueError):
        raise ValueError('fit_range: (first class, one past the last class), not %r'
                         % (fit_range,))
    if not 0 <= k0 < k1 <= K:
        raise ValueError('fit_range: classes %d..%d are not among the %d classes' % (k0, k1 - 1, K))
    return slice(k0, k1)


def class_means(isums, fsums, den, c0, n):
    """per class (NaN where a class is empty): pairs, mean r, mean ln r, mean kinship F, and the
    mean squared genetic distance (sum self - 2 sum dot) / pairs / 4 (between mean genotypes)"""
    I = np.asarray(isums, np.int64)
    S = np.asarray(fsums, np.float64)
    m = I[..., 0].astype(np.float64)
    sF, _ = _kin_sums(I, S, den, c0, n)
    with np.errstate(divide='ignore', invalid='ignore'):
        return dict(pairs=I[..., 0].copy(), mean_r=S[..., 0] / m, mean_lnr=S[..., 1] / m,
                    F=sF / m, dist2=(I[..., 2] - 2 * I[..., 1]).astype(np.float64) / m / 4.0)


def slope(isums, fsums, den, c0, n, fit_range=None):
    """the least-squares slope of F on ln r over the PAIRS of the classes in fit_range
    ((first, one past the last); default all), from the sums; NaN without two distinct
    distances.  isums [..., K, 3] and fsums [..., K, 7]: one slope per leading index"""
    I = np.asarray(isums, np.float64)
    S = np.asarray(fsums, np.float64)
    sl = _fit_slice(fit_range, I.shape[-2])
    sF, sFl = _kin_sums(I, S, den, c0, n)
    m = I[..., sl, 0].sum(axis=-1)
    sx, sxx = S[..., sl, 1].sum(axis=-1), S[..., sl, 2].sum(axis=-1)
    sy, sxy = sF[..., sl].sum(axis=-1), sFl[..., sl].sum(axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        cxx = sxx - sx * sx / m
        b = (sxy - sx * sy / m) / cxx
    return np.where((m >= 2) & (cxx > 0), b, np.nan)


def spatial_structure(isums, fsums, s_l, n, fit_range=None, perm_isums=None, perm_fsums=None):
    """everything Model.calc_spatial_structure returns besides the edges, from the observed
    sums, the sample's locus counts s_l and its size n:
    pairs, mean_r, mean_lnr, F, dist2 [K]; slope b; F1 (the first class's mean F);
    Sp = -b / (1 - F1); Nb = 1 / Sp (NaN, with a warning, where Sp <= 0).
    With the sums of nperm permutations (perm_isums [nperm][K][3], perm_fsums [nperm][K][7];
    the genomes permuted over the positions, so pairs and distances stay): perm_slope [nperm],
    p_slope = (1 + #{b_perm <= b}) / (nperm + 1) (one-sided: kinship falling with distance),
    perm_F [nperm][K] and p_F [K], two-sided about the permutations' mean:
    (1 + #{|F_perm - mean F_perm| >= |F - mean F_perm|}) / (nperm + 1), NaN for empty classes.
    den == 0 (no polymorphic locus): every genetic result is NaN, one warning"""
    I = np.asarray(isums, np.int64)
    S = np.asarray(fsums, np.float64)
    if I.ndim != 2 or I.shape[1] != 3 or S.shape != (I.shape[0], 7):
        raise ValueError('isums [K][3] and fsums [K][7]')
    n = int(n)
    if n < 2:
        raise ValueError('spatial structure: at least 2 individuals (got %d)' % n)
    _, den, c0 = locus_terms(s_l, n)
    K = I.shape[0]
    flat = den <= 0.0
    if flat:
        warnings.warn('spatial structure: no polymorphic locus in the sample (the kinship '
                      "estimator's denominator is 0): kinship, slope, Sp and Nb are NaN",
                      stacklevel=2)
        den = np.nan
    out = class_means(I, S, den, c0, n)
    b = float(slope(I, S, den, c0, n, fit_range))
    F1 = float(out['F'][0])
    with np.errstate(divide='ignore', invalid='ignore'):
        Sp = float(-b / (1.0 - F1))
    Nb = np.nan
    if Sp > 0:
        Nb = 1.0 / Sp
    elif not flat and np.isfinite(Sp):
        warnings.warn('spatial structure: Sp = %g <= 0 (kinship does not fall with distance): '
                      'the neighbourhood size is undefined (NaN)' % Sp, stacklevel=2)
    out.update(slope=b, F1=F1, Sp=Sp, Nb=Nb, n=n)
    if perm_isums is not None:
        PI = np.asarray(perm_isums, np.int64)
        PS = np.asarray(perm_fsums, np.float64)
        if PI.ndim != 3 or PI.shape[0] < 1 or PI.shape[1:] != (K, 3) or \
                PS.shape != (PI.shape[0], K, 7):
            raise ValueError('perm_isums [nperm][K][3] and perm_fsums [nperm][K][7], nperm >= 1')
        nperm = PI.shape[0]
        pb = slope(PI, PS, den, c0, n, fit_range)
        pF = class_means(PI, PS, den, c0, n)['F']
        with np.errstate(invalid='ignore'):
            centre = pF.mean(axis=0)
            p_F = (1.0 + (np.abs(pF - centre) >= np.abs(out['F'] - centre)).sum(axis=0)) \
                / (nperm + 1)
            p_F = np.where(np.isfinite(out['F']), p_F, np.nan)
            p_slope = (1.0 + (pb <= b).sum()) / (nperm + 1) if np.isfinite(b) else np.nan
        out.update(nperm=nperm, perm_slope=pb, p_slope=float(p_slope), perm_F=pF, p_F=p_F)
    return out
