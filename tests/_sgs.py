"""The numpy restatement of gnx_sgs_sums (include/gnx_hip.h) and of what sim/sgs.py makes of its
sums: every pair of the sample brute-forced exactly as the header specifies, and the explicit
per-pair Loiselle kinship with np.polyfit for the slope.  No test in it (tests/test_sgs_host.py
and tests/test_gpu_sgs.py use it)."""
import math

import numpy as np


def pair_geometry(x32, y32, edges):
    """(a, b, r, class) of the pairs a < b: dx, dy the fp64 differences of the fp32
    coordinates, r = sqrt(dx dx + dy dy) (numpy rounds every operation once: no contraction);
    class k when edges[k] <= r < edges[k + 1], -1 for no class, -2 for r == 0"""
    x = np.asarray(x32, np.float32).astype(np.float64)
    y = np.asarray(y32, np.float32).astype(np.float64)
    edges = np.asarray(edges, np.float64)
    a, b = np.triu_indices(x.size, 1)
    dx, dy = x[a] - x[b], y[a] - y[b]
    r = np.sqrt(dx * dx + dy * dy)
    k = np.searchsorted(edges, r, side='right') - 1
    k[(k < 0) | (k >= edges.size - 1)] = -1
    k[r == 0] = -2
    return a, b, r, k


def weights_dot(D, weight):
    """w_a = sum_l weight[l] d_al in fp64, loci ascending, one rounding per locus"""
    w = np.zeros(D.shape[0])
    for l in range(D.shape[1]):
        w = w + weight[l] * D[:, l].astype(np.float64)
    return w


def brute_sums(x32, y32, D, edges, weight=None):
    """isums int64 [K][3], fsums float64 [K][7] (each the correctly rounded sum of its fp64
    terms: math.fsum), n_zero, and absums [K][7] = sum |term|, of dosages D [n][L']"""
    D = np.asarray(D).astype(np.int64)
    edges = np.asarray(edges, np.float64)
    K = edges.size - 1
    a, b, r, k = pair_geometry(x32, y32, edges)
    G = D @ D.T
    self_ = np.diag(G)
    w = weights_dot(D, weight) if weight is not None else np.zeros(D.shape[0])
    isums = np.zeros((K, 3), np.int64)
    fsums = np.zeros((K, 7))
    absums = np.zeros((K, 7))
    for c in range(K):
        s = k == c
        aa, bb, rr = a[s], b[s], r[s]
        dot, ss = G[aa, bb], self_[aa] + self_[bb]
        ww = w[aa] + w[bb]
        with np.errstate(divide='ignore'):
            ln = np.log(rr)
        isums[c] = rr.size, dot.sum(), ss.sum()
        terms = [rr, ln, ln * ln, dot.astype(np.float64) * ln, ss.astype(np.float64) * ln, ww,
                 ww * ln]
        fsums[c] = [math.fsum(t) for t in terms]
        absums[c] = [math.fsum(np.abs(t)) for t in terms]
    return isums, fsums, int((k == -2).sum()), absums


def loiselle(D):
    """the explicit matrix F_ab = sum_l (p_al - pbar_l)(p_bl - pbar_l) / sum_l pbar_l (1 - pbar_l)
    + 1 / (2n - 1), p = d / 2, pbar the sample's mean frequency"""
    p = np.asarray(D, np.float64) / 2.0
    n = p.shape[0]
    pbar = p.mean(axis=0)
    c = p - pbar
    den = (pbar * (1.0 - pbar)).sum()
    with np.errstate(divide='ignore', invalid='ignore'):
        return (c @ c.T) / den + 1.0 / (2.0 * n - 1.0)


def explicit_stats(x32, y32, D, edges, fit_range=None):
    """the statistics of sim/sgs.spatial_structure from the per-pair values themselves"""
    D = np.asarray(D).astype(np.int64)
    edges = np.asarray(edges, np.float64)
    K = edges.size - 1
    a, b, r, k = pair_geometry(x32, y32, edges)
    F = loiselle(D)[a, b]
    Dh = D / 2.0
    d2 = ((Dh[:, None, :] - Dh[None, :, :]) ** 2).sum(axis=2)[a, b]
    out = dict(pairs=np.zeros(K, np.int64), mean_r=np.full(K, np.nan),
               mean_lnr=np.full(K, np.nan), F=np.full(K, np.nan), dist2=np.full(K, np.nan))
    for c in range(K):
        s = k == c
        out['pairs'][c] = s.sum()
        if s.any():
            out['mean_r'][c] = r[s].mean()
            out['mean_lnr'][c] = np.log(r[s]).mean()
            out['F'][c] = F[s].mean()
            out['dist2'][c] = d2[s].mean()
    k0, k1 = (0, K) if fit_range is None else fit_range
    s = (k >= k0) & (k < k1)
    out['slope'] = float(np.polyfit(np.log(r[s]), F[s], 1)[0])
    out['F1'] = float(out['F'][0])
    out['Sp'] = -out['slope'] / (1.0 - out['F1'])
    out['Nb'] = 1.0 / out['Sp'] if out['Sp'] > 0 else np.nan
    return out


def permuted(D, perm):
    """the dosages after the library's permutation: position i holds the genome of perm[i]"""
    return np.asarray(D)[np.asarray(perm)]
