"""Windowed linkage disequilibrium (csrc/gnx_ldwin.hip, gnx_ld_window): LD pruning, clumping of
association hits, LD scores and LD-score regression.  Pure numpy: the device gives, for every
locus, the number of kept loci inside a window around it and the sum of its r^2 with them, and
the list of the in-window pairs whose r^2 reaches a threshold; what is computed here is the
greedy choice of independent loci on that list, the scores and weights from the two per-locus
arrays, the regression of association statistics on the scores, and `brute_window`, a numpy
restatement of the whole entry point over every pair, which the tests compare the device with.

Pruning and clumping are the same step (PLINK's --indep-pairwise and --clump): visit the loci
in a given order - by minor-allele count, or by p-value - keep a locus that no kept locus has
claimed, and let it claim every later neighbour.  The result is the one maximal independent set
that order defines, whatever the order of the edge list.

LD scores (Bulik-Sullivan et al. 2015): l_j = 1 + sum_k r2_adj(j, k) over the window with
r2_adj = r2 - (1 - r2) / (N - 2), N the sampled chromosomes: l_j = 1 + S_j - (m_j - S_j) /
(N - 2) from the device's sum S_j and count m_j.  Under a polygenic model E[chi2_j] = a + (n h2 /
M) l_j with a = 1 without confounding, so structure that inflates every locus alike moves the
intercept and polygenic signal the slope.
"""
import math

import numpy as np

from . import ld as _ld


def check_window(window, unit, who='window'):
    """the window as the device takes it: 'loci' and 'morgans' as given, 'c' (a recombination
    fraction in 0..0.5; 0.5 and above: every pair) as the map distance that gives it"""
    if unit not in ('c', 'morgans', 'loci'):
        raise ValueError("%s: unit: 'c', 'morgans' or 'loci', not %r" % (who, unit))
    try:
        w = float(window)
    except (TypeError, ValueError):
        w = float('nan')
    if isinstance(window, bool) or math.isnan(w) or w < 0:
        raise ValueError('%s: window: a distance >= 0 in %s (got %r)' % (who, unit, window))
    return float(_ld.c_to_morgans(w)) if unit == 'c' else w


def check_r2(r2, who='r2'):
    if isinstance(r2, bool) or not 0.0 <= float(r2) <= 1.0:
        raise ValueError('%s: r2: a threshold in 0..1 (got %r)' % (who, r2))
    return float(r2)


def brute_window(bits, pos, window, min_minor=1, r2_min=0.0):
    """gnx_ld_window restated over every pair (include/gnx_ldwin.h): bits [n_chrom][n_loci] of
    0 / 1, the columns in the order of the request; pos [n_loci] non-decreasing.  The terms are
    computed as the device computes them (integers, then three IEEE roundings for r^2) and every
    score is the correctly rounded sum of its terms (math.fsum).
    -> dict(c1, kept (bool [n_loci]), partners int64, score [n_loci], ei, ej, er2 (the pairs with
    r2 >= r2_min, sorted by (ei, ej)), r2 [n_loci][n_loci] (NaN outside the kept pairs i < j),
    in_window (bool [n_loci][n_loci], i < j kept and within the window))"""
    H = np.asarray(bits).astype(np.int64)
    n, L = H.shape
    pos = np.asarray(pos, dtype=np.float64)
    c1 = H.sum(axis=0)
    kept = np.minimum(c1, n - c1) >= max(1, int(min_minor))
    C = H.T @ H
    i, j = np.triu_indices(L, 1)
    ok = kept[i] & kept[j]
    i, j = i[ok], j[ok]
    dn = (n * C[i, j] - c1[i] * c1[j]).astype(np.float64)
    r2 = (dn * dn) / ((c1[i] * (n - c1[i])).astype(np.float64) *
                      (c1[j] * (n - c1[j])).astype(np.float64))
    full = np.full((L, L), np.nan)
    full[i, j] = r2
    near = (pos[j] - pos[i]) <= float(window)
    inw = np.zeros((L, L), bool)
    inw[i[near], j[near]] = True
    i, j, r2 = i[near], j[near], r2[near]
    partners = np.bincount(i, minlength=L) + np.bincount(j, minlength=L)
    terms = [[] for _ in range(L)]
    for a, b, v in zip(i.tolist(), j.tolist(), r2.tolist()):
        terms[a].append(v)
        terms[b].append(v)
    score = np.array([math.fsum(t) for t in terms], dtype=np.float64).reshape(L)
    e = r2 >= float(r2_min)                  # (triu_indices is already sorted by (i, j))
    return dict(c1=c1, kept=kept, partners=partners.astype(np.int64), score=score,
                ei=i[e].astype(np.int32), ej=j[e].astype(np.int32), er2=r2[e], r2=full,
                in_window=inw)


def greedy_independent(n_loci, ei, ej, rank):
    """the loci no two of which share an edge, chosen greedily: the loci are visited in ascending
    `rank` (distinct values [n_loci]); a locus not yet removed is kept, and every neighbour of
    later rank not yet removed is removed and claimed by it.  Unique given the edges and the
    ranks: the order of the edge list does not matter.
    -> (keep bool [n_loci], claimed_by int64 [n_loci]: the kept locus that removed it, or -1)"""
    n_loci = int(n_loci)
    ei = np.asarray(ei, dtype=np.int64).ravel()
    ej = np.asarray(ej, dtype=np.int64).ravel()
    rank = np.asarray(rank).ravel()
    if ei.size != ej.size:
        raise ValueError('greedy_independent: ei and ej differ in length')
    if rank.size != n_loci or np.unique(rank).size != n_loci:
        raise ValueError('greedy_independent: rank: %d distinct values' % n_loci)
    if ei.size and (min(ei.min(), ej.min()) < 0 or max(ei.max(), ej.max()) >= n_loci or
                    (ei == ej).any()):
        raise ValueError('greedy_independent: edges between two different loci in 0..%d'
                         % (n_loci - 1))
    src = np.concatenate([ei, ej])
    dst = np.concatenate([ej, ei])
    by = np.argsort(src, kind='stable')
    dst = dst[by]
    ptr = np.searchsorted(src[by], np.arange(n_loci + 1))
    removed = np.zeros(n_loci, bool)
    claimed = np.full(n_loci, -1, np.int64)
    for v in np.argsort(rank, kind='stable').tolist():
        if removed[v] or ptr[v] == ptr[v + 1]:
            continue
        nb = dst[ptr[v]:ptr[v + 1]]
        nb = nb[~removed[nb] & (rank[nb] > rank[v])]
        removed[nb] = True
        claimed[nb] = v
    return ~removed, claimed


def maf_rank(c1, n_chrom):
    """the visiting order of prune_ld: minor-allele count descending, index ascending on ties"""
    minor = np.minimum(c1, n_chrom - c1)
    order = np.lexsort((np.arange(minor.size), -minor))
    rank = np.empty(minor.size, np.int64)
    rank[order] = np.arange(minor.size)
    return rank


def p_rank(p):
    """the visiting order of clump: p ascending, index ascending on ties"""
    p = np.asarray(p, dtype=np.float64)
    order = np.lexsort((np.arange(p.size), p))
    rank = np.empty(p.size, np.int64)
    rank[order] = np.arange(p.size)
    return rank


def clumps(p, keep, claimed_by, p1):
    """PLINK's rule on the greedy result over the request (p [m]): a kept locus with p <= p1 is
    an index locus and its clump the loci it claimed; a kept locus above p1 is dropped with its
    members -> (index (ascending p), members: a list of ascending index arrays)"""
    p = np.asarray(p, dtype=np.float64)
    idx = np.flatnonzero(keep & (p <= p1))
    idx = idx[np.lexsort((idx, p[idx]))]
    return idx, [np.flatnonzero(claimed_by == v) for v in idx.tolist()]


def ld_scores(partners, score, kept, n_chrom, adjust=True):
    """l_j = 1 + S_j - (m_j - S_j) / (N - 2) (adjust; N > 2) or 1 + S_j; NaN where not kept"""
    S = np.asarray(score, dtype=np.float64)
    m = np.asarray(partners, dtype=np.float64)
    if adjust and n_chrom <= 2:
        raise ValueError('ld_scores: the adjustment needs more than 2 chromosomes')
    out = 1.0 + S - ((m - S) / (n_chrom - 2.0) if adjust else 0.0)
    return np.where(np.asarray(kept, bool), out, np.nan)


def score_weights(ld_score):
    """1 / max(l, 1), 0 where l is NaN: the LD weights of a relationship matrix"""
    l = np.asarray(ld_score, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        w = 1.0 / np.maximum(l, 1.0)
    return np.where(np.isnan(l), 0.0, w)


def _wls(x, y, w):
    """(intercept, slope) of the weighted least squares of y on x, and the 2 x 2 pieces"""
    A = np.array([[w.sum(), (w * x).sum()], [(w * x).sum(), (w * x * x).sum()]])
    b = np.array([(w * y).sum(), (w * x * y).sum()])
    return A, b


def _solve2(A, b):
    # scaled by the diagonal: x may be of any magnitude
    s = 1.0 / np.sqrt(np.diag(A))
    return s * np.linalg.solve(A * np.outer(s, s), b * s)


def ldsc(chi2, ld_score, n, M, n_blocks=200):
    """LD-score regression: chi2 [m] on ld_score [m] over loci in genome order, weighted as LDSC
    weights it - 1 / max(l, 1) for the overcounting of loci in LD and 1 / (2 (a + b l)^2) for
    the variance of a chi-square that grows with its mean, from the fit of the step before,
    starting at a = 1 and b = (mean chi2 - 1) / mean l and iterated twice; n the individuals, M
    the loci the scores were summed over.  Standard errors by the delete-one jackknife over
    min(n_blocks, m) contiguous blocks with the last weights
    -> dict(intercept, slope, h2 (= slope M / n), intercept_se, slope_se, h2_se, ratio
    ((intercept - 1) / (mean chi2 - 1)), mean_chi2, n_loci, n_blocks)"""
    y = np.asarray(chi2, dtype=np.float64).ravel()
    x = np.asarray(ld_score, dtype=np.float64).ravel()
    if y.size != x.size or y.size < 3 or not (np.isfinite(y).all() and np.isfinite(x).all()):
        raise ValueError('ldsc: at least 3 loci with a finite chi2 and LD score each (got %d, %d)'
                         % (y.size, x.size))
    if np.ptp(x) == 0:
        raise ValueError('ldsc: the LD scores are all equal: no slope')
    if isinstance(n_blocks, bool) or int(n_blocks) != n_blocks or n_blocks < 2:
        raise ValueError('ldsc: n_blocks: at least 2 (got %r)' % (n_blocks,))
    if n < 1 or M < 1:
        raise ValueError('ldsc: n individuals and M loci, both >= 1')
    m = y.size
    nb = min(int(n_blocks), m)
    over = 1.0 / np.maximum(x, 1.0)
    a, b = 1.0, max((y.mean() - 1.0) / x.mean(), 0.0)
    for _ in range(3):                       # the starting weights, then two updates
        w = over / (2.0 * np.maximum(a + max(b, 0.0) * x, 1e-6) ** 2)
        A, r = _wls(x, y, w)
        a, b = _solve2(A, r)
    cut = np.linspace(0, m, nb + 1).astype(np.int64)
    est = np.empty((nb, 2))
    for k in range(nb):
        s = slice(cut[k], cut[k + 1])
        Ak, rk = _wls(x[s], y[s], w[s])
        est[k] = _solve2(A - Ak, r - rk)
    pseudo = nb * np.array([a, b]) - (nb - 1) * est
    se = np.sqrt(pseudo.var(axis=0, ddof=1) / nb)
    scale = float(M) / float(n)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = (a - 1.0) / (y.mean() - 1.0)
    return dict(intercept=float(a), slope=float(b), h2=float(b * scale),
                intercept_se=float(se[0]), slope_se=float(se[1]), h2_se=float(se[1] * scale),
                ratio=float(ratio), mean_chi2=float(y.mean()), n_loci=int(m), n_blocks=int(nb))
