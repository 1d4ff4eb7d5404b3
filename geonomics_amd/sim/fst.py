"""Fst between groups of individuals, per-group diversity and the site-frequency spectrum,
as host arithmetic on the per-group locus counts the device takes (gnx_stats_group_counts,
csrc/gnx_group_counts.hip): cnt1 [G][L] 1-alleles over both homologues, cnt_het [G][L]
heterozygotes, n [G] individuals per group.  Pure numpy: no device is needed here.

fst_hsht is the reference's island validation (tests/validation/island/island_test.py:54-115,
calc_Fst_HsHt under calc_Fsts_mod) in the same operation order, so that it reproduces its
values to the last bit; fst_var is its calc_Fst_var (:118-132).  fst_hudson is Hudson's
estimator as Bhatia et al. (2013, Genome Research 23:1514, eq. 10) give it.
"""
import itertools

import numpy as np


def make_groups(ids_sorted, groups):
    """Groups of living individuals -> (names, order, group_start): order indexes ids_sorted,
    grouped, and order[group_start[g]:group_start[g + 1]] are group names[g]'s individuals (in
    ascending id).  groups: a dict name -> iterable of ids (names sorted), or a 1-d integer
    label array aligned with ids_sorted (names 0 .. max label; a negative label leaves the
    individual out).  ValueError: an unknown id, an id in two groups, a label array of the
    wrong length, fewer than one group."""
    ids_sorted = np.asarray(ids_sorted, dtype=np.int64)
    if isinstance(groups, dict):
        if len(groups) < 1:
            raise ValueError('groups: at least one group')
        names = sorted(groups)
        parts, seen = [], np.zeros(ids_sorted.size, bool)
        for name in names:
            ids = np.unique(np.asarray([*groups[name]], dtype=np.int64))
            pos = np.searchsorted(ids_sorted, ids)
            ok = pos < ids_sorted.size
            ok[ok] = ids_sorted[pos[ok]] == ids[ok]
            if not ok.all():
                raise ValueError('groups: individuals not alive in group %r: %s'
                                 % (name, ids[~ok][:10].tolist()))
            if seen[pos].any():
                raise ValueError('groups: individual %d is in two groups'
                                 % int(ids_sorted[pos[seen[pos]][0]]))
            seen[pos] = True
            parts.append(pos)
        sizes = [p.size for p in parts]
        order = np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    else:
        lab = np.asarray(groups)
        if lab.ndim != 1 or lab.dtype.kind not in 'iu':
            raise ValueError('groups: a dict name -> ids or a 1-d integer label array')
        if lab.size != ids_sorted.size:
            raise ValueError('groups: %d labels for %d living individuals'
                             % (lab.size, ids_sorted.size))
        lab = lab.astype(np.int64)
        G = int(lab.max()) + 1 if lab.size else 0
        if G < 1:
            raise ValueError('groups: at least one group (every label is negative)')
        names = [*range(G)]
        keep = np.flatnonzero(lab >= 0)
        order = keep[np.argsort(lab[keep], kind='stable')].astype(np.int64)
        sizes = np.bincount(lab[keep], minlength=G).tolist()
    group_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return names, order, group_start


def _freqs(cnt1, n):
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.asarray(cnt1, dtype=np.float64) / (2 * n)[:, None]


def fst_hsht(cnt1, cnt_het, n, a, b, est_Hs=False, include_zeros=False):
    """per-locus Fst between groups a and b as the reference's calc_Fst_HsHt computes it:
    f = cnt1 / 2n, het = cnt_het / n, Ht = 2 ((f0 + f1) / 2) (1 - (f0 + f1) / 2), Hs = the mean
    of the two observed heterozygosities (est_Hs: f0 (1 - f0) + f1 (1 - f1)),
    Fst = (Ht - Hs) / Ht; NaN where f0 == f1 (0 with include_zeros); an empty group: NaN"""
    cnt1, cnt_het = np.asarray(cnt1), np.asarray(cnt_het)
    L = cnt1.shape[1]
    if n[a] == 0 or n[b] == 0:
        return np.full(L, np.nan)
    f0, f1 = cnt1[a] / (2 * int(n[a])), cnt1[b] / (2 * int(n[b]))
    het0, het1 = cnt_het[a] / int(n[a]), cnt_het[b] / int(n[b])
    Ht = 2 * ((f0 + f1) / 2) * (1 - (f0 + f1) / 2)
    if est_Hs:
        Hs = (f0 * (1 - f0)) + (f1 * (1 - f1))
    else:
        Hs = (het0 + het1) / 2            # np.mean of two: the sum, then the division
    with np.errstate(divide='ignore', invalid='ignore'):
        fst = (Ht - Hs) / Ht
    return np.where(f0 == f1, 0.0 if include_zeros else np.nan, fst)


def fst_var(cnt1, n):
    """var(f) / (mean(f) (1 - mean(f))) per locus over all groups (the reference's
    calc_Fst_var; Hartl & Clark 2007 p. 291), 0 where the denominator is 0"""
    f = _freqs(cnt1, n)
    m = np.mean(f, axis=0)
    den = m * (1 - m)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(den == 0, 0.0, np.var(f, axis=0) / den)


def fst_hudson(cnt1, n, a, b):
    """numerator and denominator per locus of Hudson's Fst (Bhatia et al. 2013, eq. 10) over
    the 2n chromosomes of each group: num = (p1 - p2)^2 - p1 (1 - p1) / (n1 - 1)
    - p2 (1 - p2) / (n2 - 1), den = p1 (1 - p2) + p2 (1 - p1), n1 = 2 n[a], n2 = 2 n[b].
    Per-locus Fst is num / den; over loci take the ratio of the averages."""
    cnt1 = np.asarray(cnt1)
    n1, n2 = 2 * int(n[a]), 2 * int(n[b])
    if n1 < 2 or n2 < 2:
        return np.full(cnt1.shape[1], np.nan), np.full(cnt1.shape[1], np.nan)
    p1, p2 = cnt1[a] / n1, cnt1[b] / n2
    num = (p1 - p2) ** 2 - p1 * (1 - p1) / (n1 - 1) - p2 * (1 - p2) / (n2 - 1)
    den = p1 * (1 - p2) + p2 * (1 - p1)
    return num, den


def tajima_constants(m):
    """(a1, a2, e1, e2) of Tajima (1989) for m chromosomes"""
    i = np.arange(1, m, dtype=np.float64)
    a1, a2 = np.sum(1 / i), np.sum(1 / i ** 2)
    b1 = (m + 1) / (3 * (m - 1))
    b2 = 2 * (m * m + m + 3) / (9 * m * (m - 1))
    c1 = b1 - 1 / a1
    c2 = b2 - (m + 2) / (a1 * m) + a2 / a1 ** 2
    return a1, a2, c1 / a1, c2 / (a1 ** 2 + a2)


def diversity(cnt1, cnt_het, n):
    """per group, over the loci given: n, S (segregating loci), pi (sum over loci of
    c (2n - c) / C(2n, 2): mean pairwise differences), theta_w (S / a1), tajima_d (NaN for
    S = 0 or 2n < 4), Ho (mean observed heterozygosity), He (mean of 2 f (1 - f) 2n / (2n - 1)),
    Fis = 1 - Ho / He  -> dict of arrays [G]"""
    cnt1, cnt_het = np.asarray(cnt1, dtype=np.int64), np.asarray(cnt_het, dtype=np.int64)
    n = np.asarray(n, dtype=np.int64)
    G, L = cnt1.shape
    out = {k: np.full(G, np.nan) for k in ('pi', 'theta_w', 'tajima_d', 'Ho', 'He', 'Fis')}
    out['n'] = n.copy()
    out['S'] = np.zeros(G, np.int64)
    for g in range(G):
        m = 2 * int(n[g])
        if m < 2:
            continue
        c = cnt1[g]
        S = int(np.count_nonzero((c > 0) & (c < m)))
        pi = float(np.sum((c * (m - c)).astype(np.float64) / (m * (m - 1) / 2)))
        a1, a2, e1, e2 = tajima_constants(m)
        out['S'][g], out['pi'][g], out['theta_w'][g] = S, pi, S / a1
        if S > 0 and m >= 4:
            out['tajima_d'][g] = (pi - S / a1) / np.sqrt(e1 * S + e2 * S * (S - 1))
        if L:
            f = c / m
            out['Ho'][g] = np.mean(cnt_het[g] / int(n[g]))
            out['He'][g] = np.mean(2 * f * (1 - f) * m / (m - 1))
            with np.errstate(divide='ignore', invalid='ignore'):
                out['Fis'][g] = 1 - out['Ho'][g] / out['He'][g]
    return out


def sfs(cnt1, n, folded=False):
    """site-frequency spectrum, one row per group: sfs[g][c] = loci with c 1-alleles among the
    2 n[g] chromosomes (folded: with min(c, 2n - c)); rows are 2 max(n) + 1 wide (folded:
    max(n) + 1) and sum to L"""
    cnt1 = np.asarray(cnt1, dtype=np.int64)
    n = np.asarray(n, dtype=np.int64)
    width = int(n.max()) + 1 if folded else 2 * int(n.max()) + 1
    out = np.zeros((cnt1.shape[0], width), np.int64)
    for g in range(cnt1.shape[0]):
        c = np.minimum(cnt1[g], 2 * n[g] - cnt1[g]) if folded else cnt1[g]
        out[g] = np.bincount(c, minlength=width)
    return out


def pairs(names):
    """the pairs of groups, in sorted order (as itertools.combinations of the sorted names)"""
    return [*itertools.combinations(range(len(names)), 2)]


def calc_fst(names, n, cnt1, cnt_het, method='HsHt', mean=True, est_Hs=False,
             include_zeros=False):
    """Species._calc_fst on counts: 'HsHt' and 'hudson' -> {(name_a, name_b): value}, the
    value the nanmean over loci ('hudson': the ratio of the averages) or, mean=False, the
    per-locus array; 'var' -> one array over all groups, or its mean"""
    if method not in ('HsHt', 'hudson', 'var'):
        raise ValueError("method: 'HsHt', 'hudson' or 'var', not %r" % (method,))
    if method == 'var':
        v = fst_var(cnt1, n)
        return float(np.mean(v)) if mean else v
    out = {}
    for a, b in pairs(names):
        if method == 'HsHt':
            v = fst_hsht(cnt1, cnt_het, n, a, b, est_Hs=est_Hs, include_zeros=include_zeros)
            if mean:
                v = float(np.nanmean(v)) if np.isfinite(v).any() else np.nan
        else:
            num, den = fst_hudson(cnt1, n, a, b)
            if mean:
                with np.errstate(divide='ignore', invalid='ignore'):
                    v = float(np.mean(num) / np.mean(den))
            else:
                with np.errstate(divide='ignore', invalid='ignore'):
                    v = num / den
        out[(names[a], names[b])] = v
    return out
