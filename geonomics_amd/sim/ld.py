"""Genome-wide linkage disequilibrium from sums over locus pairs (csrc/gnx_ld.hip, gnx_ld_bins):
the decay of r^2 with recombination distance and the LD estimate of the effective population
size.  Pure numpy: the device gives, per bin of the distance between two loci, the number of
pairs and the sums of r^2, r^4, the distance and Weir & Hill's weight; what is computed here is
the map the distances are measured on, the statistics from the sums, and `brute_bins`, a numpy
restatement of the whole entry point over every pair, which the tests compare the device with.

The map.  The simulator switches homologue between loci l - 1 and l with probability r_l,
independently per interval (structs/genome.py, Recombinations: r_0 = 0), so the recombination
fraction between loci i < j is c_ij = (1 - prod_{i < k <= j} (1 - 2 r_k)) / 2 exactly.  With
Haldane's coordinate m_l = -1/2 sum_{k <= l} ln(1 - 2 r_k) that is c_ij = (1 - exp(-2 (m_j -
m_i))) / 2: the device takes one fp64 coordinate per locus.  A rate of 0.5 (a chromosome break;
also the template's default everywhere) would add an infinite distance; it adds BREAK_MORGANS
instead, across which c is 0.5 to the last bit.  (A distance is the difference of two
coordinates: behind k breaks it carries the rounding of 40 k, 7e-15 k Morgans.)

The estimator.  For phase-known gametes under random mating (Weir & Hill 1980, with the
sample term as Waples 2006 uses it), E[r^2] ~ w(c) / N_e + 1 / n with w(c) = ((1 - c)^2 + c^2) /
(2 c (2 - c)) and n the sampled chromosomes; averaged over the pairs of a bin,
N_e = mean w / (mean r^2 - 1 / n).  For unlinked loci w = 1/3: Waples' 1 / (3 (r^2 - 1/n)).
"""
import math
import warnings

import numpy as np

BREAK_MORGANS = 40.0     # exp(-80) = 1.8e-35: c = 0.5 to the last bit


def map_positions(rates):
    """Haldane map coordinate (Morgans) of every locus from the per-locus recombination rates
    (rates[0] = 0; rates[l] between loci l - 1 and l): m_l = -1/2 sum_{k <= l} ln(1 - 2 r_k),
    a rate of 0.5 or more adding BREAK_MORGANS"""
    r = np.asarray(rates, dtype=np.float64).ravel()
    if r.size == 0 or (r < 0).any() or not np.isfinite(r).all():
        raise ValueError('rates: a non-empty list of finite recombination rates >= 0')
    step = np.full(r.size, BREAK_MORGANS)
    ok = r < 0.5
    step[ok] = np.minimum(-0.5 * np.log1p(-2.0 * r[ok]), BREAK_MORGANS)
    step[0] = 0.0
    return np.cumsum(step)


def c_to_morgans(c):
    """map distance at which Haldane's function gives recombination fraction c; c >= 0.5: inf"""
    c = np.asarray(c, dtype=np.float64)
    out = np.full(c.shape, np.inf)
    ok = c < 0.5
    out[ok] = -0.5 * np.log1p(-2.0 * c[ok])
    return out


def morgans_to_c(m):
    return -0.5 * np.expm1(-2.0 * np.asarray(m, dtype=np.float64))


def drift_weight(c):
    """w(c) = ((1 - c)^2 + c^2) / (2 c (2 - c)), evaluated as the device evaluates it; c = 0: inf"""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(divide='ignore'):
        return ((1.0 - c) * (1.0 - c) + c * c) / ((2.0 * c) * (2.0 - c))


def default_edges(unit, n_bins=20, max_dist=None, n_loci=None):
    """'c': [0, 1e-3 ... max_dist (0.5)], 'morgans': [0, 1e-3 ... max_dist (2)], the inner edges
    equally spaced in the logarithm; 'loci': distinct whole separations from 1 to max_dist + 1
    (default min(n_loci - 1, 1000)), about equally spaced in the logarithm"""
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or not 1 <= n_bins <= 64:
        raise ValueError('n_bins: 1..64 bins (got %r)' % (n_bins,))
    n_bins = int(n_bins)
    if unit in ('c', 'morgans'):
        hi = (0.5 if unit == 'c' else 2.0) if max_dist is None else float(max_dist)
        if not 1e-3 < hi < np.inf or (unit == 'c' and hi > 0.5):
            raise ValueError('max_dist: above 0.001%s (got %r)'
                             % (' and at most 0.5' if unit == 'c' else '', max_dist))
        if n_bins == 1:
            return np.array([0.0, hi])
        return np.concatenate([[0.0], np.geomspace(1e-3, hi, n_bins)])
    if unit == 'loci':
        hi = max(1, min((n_loci or 2) - 1, 1000)) if max_dist is None else int(max_dist)
        if hi < 1:
            raise ValueError('max_dist: at least one locus of separation (got %r)' % (max_dist,))
        return np.unique(np.round(np.geomspace(1.0, hi + 1.0, n_bins + 1)))
    raise ValueError("unit: 'c', 'morgans' or 'loci', not %r" % (unit,))


def check_edges(edges):
    e = np.asarray(edges, dtype=np.float64).ravel()
    if not 2 <= e.size <= 65 or np.isnan(e).any() or not np.isfinite(e[:-1]).all() or \
            (np.diff(e) <= 0).any():
        raise ValueError('edges: 2..65 ascending values, finite but for the last (got %r)'
                         % (edges,))
    return e


def min_minor(min_maf, n_chrom):
    """the smallest minor-allele count with frequency >= min_maf among n_chrom chromosomes"""
    if not 0.0 <= float(min_maf) <= 0.5:
        raise ValueError('min_maf: in 0..0.5 (got %r)' % (min_maf,))
    return max(1, int(math.ceil(float(min_maf) * n_chrom - 1e-9)))


def ld_ne(pairs, sum_r2, sum_w, n_chrom):
    """N_e = (sum_w / pairs) / (sum_r2 / pairs - 1 / n_chrom); NaN (with a warning) without
    pairs, inf when the sample's own 1 / n_chrom explains all the r^2 there is (the negative
    estimate LDNe reports as infinite)"""
    if pairs <= 0:
        warnings.warn('ld_ne: no locus pairs to estimate N_e from', RuntimeWarning, stacklevel=2)
        return float('nan')
    drift = float(sum_r2) / pairs - 1.0 / n_chrom
    if drift <= 0:
        return float('inf')
    return (float(sum_w) / pairs) / drift


def decay_stats(pairs, sum_r2, sum_r4, sum_d, sum_w, morgans):
    """per bin: mean r^2, its standard deviation over the pairs, the mean distance, the
    recombination fraction at the mean map distance and the mean drift weight (the last two NaN
    without a map); NaN where a bin is empty"""
    m = np.asarray(pairs, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = np.where(m > 0, sum_r2 / m, np.nan)
        var = np.where(m > 0, sum_r4 / m - mean * mean, np.nan)
        dist = np.where(m > 0, sum_d / m, np.nan)
        w = np.where(m > 0, sum_w / m, np.nan)
    nan = np.full(m.shape, np.nan)
    return dict(mean_r2=mean, sd_r2=np.sqrt(np.maximum(var, 0.0)), mean_dist=dist,
                mean_c=morgans_to_c(dist) if morgans else nan,
                expected_w=w if morgans else nan)


def brute_bins(bits, pos, edges, min_minor=1, morgans=False):
    """gnx_ld_bins restated over every pair (include/gnx_hip.h): bits [n_chrom][n_loci] of 0 / 1,
    the columns in the order of the request; pos [n_loci] non-decreasing; edges ascending.  The
    terms are computed as the device computes them (integers, then three IEEE roundings for
    r^2) and every sum is the correctly rounded sum of its terms (math.fsum).
    -> dict(c1, kept (bool [n_loci]), pairs, sum_r2, sum_r4, sum_d, sum_w, r2 [n_loci][n_loci]
    (NaN outside the kept pairs i < j))"""
    H = np.asarray(bits).astype(np.int64)
    n, L = H.shape
    pos = np.asarray(pos, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64)
    nb = e.size - 1
    c1 = H.sum(axis=0)
    kept = np.minimum(c1, n - c1) >= max(1, int(min_minor))
    C = H.T @ H
    i, j = np.triu_indices(L, 1)
    ok = kept[i] & kept[j]
    i, j = i[ok], j[ok]
    dn = (n * C[i, j] - c1[i] * c1[j]).astype(np.float64)
    r2 = (dn * dn) / ((c1[i] * (n - c1[i])).astype(np.float64) *
                      (c1[j] * (n - c1[j])).astype(np.float64))
    d = pos[j] - pos[i]
    full = np.full((L, L), np.nan)
    full[i, j] = r2
    b = np.searchsorted(e, d, side='right') - 1
    b[(d < e[0]) | ~(d < e[-1])] = -1
    w = drift_weight(morgans_to_c(d)) if morgans else np.zeros(d.size)
    out = dict(c1=c1, kept=kept, r2=full, pairs=np.zeros(nb, np.int64),
               sum_r2=np.zeros(nb), sum_r4=np.zeros(nb), sum_d=np.zeros(nb), sum_w=np.zeros(nb))
    for k in range(nb):
        s = b == k
        out['pairs'][k] = int(s.sum())
        out['sum_r2'][k] = math.fsum(r2[s])
        out['sum_r4'][k] = math.fsum(r2[s] * r2[s])
        out['sum_d'][k] = math.fsum(d[s])
        out['sum_w'][k] = math.fsum(w[s])
    return out
