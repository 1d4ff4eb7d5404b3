"""Haplotype sweep scans of the phased genomes (csrc/gnx_sweeps.hip, gnx_sweeps_scan): extended
haplotype homozygosity (EHH; Sabeti et al. 2002), its integral iHH, the integrated haplotype
score iHS (Voight et al. 2006), nSL (Ferrer-Admetlla et al. 2014: iHS measured in segregating
sites) and the cross-population XP-EHH (Sabeti et al. 2007).  Pure numpy: the device gives, per
core locus, direction and class, the integer area under the curve of identical pairs; what is
computed here is the integer coordinate the areas are measured on (`sweep_map`), the statistics
from the areas, and `brute_scan`, a numpy restatement of the entry point as include/gnx_hip.h
defines it, which the tests compare the device with bit for bit.

The coordinate.  A map position in Morgans (sim/ld.py, map_positions) is quantised to
POS_PER_MORGAN = 2^24 units per Morgan (6e-8 Morgans): an area is a sum of pair counts (below
2^23 for the 4096 chromosomes a call takes) times distances, and stays inside int64 up to a map of
2^14 Morgans, chromosome breaks (40 Morgans each) included.  A rate of 0.5 or more between two loci
is a chromosome boundary: no scan crosses it.
"""
import numpy as np

from . import ld as _ld

POS_PER_MORGAN = 2 ** 24
CUT_DEN = 2 ** 20
MAX_N = 2048

LEFT, RIGHT = 0, 1
ST_CUTOFF, ST_EDGE, ST_GAP, ST_EXTENT, ST_NO_CLASS, ST_NOT_SCANNED = 0, 1, 2, 3, 4, 5


def sweep_map(rates, unit='morgans', kept=None):
    """(pos int64 [L], brk uint8 [L], scale) from the per-locus recombination rates (rates[l]
    between loci l - 1 and l); a length in the unit is an integer length / scale.  'morgans': pos
    = rint(map_positions(rates) 2^24), scale 2^24; 'loci': pos = l; 'sites': pos = the rank of
    the locus among the kept loci (kept bool [L]; a locus that is not kept gets the rank of the
    last kept one before it).  brk[l] = rates[l] >= 0.5 in every unit (brk[0] is never set)"""
    r = np.asarray(rates, dtype=np.float64).ravel()
    if r.size == 0:
        raise ValueError('rates: a non-empty list of recombination rates')
    scale = 1
    if unit == 'morgans':
        pos = np.rint(_ld.map_positions(r) * POS_PER_MORGAN).astype(np.int64)
        scale = POS_PER_MORGAN
    elif unit == 'loci':
        pos = np.arange(r.size, dtype=np.int64)
    elif unit == 'sites':
        if kept is None:
            raise ValueError("unit 'sites' needs the mask of the kept loci")
        k = np.asarray(kept, dtype=bool).ravel()
        if k.size != r.size:
            raise ValueError('kept: %d entries for %d loci' % (k.size, r.size))
        pos = np.maximum(np.cumsum(k) - 1, 0).astype(np.int64)
    else:
        raise ValueError("unit: 'morgans', 'loci' or 'sites', not %r" % (unit,))
    brk = (r >= 0.5).astype(np.uint8)
    brk[0] = 0
    return pos, brk, scale


def cutoff_fraction(cutoff):
    """the EHH cutoff as the fraction (num, 2^20) the device compares integers with"""
    c = float(cutoff)
    if not 0.0 <= c <= 1.0:
        raise ValueError('cutoff: an EHH value in 0..1 (got %r)' % (cutoff,))
    return int(round(c * CUT_DEN)), CUT_DEN


def kept_loci(c1, n_chrom, min_minor):
    """bool [n_loci]: min(c1, N - c1) >= max(2, min_minor)"""
    c1 = np.asarray(c1, dtype=np.int64)
    return np.minimum(c1, int(n_chrom) - c1) >= max(2, int(min_minor))


def scan_work(n_scanned, n_chrom, n_kept):
    return int(n_scanned) * 4 * ((int(n_chrom) + 63) // 64) * max(0, int(n_kept) - 1)


# ---------------------------------------------------------------------- the restatement
def _extend(lab, allele):
    """the labels of the tuples extended by one allele (renumbered 0 .. groups - 1) and the
    number of pairs with equal tuples"""
    key = lab * 2 + allele
    cnt = np.bincount(key)
    used = cnt > 0
    return (np.cumsum(used) - 1)[key], int((cnt * (cnt - 1) // 2).sum())


def brute_scan(rows, pos, brk=None, cls=None, cores=None, min_minor=2, cut_num=0, cut_den=1,
               max_gap=0, max_extent=0, curve=False):
    """gnx_sweeps_scan restated (include/gnx_hip.h), the slow and obvious way.  rows [N][n_loci]
    of 0 / 1: the sampled chromosomes (2 i + h) at the request's loci.  Every chromosome of the
    class carries the tuple of its alleles at the kept loci passed so far, extended step by step
    (held as a label: two chromosomes have the same label iff their tuples are equal), and P is
    the number of pairs with equal tuples
    -> dict(c1 int64 [n_loci], area int64, steps int32, status uint8 [n_loci][2][2], curve int64
    [2][2][n_loci] or None, work, kept bool [n_loci])"""
    R = np.asarray(rows).astype(np.int64)
    N, n_loci = R.shape
    pos = np.asarray(pos, dtype=np.int64).ravel()
    b = np.zeros(n_loci, bool) if brk is None else np.asarray(brk).ravel() != 0
    c1 = R.sum(axis=0)
    keep = kept_loci(c1, N, min_minor)
    kept = np.flatnonzero(keep)
    K = kept.size
    # a break anywhere in (kept[k - 1], kept[k]] separates the two
    nb = np.cumsum(np.r_[False, b[1:]])
    kb = np.zeros(K, bool)
    kb[1:] = nb[kept[1:]] > nb[kept[:-1]]
    kof = np.full(n_loci, -1)
    kof[kept] = np.arange(K)
    core_list = kept if cores is None else [int(j) for j in cores]
    if curve and len(core_list) != 1:
        raise ValueError('curve: exactly one core')
    area = np.zeros((n_loci, 2, 2), np.int64)
    steps = np.zeros((n_loci, 2, 2), np.int32)
    status = np.full((n_loci, 2, 2), ST_NOT_SCANNED, np.uint8)
    cv = np.full((2, 2, n_loci), -1, np.int64) if curve else None
    if cls is not None:
        cls = np.asarray(cls, dtype=np.uint8).ravel()
    n_scanned = 0
    for j in core_list:
        if kof[j] < 0:
            continue
        n_scanned += 1
        kc = int(kof[j])
        for d in (LEFT, RIGHT):
            for c in (0, 1):
                members = np.flatnonzero((R[:, j] if cls is None else cls) == c)
                m = members.size
                if m < 2:
                    status[j, d, c] = ST_NO_CLASS
                    continue
                Tc = m * (m - 1) // 2
                lab = np.zeros(m, np.int64)
                cols = R[np.ix_(members, kept)]
                P, A, s, k = Tc, 0, 0, kc
                if cv is not None:
                    cv[d, c, 0] = P
                while True:
                    kn = k + (1 if d == RIGHT else -1)
                    if kn < 0 or kn >= K or kb[max(k, kn)]:
                        st = ST_EDGE
                        break
                    gap = abs(int(pos[kept[kn]]) - int(pos[kept[k]]))
                    if max_gap > 0 and gap > max_gap:
                        st = ST_GAP
                        break
                    if max_extent > 0 and abs(int(pos[kept[kn]]) - int(pos[j])) > max_extent:
                        st = ST_EXTENT
                        break
                    lab, Pn = _extend(lab, cols[:, kn])
                    if cv is not None:
                        cv[d, c, s + 1] = Pn
                    if Pn * cut_den < cut_num * Tc:
                        st = ST_CUTOFF
                        break
                    A += (P + Pn) * gap
                    P, s, k = Pn, s + 1, kn
                area[j, d, c], steps[j, d, c], status[j, d, c] = A, s, st
    return dict(c1=c1, area=area, steps=steps, status=status, curve=cv,
                work=scan_work(n_scanned, N, K), kept=keep)


# ---------------------------------------------------------------------- the statistics
def class_pairs(m):
    """T = m (m - 1) / 2"""
    m = np.asarray(m, dtype=np.int64)
    return m * (m - 1) // 2


def ihh(area, T):
    """the integrated EHH in the caller's integer unit: area / (2 T); NaN where T == 0"""
    a = np.asarray(area, dtype=np.float64)
    t = np.asarray(T, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(t > 0, a / (2.0 * t), np.nan)


def ihh_both(area, status, T0, T1, keep_edge=False):
    """(iHH of class 0, iHH of class 1) [n_loci], each the sum of both directions; NaN where one
    of the locus's four scans was not run (status 4, 5) or - unless keep_edge - ended at an edge
    or a gap (status 1, 2) before the cutoff"""
    area = np.asarray(area, dtype=np.int64)
    st = np.asarray(status)
    bad = (st >= ST_NO_CLASS).any(axis=(1, 2))
    if not keep_edge:
        bad |= ((st == ST_EDGE) | (st == ST_GAP)).any(axis=(1, 2))
    h0 = ihh(area[:, 0, 0] + area[:, 1, 0], T0)
    h1 = ihh(area[:, 0, 1] + area[:, 1, 1], T1)
    h0[bad] = np.nan
    h1[bad] = np.nan
    return h0, h1


def log_ratio(num, den):
    """ln(num / den); NaN where either is NaN or 0"""
    a = np.asarray(num, dtype=np.float64)
    b = np.asarray(den, dtype=np.float64)
    ok = (a > 0) & (b > 0)
    out = np.full(a.shape, np.nan)
    out[ok] = np.log(a[ok] / b[ok])
    return out


def ihs_unstandardized(area, status, c1, n_chrom, keep_edge=False):
    """ln(iHH_1 / iHH_0) per locus, class 1 the derived allele (c1 carriers), iHH the sum of both
    directions.  NaN if any of the four scans has status 1, 2, 4 or 5 (keep_edge: only 4 or 5),
    or if an iHH is 0 -> (ihs_unstd, ihh1, ihh0)"""
    c1 = np.asarray(c1, dtype=np.int64)
    h0, h1 = ihh_both(area, status, class_pairs(int(n_chrom) - c1), class_pairs(c1), keep_edge)
    return log_ratio(h1, h0), h1, h0


def standardize(x):
    """(x - mean) / sd over the defined entries (sd with ddof 0); all NaN with fewer than 2
    defined entries or sd 0"""
    x = np.asarray(x, dtype=np.float64)
    ok = np.isfinite(x)
    out = np.full(x.shape, np.nan)
    if ok.sum() >= 2:
        sd = x[ok].std()
        if sd > 0:
            out[ok] = (x[ok] - x[ok].mean()) / sd
    return out


def standardize_by_frequency(x, freq, n_bins=20):
    """x standardised within bins of the derived-allele frequency: n_bins bins of equal width over
    0..1 (frequency 1 in the last); bins with fewer than 2 defined values (or sd 0) give NaN"""
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or n_bins < 1:
        raise ValueError('n_freq_bins: at least 1 bin (got %r)' % (n_bins,))
    x = np.asarray(x, dtype=np.float64)
    f = np.asarray(freq, dtype=np.float64)
    if f.shape != x.shape:
        raise ValueError('freq: one frequency per value')
    b = np.minimum((f * int(n_bins)).astype(np.int64), int(n_bins) - 1)
    out = np.full(x.shape, np.nan)
    for k in np.unique(b):
        i = np.flatnonzero(b == k)
        out[i] = standardize(x[i])
    return out


def ehh_curve(curve, kept, core, T, n_loci):
    """the decay curve of one core over the request's loci from curve [2][2][n_loci] (P per step):
    (ehh0, ehh1) float64 [n_loci], P / T at the kept locus each step reached (the core itself:
    1), NaN at loci that are not kept and past the scan's end; where the scan ended at the
    cutoff, the first value below the cutoff is included"""
    kept_idx = np.flatnonzero(np.asarray(kept, dtype=bool))
    kc = int(np.searchsorted(kept_idx, core))
    if kc >= kept_idx.size or kept_idx[kc] != core:
        raise ValueError('the core is not a kept locus')
    out = np.full((2, n_loci), np.nan)
    for c in (0, 1):
        if T[c] <= 0:
            continue
        for d, sign in ((LEFT, -1), (RIGHT, 1)):
            p = np.asarray(curve[d][c])
            ns = int((p >= 0).sum())
            k = kc + sign * np.arange(ns)
            out[c, kept_idx[k]] = p[:ns] / float(T[c])
    return out[0], out[1]
