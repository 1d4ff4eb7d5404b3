"""Moving-window diversity rasters: where on the landscape diversity is high or low.

Definition (what Model.calc_diversity_map, Species._calc_diversity_map and the device call
gnx_divmap_sums, csrc/gnx_divmap.hip, all mean):

* Map grid: the landscape cut into nx x ny rectangles by coordinate exactly as
  Species._group_by_grid cuts it (label iy * nx + ix).  Rasters are indexed [iy][ix], like a
  Layer's rast[y, x].
* Window: the window of map cell (iy, ix) is the set of map cells within Chebyshev distance
  r = (win - 1) / 2, clipped at the landscape's edge; win is odd and >= 1.  Windows overlap: an
  individual belongs to every window whose centre is within r map cells of its own.
* Per-locus counts: for a window with n individuals, locus l has c_l 1-alleles over both
  homologues (0 .. 2n) and h_l heterozygotes.
* The device returns per window, over the L' selected loci, four exact integers:
  n (int32), S = #{l : 0 < c_l < 2n} (int32), sum_het = sum_l h_l (int64),
  sum_cc = sum_l c_l (2n - c_l) (int64).
* The host arithmetic (window_stats) agrees with sim/fst.diversity:
  pi = sum_cc / (n (2n - 1)) (a sum over loci, as there), He = pi / L', Ho = sum_het / (n L'),
  Fis = 1 - Ho / He, theta_w = S / a1, tajima_d with fst.tajima_constants(2n) (NaN for S = 0 or
  2n < 4).  Windows with n < min_n (min_n >= 1, default 2) are NaN in every float raster.

Pure numpy: no device is needed here.
"""
import numpy as np

from . import fst as _fst

FLOAT_KEYS = ('pi', 'theta_w', 'tajima_d', 'Ho', 'He', 'Fis')


def box_sum(a, r):
    """out[iy][ix] = the sum of a over the cells within Chebyshev distance r of (iy, ix), clipped
    at the edges; a: 2-d integers -> int64, the same shape"""
    a = np.asarray(a, dtype=np.int64)
    if a.ndim != 2:
        raise ValueError('box_sum: a 2-d array')
    r = int(r)
    if r < 0:
        raise ValueError('box_sum: r >= 0')
    ny, nx = a.shape
    sat = np.zeros((ny + 1, nx + 1), np.int64)
    sat[1:, 1:] = a.cumsum(axis=0).cumsum(axis=1)
    y0 = np.clip(np.arange(ny) - r, 0, ny)[:, None]
    y1 = np.clip(np.arange(ny) + r + 1, 0, ny)[:, None]
    x0 = np.clip(np.arange(nx) - r, 0, nx)[None, :]
    x1 = np.clip(np.arange(nx) + r + 1, 0, nx)[None, :]
    return sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0]


def window_stats(n, S, sum_het, sum_cc, n_loci, min_n=2):
    """the float rasters of the four integer rasters over n_loci loci -> dict pi, theta_w,
    tajima_d, Ho, He, Fis (float64, the shape of n); NaN where n < min_n.
    tajima_constants is taken once per distinct n."""
    n = np.asarray(n, dtype=np.int64)
    S = np.asarray(S, dtype=np.int64)
    sum_het = np.asarray(sum_het, dtype=np.int64)
    sum_cc = np.asarray(sum_cc, dtype=np.int64)
    if not n.shape == S.shape == sum_het.shape == sum_cc.shape:
        raise ValueError('window_stats: n, S, sum_het and sum_cc of one shape')
    min_n, n_loci = int(min_n), int(n_loci)
    if min_n < 1:
        raise ValueError('min_n: at least 1')
    if n_loci < 0:
        raise ValueError('n_loci: not negative')
    out = {k: np.full(n.shape, np.nan) for k in FLOAT_KEYS}
    for nv in np.unique(n):
        nv = int(nv)
        if nv < min_n:
            continue
        at = n == nv
        m = 2 * nv
        a1, a2, e1, e2 = _fst.tajima_constants(m)
        s = S[at].astype(np.float64)
        # n (2n - 1) < 2^61 and sum_cc < 2^63: one rounding each, then one division
        pi = sum_cc[at].astype(np.float64) / float(nv * (m - 1))
        out['pi'][at] = pi
        with np.errstate(divide='ignore', invalid='ignore'):
            out['theta_w'][at] = s / a1
            if m >= 4:
                d = (pi - s / a1) / np.sqrt(e1 * s + e2 * s * (s - 1))
                out['tajima_d'][at] = np.where(s > 0, d, np.nan)
            if n_loci:
                he = pi / n_loci
                ho = sum_het[at].astype(np.float64) / float(nv * n_loci)
                out['He'][at], out['Ho'][at] = he, ho
                out['Fis'][at] = 1 - ho / he
    return out
