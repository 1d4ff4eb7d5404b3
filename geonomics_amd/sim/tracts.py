"""Identity tracts of the phased genomes (csrc/gnx_tracts.hip: gnx_tracts_self, gnx_tracts_pairs):
runs of homozygosity per individual, and tracts shared identical-by-state between the haplotypes
of two individuals as a function of their geographic distance.  Pure numpy: the device gives
integer sums over the qualifying tracts; what is computed here is the integer coordinate the
lengths are measured on (`tract_map`), the statistics from the sums (`roh_stats`,
`sharing_stats`), and `brute_self` / `brute_pairs`, numpy restatements of the two entry points as
include/gnx_hip.h defines them, which the tests compare the device with bit for bit.

The coordinate.  The device compares integers, so a map position in Morgans (sim/ld.py,
map_positions) is quantised to POS_PER_MORGAN = 2^32 units per Morgan (2.3e-10 Morgans: far
below any interval between loci; 40 Morgans per chromosome break stay far inside int64).  A rate
of 0.5 or more between two loci is a chromosome boundary: no tract continues across it.  Under
the template's free recombination (r = 0.5 everywhere) every locus is a break, so every tract is
one locus long.
"""
import math

import numpy as np

from . import ld as _ld

POS_PER_MORGAN = 2 ** 32
INT64_MAX = 2 ** 63 - 1


def tract_map(rates, unit='morgans'):
    """(pos int64 [L], brk bool [L], genome_len) from the per-locus recombination rates (rates[l]
    between loci l - 1 and l).  'morgans': pos = rint(map_positions(rates) 2^32); 'loci': pos =
    l.  brk[l] = rates[l] >= 0.5 in both units (brk[0] is never set).  genome_len = the sum over
    the break-delimited segments of pos[last] - pos[first], as an int"""
    r = np.asarray(rates, dtype=np.float64).ravel()
    if unit == 'morgans':
        pos = np.rint(_ld.map_positions(r) * POS_PER_MORGAN).astype(np.int64)
    elif unit == 'loci':
        if r.size == 0:
            raise ValueError('rates: a non-empty list of recombination rates')
        pos = np.arange(r.size, dtype=np.int64)
    else:
        raise ValueError("unit: 'morgans' or 'loci', not %r" % (unit,))
    brk = r >= 0.5
    brk[0] = False
    first = np.r_[0, np.flatnonzero(brk)]
    last = np.r_[first[1:] - 1, r.size - 1]
    return pos, brk, int((pos[last] - pos[first]).sum())


def to_units(v, unit):
    """a length or an edge given in the unit (Morgans or loci) as the integer the device compares
    with: the smallest integer length at or above it (inf: INT64_MAX)"""
    v = float(v)
    if v != v:
        raise ValueError('a length threshold is NaN')
    if v == np.inf:
        return INT64_MAX
    x = v * POS_PER_MORGAN if unit == 'morgans' else v
    if abs(x) >= 2.0 ** 62:
        raise ValueError('a length of %r %s is outside the coordinate range' % (v, unit))
    return int(math.ceil(x))


def from_units(a, unit):
    """integer lengths back in the unit, as floats"""
    a = np.asarray(a, dtype=np.float64)
    return a / POS_PER_MORGAN if unit == 'morgans' else a


def pack_breaks(brk, W64):
    """bool [L] -> the uint64 [W64] mask the device takes"""
    brk = np.asarray(brk, dtype=bool).ravel()
    out = np.zeros(W64, np.uint64)
    l = np.flatnonzero(brk)
    np.bitwise_or.at(out, l >> 6, np.uint64(1) << (l & 63).astype(np.uint64))
    return out


def check_tract_edges(edges):
    e = np.asarray(edges, dtype=np.int64).ravel()
    if not 2 <= e.size <= 65 or (np.diff(e) <= 0).any():
        raise ValueError('tract edges: 2..65 strictly ascending lengths (got %r)' % (edges,))
    return e


# ---------------------------------------------------------------------- the restatement
def _tracts(D, brk):
    """every tract of the haplotype pairs whose differences are D bool [m][L]
    -> (row, s, e), the tracts of a row in ascending order"""
    Z = ~np.asarray(D, dtype=bool)
    m, L = Z.shape
    b = np.zeros(L, bool) if brk is None else np.asarray(brk, dtype=bool).copy()
    b[0] = False
    start = Z.copy()
    start[:, 1:] &= ~Z[:, :-1] | b[None, 1:]
    end = Z.copy()
    end[:, :-1] &= ~Z[:, 1:] | b[None, 1:]
    row, s = np.nonzero(start)
    row_e, e = np.nonzero(end)
    assert (row == row_e).all() and (s <= e).all()
    return row, s, e


def _qualifying(D, pos, brk, min_loci, min_len):
    row, s, e = _tracts(D, brk)
    count = e - s + 1
    length = pos[e] - pos[s]
    ok = (count >= max(1, int(min_loci))) & (length >= int(min_len))
    return row[ok], s[ok], e[ok], count[ok], length[ok]


def _binned(hist, cover, s, e, length, edges):
    if hist is not None and length.size:
        b = np.searchsorted(edges, length, side='right') - 1
        b[(length < edges[0]) | ~(length < edges[-1])] = -1
        k = b >= 0
        np.add.at(hist[:, 0], b[k], 1)
        np.add.at(hist[:, 1], b[k], length[k])
    if cover is not None and s.size:
        d = np.zeros(cover.size + 1, np.int64)
        np.add.at(d, s, 1)
        np.add.at(d, e + 1, -1)
        cover += np.cumsum(d[:-1])


def _outputs(L, edges, cover):
    e = None if edges is None else check_tract_edges(edges)
    hist = None if e is None else np.zeros((e.size - 1, 2), np.int64)
    return e, hist, (np.zeros(L, np.int64) if cover else None)


def brute_self(haps, pos, brk=None, min_loci=1, min_len=0, edges=None, cover=False):
    """gnx_tracts_self restated (include/gnx_hip.h): haps [n][2][L] of 0 / 1, homologue 0
    against homologue 1 of every individual -> dict(per int64 [n][4] = {tracts, loci, length,
    longest}, hist int64 [n_edges - 1][2] or None, cover int64 [L] or None)"""
    H = np.asarray(haps).astype(bool)
    n, _, L = H.shape
    pos = np.asarray(pos, dtype=np.int64)
    e, hist, cov = _outputs(L, edges, cover)
    per = np.zeros((n, 4), np.int64)
    row, s, t, count, length = _qualifying(H[:, 0] ^ H[:, 1], pos, brk, min_loci, min_len)
    np.add.at(per[:, 0], row, 1)
    np.add.at(per[:, 1], row, count)
    np.add.at(per[:, 2], row, length)
    np.maximum.at(per[:, 3], row, length)
    _binned(hist, cov, s, t, length, e)
    return dict(per=per, hist=hist, cover=cov)


def pairs_work(n, L):
    return (2 * n * (n - 1) + n) * ((L + 63) // 64)


def brute_pairs(haps, pos, brk=None, min_loci=1, min_len=0, edges=None, cover=False):
    """gnx_tracts_pairs restated: for a != b the four haplotype pairs (a_h, b_g), the diagonal
    the individual's own pair; hist and cover over the off-diagonal unordered pairs
    -> dict(cnt int32 [n][n], len, longest int64 [n][n], hist, cover, work)"""
    H = np.asarray(haps).astype(bool)
    n, _, L = H.shape
    pos = np.asarray(pos, dtype=np.int64)
    e, hist, cov = _outputs(L, edges, cover)
    cnt = np.zeros((n, n), np.int32)
    tot = np.zeros((n, n), np.int64)
    longest = np.zeros((n, n), np.int64)
    own = brute_self(H, pos, brk, min_loci, min_len)['per']
    idx = np.arange(n)
    cnt[idx, idx], tot[idx, idx], longest[idx, idx] = own[:, 0], own[:, 2], own[:, 3]
    for a in range(n - 1):
        # rows: (b - a - 1) * 4 + 2 h + g
        D = (H[a][None, :, None, :] ^ H[a + 1:][:, None, :, :]).reshape(-1, L)
        row, s, t, count, length = _qualifying(D, pos, brk, min_loci, min_len)
        b = a + 1 + row // 4
        np.add.at(cnt[a], b, 1)
        np.add.at(tot[a], b, length)
        np.maximum.at(longest[a], b, length)
        _binned(hist, cov, s, t, length, e)
    for M in (cnt, tot, longest):
        M += np.triu(M, 1).T
    return dict(cnt=cnt, len=tot, longest=longest, hist=hist, cover=cov, work=pairs_work(n, L))


# ---------------------------------------------------------------------- the statistics
def roh_stats(roh_loci, roh_len, genome_len, L, unit):
    """per-individual F_ROH and its mean: the share of the genome in runs of homozygosity, by
    length ('morgans': roh_len / genome_len) or by locus count ('loci': roh_loci / L)"""
    if unit == 'morgans':
        num, den = np.asarray(roh_len, np.float64), float(genome_len)
    else:
        num, den = np.asarray(roh_loci, np.float64), float(L)
    f = num / den if den > 0 else np.full(num.shape, np.nan)
    return f, (float(f.mean()) if f.size else float('nan'))


def sharing_stats(x, y, cnt, length, edges):
    """per class of geographic distance (edges[k] <= r < edges[k + 1], r in fp64 from fp32 x, y)
    over the unordered pairs: the number of pairs, the mean tracts per pair, the mean shared
    length per pair and the share of pairs with at least one tract (NaN in an empty class)
    -> dict(pairs, mean_tracts, mean_len, share_with_tract, mean_dist)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32).astype(np.float64)
    e = np.asarray(edges, np.float64)
    i, j = np.triu_indices(x.size, 1)
    dx, dy = x[i] - x[j], y[i] - y[j]
    r = np.sqrt(dx * dx + dy * dy)
    k = np.searchsorted(e, r, side='right') - 1
    k[(r < e[0]) | ~(r < e[-1])] = -1
    nb = e.size - 1
    c = np.asarray(cnt)[i, j].astype(np.float64)
    ln = np.asarray(length, np.float64)[i, j]
    ok = k >= 0
    m = np.bincount(k[ok], minlength=nb).astype(np.int64)
    with np.errstate(divide='ignore', invalid='ignore'):
        md = m.astype(np.float64)
        out = dict(pairs=m,
                   mean_tracts=np.bincount(k[ok], c[ok], nb) / md,
                   mean_len=np.bincount(k[ok], ln[ok], nb) / md,
                   share_with_tract=np.bincount(k[ok], (c[ok] > 0).astype(np.float64), nb) / md,
                   mean_dist=np.bincount(k[ok], r[ok], nb) / md)
    return out
