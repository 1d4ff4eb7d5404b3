"""Pairwise coalescence through the recorded pedigree (csrc/gnx_coal.hip: gnx_coal_times,
gnx_coal_segments): the time to the most recent common ancestor of pairs of sample nodes, its
distribution, and the segments two genomes inherited from one ancestor (identity by descent).
Pure numpy: the device gives integer sums over the (pair, locus) cells; what is computed here is
the statistics from those integers (`tmrca_stats`, `branch_diversity`, `tmrca_by_distance`,
`coal_rate`, `fold_to_individuals`) and `coal_mrca_np` / `coal_times_np` / `coal_segments_np`,
numpy restatements of the two entry points as include/gnx_hip.h defines them, which the tests
compare the device with bit for bit.

The restatement does not walk as the device does.  The device merges the two lineages step by
step and stores nothing; here both chains are written out in full (TreeTables.lineages with
drop_before_sim=False, the walk tests/test_lineage_host.py checks against the edge rows) and the
MRCA is their largest common element.
"""
import numpy as np

from . import tracts as _tr


def n_pairs(n):
    return n * (n - 1) // 2


def pair_index(n):
    """(i, j) of the unordered pairs in the row-major upper-triangle order of the device"""
    return np.triu_indices(n, 1)


# ---------------------------------------------------------------------- the restatement
def _path_bits(paths, L):
    """bool [n_paths][L] from bool / 0-1 rows, or from the packed uint64 words of the device"""
    p = np.asarray(paths)
    if p.dtype == np.uint64:
        b = (p[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
        return b.reshape(p.shape[0], -1)[:, :L].astype(bool)
    return p.astype(bool)


def _chains(tab, paths_or_tt, nodes, loci):
    """every chain in full, youngest first: int64 [n_loci][n_nodes][longest], padded with -1"""
    nodes = np.asarray(nodes, dtype=np.int64).ravel()
    loci = np.asarray(loci, dtype=np.int64).ravel()
    nq = nodes.size * loci.size
    if hasattr(paths_or_tt, 'lineages'):
        off, chain = paths_or_tt.lineages(nodes, loci, 0, drop_before_sim=False)
        chain = chain.astype(np.int64)
    else:                                  # path bits: follow anc(v, l) as the header defines it
        tab = np.asarray(tab, dtype=np.int64)
        bits = _path_bits(paths_or_tt, int(loci.max()) + 1)
        cur = np.tile(nodes, loci.size)
        loc = np.repeat(loci, nodes.size)
        act = np.arange(nq)
        qs, cs = [], []
        while act.size:
            c = cur[act]
            qs.append(act)
            cs.append(c)
            go = tab[c, 0] >= 0
            act, c = act[go], c[go]
            ks = tab[c, 1]
            cur[act] = 2 * tab[c, 0] + ((ks & 1) ^ bits[ks >> 1, loc[act]])
        q, c = np.concatenate(qs), np.concatenate(cs)
        order = np.argsort(q, kind='stable')
        off = np.zeros(nq + 1, np.int64)
        np.cumsum(np.bincount(q, minlength=nq), out=off[1:])
        chain = c[order]
    n_len = np.diff(off)
    out = np.full((nq, int(n_len.max())), -1, np.int64)
    k = np.arange(chain.size) - np.repeat(off[:-1], n_len)
    out[np.repeat(np.arange(nq), n_len), k] = chain
    return out.reshape(loci.size, nodes.size, -1)


def coal_mrca_np(tab, bt, paths_or_tt, nodes, loci):
    """mrca(a, b, l) of include/gnx_hip.h for every two of `nodes` at `loci`: the largest node id
    on both chains, -1 if there is none; no age limit.  paths_or_tt: the TreeTables the node
    table (tab, bt) comes from, or the recombination paths as bit rows [n_paths][L] (or packed
    uint64 words).  -> int32 [n_loci][n_pairs], the pairs in row-major upper-triangle order"""
    nodes = np.asarray(nodes, dtype=np.int64).ravel()
    tab = np.asarray(tab)
    C = _chains(tab, paths_or_tt, nodes, loci)
    n_loci, n, _ = C.shape
    out = np.full((n_loci, n_pairs(n)), -1, np.int32)
    li = np.arange(n_loci)
    k = 0
    for i in range(n - 1):
        mark = np.zeros((n_loci, tab.shape[0] + 1), bool)       # (the padding -1: the last column)
        mark[li[:, None], C[:, i, :]] = True
        mark[:, -1] = False
        others = C[:, i + 1:, :]
        hit = mark[li[:, None, None], others]
        first = hit.argmax(axis=2)                               # chains descend: the largest
        m = np.take_along_axis(others, first[:, :, None], axis=2)[:, :, 0]
        out[:, k:k + n - 1 - i] = np.where(hit.any(axis=2), m, -1)
        k += n - 1 - i
    return out


def coal_mask(mrca, bt, t_curr, max_ago=-1):
    """(the MRCA where the pair coalesces, -1 elsewhere; T there, 0 elsewhere): a pair coalesces
    where mrca >= 0 and ago(mrca) = bt[mrca >> 1] + t_curr <= max_ago (max_ago < 0: no limit)"""
    mrca = np.asarray(mrca, dtype=np.int64)
    bt = np.asarray(bt, dtype=np.int64)
    ago = bt[np.maximum(mrca, 0) >> 1] + int(t_curr)
    ok = mrca >= 0
    if max_ago is not None and max_ago >= 0:
        ok &= ago <= int(max_ago)
    return np.where(ok, mrca, -1).astype(np.int32), np.where(ok, ago, 0)


def coal_times_np(tab, bt, paths_or_tt, nodes, loci, t_curr, max_ago=-1, tedges=None):
    """gnx_coal_times restated: every output of the entry point
    -> dict(pair_sum int64 [n][n], pair_cnt int32 [n][n], locus_sum, locus_cnt int64 [n_loci],
    locus_max int32 [n_loci], thist int64 [n_tedges - 1] or None, mrca int32 [n_loci][n_pairs],
    work)"""
    nodes = np.asarray(nodes, dtype=np.int64).ravel()
    n = nodes.size
    m, T = coal_mask(coal_mrca_np(tab, bt, paths_or_tt, nodes, loci), bt, t_curr, max_ago)
    hit = m >= 0
    i, j = pair_index(n)
    pair_sum = np.zeros((n, n), np.int64)
    pair_cnt = np.zeros((n, n), np.int32)
    pair_sum[i, j] = pair_sum[j, i] = T.sum(axis=0)
    pair_cnt[i, j] = pair_cnt[j, i] = hit.sum(axis=0)
    thist = None
    if tedges is not None:
        e = np.asarray(tedges, dtype=np.int64).ravel()
        t = T[hit]
        b = np.searchsorted(e, t, side='right') - 1
        b = b[(t >= e[0]) & (t < e[-1])]
        thist = np.bincount(b, minlength=e.size - 1).astype(np.int64)
    return dict(pair_sum=pair_sum, pair_cnt=pair_cnt, locus_sum=T.sum(axis=1).astype(np.int64),
                locus_cnt=hit.sum(axis=1).astype(np.int64),
                locus_max=np.where(hit.any(axis=1), np.where(hit, T, -2 ** 31).max(axis=1),
                                   -1).astype(np.int32),
                thist=thist, mrca=m, work=n_pairs(n) * m.shape[0])


def segments_of(M, pos, brk=None, min_loci=1, min_len=0):
    """the qualifying segments of rows of MRCAs M int [rows][n_loci] (-1: the pair does not
    coalesce there): maximal stretches of list positions with one MRCA >= 0 and no break inside
    -> (row, s, e, count, length), a row's segments in ascending order"""
    M = np.atleast_2d(np.asarray(M, dtype=np.int64))
    pos = np.asarray(pos, dtype=np.int64).ravel()
    nl = M.shape[1]
    b = np.zeros(nl, bool) if brk is None else np.asarray(brk).astype(bool).ravel().copy()
    b[0] = False
    ok = M >= 0
    cont = np.zeros(M.shape, bool)                  # the segment at q - 1 continues into q
    cont[:, 1:] = ok[:, 1:] & (M[:, 1:] == M[:, :-1]) & ~b[None, 1:]
    start = ok & ~cont
    end = ok.copy()
    end[:, :-1] &= ~cont[:, 1:]
    row, s = np.nonzero(start)
    row_e, e = np.nonzero(end)
    assert (row == row_e).all() and (s <= e).all()
    count = e - s + 1
    length = pos[e] - pos[s]
    q = (count >= max(1, int(min_loci))) & (length >= int(min_len))
    return row[q], s[q], e[q], count[q], length[q]


def coal_segments_np(tab, bt, paths_or_tt, nodes, loci, pos, brk=None, t_curr=0, max_ago=-1,
                     min_loci=1, min_len=0, edges=None, cover=False):
    """gnx_coal_segments restated: every output of the entry point
    -> dict(cnt int32 [n][n], len, longest int64 [n][n], hist int64 [n_edges - 1][2] or None,
    cover int64 [n_loci] or None, work)"""
    nodes = np.asarray(nodes, dtype=np.int64).ravel()
    loci = np.asarray(loci, dtype=np.int64).ravel()
    if (np.diff(loci) <= 0).any():
        raise ValueError('loci must be strictly ascending')
    n = nodes.size
    m, _ = coal_mask(coal_mrca_np(tab, bt, paths_or_tt, nodes, loci), bt, t_curr, max_ago)
    row, s, e, _, length = segments_of(m.T, pos, brk, min_loci, min_len)
    i, j = pair_index(n)
    cnt = np.zeros((n, n), np.int32)
    tot = np.zeros((n, n), np.int64)
    longest = np.zeros((n, n), np.int64)
    np.add.at(cnt, (i[row], j[row]), 1)
    np.add.at(tot, (i[row], j[row]), length)
    np.maximum.at(longest, (i[row], j[row]), length)
    for M in (cnt, tot, longest):
        M += M.T
    ed, hist, cov = _tr._outputs(loci.size, edges, cover)
    _tr._binned(hist, cov, s, e, length, ed)
    return dict(cnt=cnt, len=tot, longest=longest, hist=hist, cover=cov,
                work=n_pairs(n) * loci.size)


# ---------------------------------------------------------------------- the statistics
def default_time_edges(top, n_bins):
    """at most n_bins integer bins of about equal width over 0 .. top (both included in the
    first and last bin) -> int64 edges, strictly ascending"""
    if isinstance(n_bins, bool) or int(n_bins) != n_bins or not 1 <= n_bins <= 64:
        raise ValueError('n_time_bins: 1..64 bins (got %r)' % (n_bins,))
    e = np.unique(np.rint(np.linspace(0, int(top) + 1, int(n_bins) + 1)).astype(np.int64))
    return e


def tmrca_stats(pair_sum, pair_cnt, locus_sum, locus_cnt, locus_max):
    """the means from the integers: tmrca float64 [n][n] (mean T of a pair over the loci at
    which it coalesces, NaN where it never does), per_locus dict(mean, share_coalesced, max: NaN
    where no pair coalesces), share_coalesced (of all cells)"""
    n = pair_cnt.shape[0]
    with np.errstate(divide='ignore', invalid='ignore'):
        tm = pair_sum.astype(np.float64) / pair_cnt.astype(np.float64)
        tm[pair_cnt == 0] = np.nan
        mean = locus_sum.astype(np.float64) / locus_cnt.astype(np.float64)
        mean[locus_cnt == 0] = np.nan
    np_ = float(n_pairs(n))
    per = dict(mean=mean, share_coalesced=locus_cnt / np_,
               max=np.where(locus_cnt > 0, locus_max.astype(np.float64), np.nan))
    return tm, per, float(locus_cnt.sum() / (np_ * locus_cnt.size))


def _mean_t(pair_sum, pair_cnt, a, b):
    """(mean T, coalesced cells, all cells per locus) over the unordered pairs between the node
    index sets a and b (a is b: within)"""
    S, Cn = pair_sum[np.ix_(a, b)], pair_cnt[np.ix_(a, b)]
    if a is b:
        s, c, cells = int(np.triu(S, 1).sum()), int(np.triu(Cn, 1).sum()), n_pairs(len(a))
    else:
        s, c, cells = int(S.sum()), int(Cn.sum()), len(a) * len(b)
    return (s / c if c else float('nan')), c, cells


def branch_diversity(pair_sum, pair_cnt, node_groups=None):
    """branch-mode diversity and divergence, 2 x the mean T over the (pair, locus) cells that
    coalesce (tskit's divergence(mode='branch') per unit of sequence, where every cell
    coalesces).  node_groups: a list of arrays of node indices (disjoint)
    -> (within all, by_group dict(within [G], between [G][G]) or None)"""
    everyone = np.arange(pair_cnt.shape[0])
    total = 2.0 * _mean_t(pair_sum, pair_cnt, everyone, everyone)[0]
    if node_groups is None:
        return total, None
    G = len(node_groups)
    within = np.full(G, np.nan)
    between = np.full((G, G), np.nan)
    for g in range(G):
        if len(node_groups[g]) >= 2:
            within[g] = 2.0 * _mean_t(pair_sum, pair_cnt, node_groups[g], node_groups[g])[0]
        for k in range(g + 1, G):
            if len(node_groups[g]) and len(node_groups[k]):
                between[g, k] = between[k, g] = 2.0 * _mean_t(pair_sum, pair_cnt, node_groups[g],
                                                              node_groups[k])[0]
    return total, dict(within=within, between=between)


def fold_to_individuals(cnt, tot, longest):
    """node matrices [2m][2m] (nodes 2 i, 2 i + 1 of individual i) folded to individuals [m][m]
    as gnx_tracts_pairs defines its matrices: off the diagonal the four node pairs summed (the
    max for longest), on the diagonal the individual's own two nodes"""
    def four(M):
        m = M.shape[0] // 2
        return np.asarray(M).reshape(m, 2, m, 2)
    c4, t4, g4 = four(cnt), four(tot), four(longest)
    c, t, g = c4.sum(axis=(1, 3)), t4.sum(axis=(1, 3)), g4.max(axis=(1, 3))
    d = np.arange(c.shape[0])
    c[d, d], t[d, d], g[d, d] = c4[d, 0, d, 1], t4[d, 0, d, 1], g4[d, 0, d, 1]
    return c.astype(np.int32), t.astype(np.int64), g.astype(np.int64)


def tmrca_by_distance(x, y, pair_sum, pair_cnt, n_loci, edges):
    """mean T per class of geographic distance over the between-individual pairs (the four node
    pairs of two individuals; nodes 2 i, 2 i + 1 belong to individual i at x[i], y[i]; classes
    as sim/tracts.sharing_stats) -> dict(pairs, mean_tmrca, share_coalesced, mean_dist)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32).astype(np.float64)
    e = np.asarray(edges, np.float64)
    m = x.size
    S = pair_sum.reshape(m, 2, m, 2).sum(axis=(1, 3)).astype(np.float64)
    Cn = pair_cnt.reshape(m, 2, m, 2).sum(axis=(1, 3)).astype(np.float64)
    i, j = np.triu_indices(m, 1)
    dx, dy = x[i] - x[j], y[i] - y[j]
    r = np.sqrt(dx * dx + dy * dy)
    k = np.searchsorted(e, r, side='right') - 1
    k[(r < e[0]) | ~(r < e[-1])] = -1
    ok = k >= 0
    nb = e.size - 1
    pairs = np.bincount(k[ok], minlength=nb).astype(np.int64)
    with np.errstate(divide='ignore', invalid='ignore'):
        c = np.bincount(k[ok], Cn[i, j][ok], nb)
        return dict(pairs=pairs, mean_tmrca=np.bincount(k[ok], S[i, j][ok], nb) / c,
                    share_coalesced=c / (4.0 * n_loci * pairs),
                    mean_dist=np.bincount(k[ok], r[ok], nb) / pairs)


def coal_rate(thist, tedges, n_cells, n_before=0):
    """the inverse coalescence rate per time bin from the histogram of T.  R_k = the (pair,
    locus) cells not yet coalesced at tedges[k]: n_cells - n_before (the cells with T <
    tedges[0]) at k = 0, then R_k - c_k.  p_k = 1 - (1 - c_k / R_k)^(1 / (tedges[k + 1] -
    tedges[k])) is the chance per generation that a cell at risk coalesces, and Ne_k = 1 / (2
    p_k): NaN where R_k = 0, inf where c_k = 0
    -> dict(edges, counts, at_risk, ne)"""
    c = np.asarray(thist, dtype=np.int64).ravel()
    e = np.asarray(tedges, dtype=np.int64).ravel()
    R = int(n_cells) - int(n_before) - np.r_[0, np.cumsum(c)[:-1]]
    w = np.diff(e).astype(np.float64)
    ne = np.full(c.size, np.nan)
    risk = R > 0
    with np.errstate(divide='ignore'):
        p = 1.0 - (1.0 - c[risk] / R[risk].astype(np.float64)) ** (1.0 / w[risk])
        ne[risk] = 1.0 / (2.0 * p)
    return dict(edges=e, counts=c, at_risk=R.astype(np.int64), ne=ne)
