"""What the kinship tests share (test_kin_host.py, test_gpu_kin.py): a synthetic pedigree with
known relations, the brute-force pair list that include/gnx_hip.h specifies for gnx_kin_pairs,
and a numpy stand-in for the device's two calls."""
import numpy as np

from geonomics_amd.sim import kin as K


def gamete(rng, g):
    """one gamete of genotype g [L][2] under free recombination: at every locus one of the two
    alleles, independently"""
    pick = rng.randint(0, 2, g.shape[0])
    return g[np.arange(g.shape[0]), pick]


def child(rng, mother, father):
    return np.stack([gamete(rng, mother), gamete(rng, father)], axis=1)


def synthetic_pedigree(seed, L=16384, n_founders=40, n_fam=8):
    """40 founders with allele frequencies p ~ U(0.1, 0.9) at L loci and, under free
    recombination, eight families: mother and father (founders), two full sibs, a half sib (the
    mother with another founder) and a grandchild (the first sib with a fresh founder).
    -> (G uint8 [n][L][2], parents int64 [n][2] as row indices (-1: founder), dict of sets of
    (a, b) with a < b: 'PO', 'FS', 'second' (half sibs, grandparents, full avuncular),
    'half_avuncular', 'unrelated' (every other pair))"""
    rng = np.random.RandomState(seed)
    assert n_founders >= 4 * n_fam
    p = rng.uniform(0.1, 0.9, L)
    G = [(rng.random_sample((L, 2)) < p[:, None]).astype(np.uint8) for _ in range(n_founders)]
    parents = [(-1, -1)] * n_founders
    rel = {k: set() for k in ('PO', 'FS', 'second', 'half_avuncular')}

    def add(kind, a, b):
        rel[kind].add((min(a, b), max(a, b)))

    def born(m, f):
        G.append(child(rng, G[m], G[f]))
        parents.append((m, f))
        add('PO', m, len(G) - 1)
        add('PO', f, len(G) - 1)
        return len(G) - 1

    for fam in range(n_fam):
        m, f, other, fresh = 4 * fam, 4 * fam + 1, 4 * fam + 2, 4 * fam + 3
        s1, s2 = born(m, f), born(m, f)
        h = born(m, other)
        g = born(s1, fresh)
        add('FS', s1, s2)
        add('second', s1, h)
        add('second', s2, h)
        add('second', m, g)
        add('second', f, g)
        add('second', s2, g)
        add('half_avuncular', h, g)
    n = len(G)
    named = set().union(*rel.values())
    rel['unrelated'] = {(a, b) for a in range(n) for b in range(a + 1, n)} - named
    return np.stack(G), np.array(parents, np.int64), rel


def labels(G, loci=None):
    """(kinship [n][n], ibs0 [n][n], relationship [n][n]) of the restatement"""
    c = K.counts_numpy(G, loci)
    nh = c['nhet']
    kin = K.king(c['hh'], c['ibs0'], nh[:, None], nh[None, :])
    return kin, c['ibs0'], K.relationship(kin, c['ibs0'])


def pair_radius(x, y):
    """r [n][n] as include/gnx_hip.h takes it: fp64 from the fp32 coordinates"""
    x = np.asarray(x, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32).astype(np.float64)
    dx, dy = x[:, None] - x[None, :], y[:, None] - y[None, :]
    return np.sqrt(dx * dx + dy * dy)


def brute_pairs(G, x, y, T, max_dist=None, loci=None):
    """gnx_kin_pairs restated: every pair a < b, candidates r < max_dist (None: all), kept by the
    integer rule, in (a, b) order
    -> dict(pa, pb, hh, ibs0, nhet, n_candidates, n_found)"""
    c = K.counts_numpy(G, loci)
    n = c['nhet'].size
    a, b = np.triu_indices(n, 1)
    cand = np.ones(a.size, bool) if max_dist is None else pair_radius(x, y)[a, b] < max_dist
    keep = cand & K.keep_rule(c['hh'][a, b], c['ibs0'][a, b], c['nhet'][a], c['nhet'][b], T)
    return dict(pa=a[keep], pb=b[keep], hh=c['hh'][a, b][keep], ibs0=c['ibs0'][a, b][keep],
                nhet=c['nhet'], n_candidates=int(cand.sum()), n_found=int(keep.sum()))


class NumpyDevice:
    """the two kinship calls of _native.Device restated in numpy over genotypes G [n][L][2] in
    slot order"""

    def __init__(self, G, x, y):
        self.G, self.x, self.y = np.asarray(G), x, y
        self.L = self.G.shape[1]
        self.W64 = (self.L + 1023) // 1024 * 16

    def _loci(self, locus_mask):
        if locus_mask is None:
            return None
        l = np.arange(self.L)
        return l[((locus_mask[l >> 6] >> (l & 63).astype(np.uint64)) & np.uint64(1)) == 1]

    def kin_matrix(self, slots=None, locus_mask=None):
        G = self.G if slots is None else self.G[slots]
        c = K.counts_numpy(G, self._loci(locus_mask))
        return dict(nhet=c['nhet'].astype(np.int32), hh=c['hh'].astype(np.int32),
                    ibs0=c['ibs0'].astype(np.int32))

    def kin_pairs(self, T, max_dist=None, slots=None, locus_mask=None, max_pairs=1 << 22,
                  max_work=0):
        from geonomics_amd import _native as nat
        s = np.arange(self.G.shape[0]) if slots is None else slots
        loci = self._loci(locus_mask)
        nw = np.unique((np.arange(self.L) if loci is None else loci) >> 6).size
        work = s.size * (s.size - 1) // 2 * nw          # (one cell: every pair)
        if work > max_work:
            raise nat.GnxError('gnx_kin_pairs: %d pair-words of work exceed max_work = %d'
                               % (work, max_work))
        got = brute_pairs(self.G[s], self.x[s], self.y[s], T, max_dist, loci)
        if got['n_found'] > max_pairs:
            err = nat.GnxError('gnx_kin_pairs: %d kept pairs exceed max_pairs = %d'
                               % (got['n_found'], max_pairs))
            err.n_found = got['n_found']
            raise err
        got.update(work=work)
        return got
