"""Fixture for the linkage-disequilibrium restatement (geonomics_amd/sim/ld.py, brute_bins;
reference sim/stats.py:359-390, _calc_ld).

Runs only where the reference is readable (as make_golden.py); nothing under tests/ imports it
at test time.  The reference's sim/stats.py is parsed with ast and only the function definition
_calc_ld is compiled, at run time, into a namespace holding numpy; it is then called on a
stand-in Species exposing what it reads: _get_genotypes() and gen_arch.L.

The sample: n = 37 individuals (74 chromosomes: one full word of 64 and 10 bits), L = 26 loci -
locus 3 fixed at 0 and locus 17 fixed at 1 (the reference's r^2 is NaN for every pair with
either), locus 9 a singleton, loci 11 and 12 in complete LD, the rest at frequencies 0.1..0.9
with blocks of correlated neighbours.  Stored (only data): genotypes uint8 [n][L][2], the
reference's r2 [L][L] (NaN on the diagonal and for monomorphic loci), edges of bins of locus
separation and per bin the number of finite pairs i < j and their mean r^2.

    python tests/golden/make_ld_fixture.py   ->  tests/golden/g22_ld.npz
"""
import ast
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF_ROOT   # noqa: E402  (where the reference lives)

REF_STATS = os.path.join(REF_ROOT, 'geonomics', 'sim', 'stats.py')
EDGES = np.array([1.0, 2.0, 4.0, 8.0, 26.0])


def reference_calc_ld():
    with open(REF_STATS) as f:
        tree = ast.parse(f.read(), REF_STATS)
    defs = [node for node in tree.body
            if isinstance(node, ast.FunctionDef) and node.name == '_calc_ld']
    assert len(defs) == 1
    ns = {'np': np}
    exec(compile(ast.Module(body=defs, type_ignores=[]), REF_STATS, 'exec'), ns)
    return ns['_calc_ld']


class _GenArch:
    def __init__(self, L):
        self.L = L


class _Species:
    def __init__(self, gts):
        self.gts, self.gen_arch = gts, _GenArch(gts.shape[1])

    def _get_genotypes(self):
        return self.gts


def sample(seed=22):
    rng = np.random.RandomState(seed)
    n, L = 37, 26
    p = rng.uniform(0.1, 0.9, L)
    bits = (rng.rand(2 * n, L) < p).astype(np.uint8)
    for l in (5, 6, 7, 20, 21):                 # correlated neighbours: copy most chromosomes
        same = rng.rand(2 * n) < 0.8
        bits[same, l] = bits[same, l - 1]
    bits[:, 3], bits[:, 17] = 0, 1
    bits[:, 9] = 0
    bits[13, 9] = 1
    bits[:, 12] = bits[:, 11]
    return bits.reshape(n, 2, L).transpose(0, 2, 1).copy()      # [n][L][2]


def main():
    calc_ld = reference_calc_ld()
    gts = sample()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)         # 0 / 0 at monomorphic loci
        r2 = np.asarray(calc_ld(_Species(gts.astype(np.int8))), dtype=np.float64)
    L = gts.shape[1]
    assert r2.shape == (L, L) and np.isnan(np.diag(r2)).all()
    i, j = np.triu_indices(L, 1)
    v, sep = r2[i, j], (j - i).astype(np.float64)
    pairs = np.zeros(EDGES.size - 1, np.int64)
    mean = np.full(EDGES.size - 1, np.nan)
    for k in range(EDGES.size - 1):
        s = (sep >= EDGES[k]) & (sep < EDGES[k + 1]) & np.isfinite(v)
        pairs[k] = s.sum()
        mean[k] = v[s].mean()
    print('finite pairs per bin', pairs, 'mean r2', mean)
    np.savez_compressed(os.path.join(HERE, 'g22_ld.npz'), genotypes=gts, r2=r2, edges=EDGES,
                        pairs=pairs, mean_r2=mean)
    print('wrote g22_ld.npz: n = %d, L = %d' % gts.shape[:2])


if __name__ == '__main__':
    main()
