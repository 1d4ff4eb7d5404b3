"""The per-individual columns a step carries from slot to slot - e, z, fit - checked against
the oracle in plain numpy, f64.

Selection never reads a genome row: an offspring's alleles at the selected loci are blended
from its parents' compact table, its phenotype comes from those words, its fitness from e, z
and the deleterious bits of the table, and from then on the cell sort, the compactions and the
tile staging carry all of it along without recomputing anything.  `check_columns` recomputes
every one of them from what cannot be stale: the position, the rasters and the genome row.

An architecture is a dict:
    traits      list of dict(loci, alpha, layer, phi, gamma, univ_adv); phi a scalar or an
                [H][W] raster (the value at the individual's cell counts)
    dom         None or uint8 [L]
    delet_loci  int [n_delet] (may be empty), delet_s float [n_delet]
"""
import numpy as np

import gnx_oracle as O


def ulp32(ref):
    """one f32 ulp at the f64 reference value, plus 1e-14 for sums that cancel to ~0.

    The device accumulates in f64 in the oracle's order and rounds to f32 once.  A contracted
    multiply-add or a libm pow that differs in the last f64 bits moves the f64 value by
    ~1e-16 per term, which can only flip that one rounding: half an ulp for the rounding,
    half for the flip."""
    return np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64) \
        + 1e-14


def delet_counts(geno, loci):
    """number of 1-alleles (0, 1, 2) at `loci` of packed genomes [N][2][W64] -> int [N][n]"""
    loci = np.asarray(loci, dtype=np.int64)
    w = loci >> 6
    b = (loci & 63).astype(np.uint64)
    a0 = (geno[:, 0, :][:, w] >> b) & np.uint64(1)
    a1 = (geno[:, 1, :][:, w] >> b) & np.uint64(1)
    return (a0 + a1).astype(np.int64)


def fitness_ref(e, z, cx, cy, geno, arch):
    """w of ops/selection.py:51-125 as death_prob_one composes it, f64 [N]: the traits'
    product clipped at 0.001 (no clip without traits), then the deleterious product.
    e [n_layers][N] and z [n_traits][N] are the device's own f32 columns."""
    N = geno.shape[0]
    traits = arch['traits']
    w = np.ones(N)
    if traits:
        phi = [np.asarray(t['phi'], np.float32).astype(np.float64)[cy, cx]
               if np.ndim(t['phi']) == 2 else float(t['phi']) for t in traits]
        w = O.fitness_traits(np.asarray(e, np.float64).T, np.asarray(z, np.float64).T,
                             [t['layer'] for t in traits], phi,
                             [t['gamma'] for t in traits], [t['univ_adv'] for t in traits])
    if len(arch['delet_loci']):
        cnt = delet_counts(geno, arch['delet_loci'])
        w = w * (1.0 - cnt * np.asarray(arch['delet_s'], np.float64)).prod(axis=1)
    return w


def _first_bad(bad, ids):
    k = np.nonzero(bad)[0]
    return k[np.argmin(ids[k])]


def check_columns(cols, rasts, arch, check_fit):
    """cols: dict(ids [N], x [N], y [N], e [n_layers][N], z [n_traits][N], fit [N],
    geno uint64 [N][2][W64]) in any slot order; rasts f32 [n_layers][H][W].

    ids unique; e == the raster at the cell, exactly; z within one f32 ulp of
    O.phenotype_packed of the genome row; with check_fit, fit within one f32 ulp of the
    oracle's fitness of the device's own e and z and of the row's deleterious bits.
    (fit is that of the last death pass: valid for everybody alive at the end of a step that
    ran with selection, stale after set_z or a mutation until the next step.)"""
    ids = np.asarray(cols['ids'])
    N = ids.size
    x, y = np.asarray(cols['x']), np.asarray(cols['y'])
    e, z, fit, geno = (np.asarray(cols[k]) for k in ('e', 'z', 'fit', 'geno'))
    rasts = np.asarray(rasts, np.float32)
    traits = arch['traits']
    assert x.shape == y.shape == fit.shape == (N,) and geno.shape[0] == N
    assert e.shape == (rasts.shape[0], N) and z.shape == (len(traits), N)
    u, cnt = np.unique(ids, return_counts=True)
    assert u.size == N, 'ids: id %d is held by %d slots' % (u[cnt > 1][0], cnt[cnt > 1][0])
    if N == 0:
        return
    cx, cy = x.astype(np.int64), y.astype(np.int64)
    for l in range(rasts.shape[0]):
        ref = rasts[l][cy, cx]
        bad = e[l] != ref
        if bad.any():
            k = _first_bad(bad, ids)
            raise AssertionError('id %d: e of layer %d is %.9g, the raster at its cell (%d, %d) '
                                 'has %.9g (%d of %d individuals differ)'
                                 % (ids[k], l, e[l][k], cx[k], cy[k], ref[k], bad.sum(), N))
    rows = np.arange(N)
    for t, tr in enumerate(traits):
        ref = O.phenotype_packed(geno, rows, tr['loci'], tr['alpha'], arch['dom'])
        bad = ~(np.abs(z[t].astype(np.float64) - ref) <= ulp32(ref))
        if bad.any():
            k = _first_bad(bad, ids)
            raise AssertionError('id %d: z of trait %d is %.9g, the oracle computes %.17g from its '
                                 'genome (%d of %d individuals differ)'
                                 % (ids[k], t, z[t][k], ref[k], bad.sum(), N))
    if check_fit:
        ref = fitness_ref(e, z, cx, cy, geno, arch)
        bad = ~(np.abs(fit.astype(np.float64) - ref) <= ulp32(ref))
        if bad.any():
            k = _first_bad(bad, ids)
            raise AssertionError('id %d: fit is %.9g, the oracle computes %.17g from its e, z and '
                                 'deleterious alleles (%d of %d individuals differ)'
                                 % (ids[k], fit[k], ref[k], bad.sum(), N))
