"""Close-kin pairs (csrc/gnx_kin.hip: gnx_kin_matrix, gnx_kin_pairs): KING-robust kinship
(Manichaikul et al. 2010) and the IBS0 count of pairs of individuals, the relationship they
name, and the truth of the recorded pedigree to hold them against.  Pure numpy: the device gives
the integers per individual and per pair that include/gnx_hip.h defines; what is computed here
is the kinship from them (`king`), the integer rule by which the device keeps a pair
(`threshold`, `keep_rule`), the label (`relationship`), the true relations from the parents' ids
(`pair_truth`, `pedigree_relations`), and `counts_numpy`, the numpy restatement of the device's
integers, which the tests compare the device with bit for bit.

For individual a with alleles a0, a1 at a locus: het_a = a0 != a1, P_a = a0 & a1 (homozygous 1),
O_a = a0 | a1.  nhet_a = sum het_a; hh_ab = sum het_a & het_b; ibs0_ab = sum P_a & ~O_b +
sum P_b & ~O_a (opposite homozygotes); kinship_ab = (hh_ab - 2 ibs0_ab) / (nhet_a + nhet_b).
Its expectation is 1/2 for a pair of identical genotypes, 1/4 for first-degree relatives, 1/8
for second-degree ones and 0 for unrelated individuals of one population, whatever the allele
frequencies (it uses none).  Without genotyping error a parent and its child are never opposite
homozygotes, which tells parent-offspring (ibs0 == 0) from full sibs.
"""
import math

import numpy as np

SHIFT = 20                          # the device compares with T / 2^20
# KING's published cutoffs between duplicate / first / second / third degree / unrelated
CUTOFFS = (2.0 ** -1.5, 2.0 ** -2.5, 2.0 ** -3.5, 2.0 ** -4.5)


def counts_numpy(G, loci=None):
    """the device's integers from genotypes G [n][L][2] of 0 / 1 at `loci` (all by default)
    -> dict(nhet int64 [n], hh int64 [n][n], ibs0 int64 [n][n])"""
    G = np.asarray(G)
    if G.ndim != 3 or G.shape[2] != 2:
        raise ValueError('G: genotypes [n][L][2], not %s' % (G.shape,))
    if loci is not None:
        G = G[:, np.asarray(loci, dtype=np.int64).ravel(), :]
    a0, a1 = G[:, :, 0].astype(bool), G[:, :, 1].astype(bool)
    # (float64 products of 0 / 1 are exact below 2^53 loci)
    het = (a0 ^ a1).astype(np.float64)
    P = (a0 & a1).astype(np.float64)
    N = (~(a0 | a1)).astype(np.float64)
    hh = np.rint(het @ het.T).astype(np.int64)
    M = np.rint(P @ N.T).astype(np.int64)
    return dict(nhet=np.rint(het.sum(axis=1)).astype(np.int64), hh=hh, ibs0=M + M.T)


def threshold(min_kinship):
    """the integer T the device is given for min_kinship: ceil(min_kinship 2^20)"""
    k = float(min_kinship)
    if not -1.0 <= k <= 0.5:                 # (NaN fails too)
        raise ValueError('min_kinship: a finite number in [-1, 0.5] (got %r)' % (min_kinship,))
    return int(math.ceil(k * (1 << SHIFT)))


def keep_rule(hh, ibs0, nh_a, nh_b, T):
    """the device's rule, in int64: a pair is kept iff nh_a + nh_b > 0 and
    (hh - 2 ibs0) 2^20 >= T (nh_a + nh_b)"""
    num = np.asarray(hh, dtype=np.int64) - 2 * np.asarray(ibs0, dtype=np.int64)
    den = np.asarray(nh_a, dtype=np.int64) + np.asarray(nh_b, dtype=np.int64)
    return (den > 0) & (num * (1 << SHIFT) >= int(T) * den)


def king(hh, ibs0, nh_a, nh_b):
    """KING-robust kinship in fp64; NaN where neither individual has a heterozygous locus"""
    num = (np.asarray(hh, dtype=np.int64) - 2 * np.asarray(ibs0, dtype=np.int64)) \
        .astype(np.float64)
    den = (np.asarray(nh_a, dtype=np.int64) + np.asarray(nh_b, dtype=np.int64)) \
        .astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


def relationship(kinship, ibs0, po_max_ibs0=0):
    """the label of a pair by KING's cutoffs: 'dup' above 2^-1.5, first degree from 2^-2.5 -
    'PO' iff ibs0 <= po_max_ibs0, else 'FS' -, '2nd' from 2^-3.5, '3rd' from 2^-4.5, else 'un'
    (NaN too).  Arrays in, an array of str out; scalars in, a str out"""
    k = np.asarray(kinship, dtype=np.float64)
    z = np.asarray(ibs0)
    k, z = np.broadcast_arrays(k, z)
    out = np.full(k.shape, 'un', dtype='<U3')
    with np.errstate(invalid='ignore'):
        out[k >= CUTOFFS[3]] = '3rd'
        out[k >= CUTOFFS[2]] = '2nd'
        first = (k >= CUTOFFS[1]) & (k <= CUTOFFS[0])
        out[first & (z <= po_max_ibs0)] = 'PO'
        out[first & (z > po_max_ibs0)] = 'FS'
        out[k > CUTOFFS[0]] = 'dup'
    return str(out[()]) if out.ndim == 0 else out


def pair_truth(id_a, id_b, par_a, par_b):
    """the true relation of each listed pair from the recorded parents: id_a, id_b [k] the two
    ids, par_a, par_b [k][2] their parents' ids (-1: not recorded)
    -> array of str [k]: 'PO' (one is a parent of the other), 'FS' (the same two recorded
    parents), 'HS' (one recorded parent shared) or ''"""
    id_a, id_b = np.asarray(id_a, dtype=np.int64), np.asarray(id_b, dtype=np.int64)
    pa = np.sort(np.asarray(par_a, dtype=np.int64).reshape(-1, 2), axis=1)
    pb = np.sort(np.asarray(par_b, dtype=np.int64).reshape(-1, 2), axis=1)
    out = np.full(id_a.shape, '', dtype='<U2')
    shared = np.zeros(id_a.shape, bool)
    for i in range(2):
        for j in range(2):
            shared |= (pa[:, i] >= 0) & (pa[:, i] == pb[:, j])
    out[shared] = 'HS'
    out[(pa[:, 0] >= 0) & (pa[:, 0] == pb[:, 0]) & (pa[:, 1] == pb[:, 1])] = 'FS'
    po = (pb == id_a[:, None]).any(axis=1) | (pa == id_b[:, None]).any(axis=1)
    out[po] = 'PO'
    return out


def pedigree_relations(parents, ids=None):
    """the true parent-offspring, full-sib and half-sib pairs among n individuals: parents
    int [n][2], the parents' ids (-1: not recorded); ids [n] (default 0..n-1, so that parents
    holds indices).  Every pair is looked at (n^2 / 2 of them: for samples, not populations)
    -> dict('PO', 'FS', 'HS': int64 [k][2], index pairs a < b in ascending order)"""
    parents = np.asarray(parents, dtype=np.int64).reshape(-1, 2)
    n = parents.shape[0]
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64).ravel()
    if ids.size != n:
        raise ValueError('ids: %d entries for %d rows of parents' % (ids.size, n))
    a, b = np.triu_indices(n, 1)
    rel = pair_truth(ids[a], ids[b], parents[a], parents[b])
    return {k: np.stack([a[rel == k], b[rel == k]], axis=1).astype(np.int64)
            for k in ('PO', 'FS', 'HS')}
