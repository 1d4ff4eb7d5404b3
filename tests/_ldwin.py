"""What tests/test_ldwin_host.py and tests/test_gpu_ldwin.py share: the cases of the issue as
numpy arrays, the any-order bound of a locus' score, and the two properties of a greedy choice of
independent loci.  The restatement of gnx_ld_window itself is
geonomics_amd/sim/ldwin.brute_window."""
import numpy as np

from _ld import U53
from geonomics_amd.sim import ld as LD


def case_a():
    """test_gpu_ld._case_a: 131 individuals (262 chromosomes: four full words and 6 bits), L =
    130 (two full tiles and 2 loci); two zero rates (tied positions: 39, 40, 41) and one 0.5 (a
    break before locus 90); loci 5 and 129 monomorphic, locus 70 a singleton
    -> (dosages D [131][130], map positions [130])"""
    rng = np.random.RandomState(16)
    n, L = 131, 130
    D = rng.binomial(2, rng.uniform(0.1, 0.9, L), size=(n, L))
    D[:, 5], D[:, 129] = 0, 2
    D[:, 70] = 0
    D[17, 70] = 1
    rates = rng.uniform(0.001, 0.05, L)
    rates[0] = rates[40] = rates[41] = 0.0
    rates[90] = 0.5
    return D, LD.map_positions(rates)


def gts_of(D):
    """the genotypes test_gpu_mmrr._handle uploads for dosages D"""
    return np.stack([D >= 1, D == 2], axis=2).astype(np.uint8)


def gts_of_bits(bits):
    """bits [2 n][L] -> genotypes [n][L][2], the inverse of _ld.bits_of"""
    bits = np.asarray(bits)
    return bits.reshape(bits.shape[0] // 2, 2, bits.shape[1]).transpose(0, 2, 1).astype(np.uint8)


def score_bound(ref):
    """|score - score_ref| <= (m_j + 1) 2^-53 score_ref[j]: m_j units for the m_j non-negative,
    bit-equal terms added in any order and one for the restatement's correctly rounded sum"""
    return (ref['partners'].astype(np.float64) + 1.0) * U53 * ref['score']


def check_independent(keep, claimed, rank, adj):
    """the two properties of greedy_independent on the symmetric boolean adjacency adj: no two
    kept loci share an edge; every removed locus has a kept neighbour of earlier rank, and the
    one that claimed it is the earliest of them"""
    kept = np.flatnonzero(keep)
    assert not adj[np.ix_(kept, kept)].any()
    for v in np.flatnonzero(~keep).tolist():
        nb = kept[adj[v, kept]]
        assert nb.size and rank[nb].min() < rank[v]
        assert claimed[v] == nb[np.argmin(rank[nb])]
    assert (claimed[kept] == -1).all()
