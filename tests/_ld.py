"""What tests/test_ld_host.py and tests/test_gpu_ld.py share: the chromosome-major bit matrix of
a genotype array, the fixture g22_ld.npz, the any-order bound of the device's fp64 sums, and a
numpy Wright-Fisher population to try the estimator on.  The restatement of gnx_ld_bins itself
is geonomics_amd/sim/ld.brute_bins."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
U53 = 2.0 ** -53
SUMS = ('sum_r2', 'sum_r4', 'sum_d', 'sum_w')
# units of 2^-53 per term granted beside the m of the any-order sum and the 1 of the oracle's
# rounding: r2, r2 r2 and d are bit-equal on both sides; w carries the two expm1 (each within
# 1 ulp = 2 units of the true value: 4)
C_TERM = {'sum_r2': 1, 'sum_r4': 1, 'sum_d': 1, 'sum_w': 5}


def bits_of(gts):
    """genotypes [n][L][2] -> bits [2 n][L]: chromosome 2 i + h is homologue h of individual i"""
    gts = np.asarray(gts)
    return gts.transpose(0, 2, 1).reshape(2 * gts.shape[0], gts.shape[1])


def fixture():
    with np.load(os.path.join(HERE, 'golden', 'g22_ld.npz')) as z:
        return {k: z[k] for k in z.files}


def sum_bounds(ref):
    """{name: bound [n_bins]} of |S - S_ref| for the four fp64 sums: (m + c) 2^-53 sum |term|;
    every term is >= 0, so sum |term| is the oracle's sum itself (inf stays inf)"""
    m = ref['pairs'].astype(np.float64)
    return {k: (m + C_TERM[k]) * U53 * ref[k] for k in SUMS}


def wright_fisher(N, L, r, gens, seed):
    """bits [2 N][L] of a monoecious Wright-Fisher population of N diploids after `gens`
    generations: every offspring draws two parents with replacement; a gamete starts on a random
    homologue of its parent and switches before locus l with probability r (r_0 unused), as the
    simulator's recombination paths do.  Founders: independent loci at frequency 0.5"""
    rng = np.random.RandomState(seed)
    pop = (rng.rand(N, 2, L) < 0.5).astype(np.uint8)
    cols = np.arange(L)[None, :]
    for _ in range(gens):
        par = rng.randint(0, N, size=(N, 2))
        sw = rng.rand(N, 2, L) < r
        sw[:, :, 0] = rng.rand(N, 2) < 0.5
        hom = np.cumsum(sw, axis=2) & 1
        new = np.empty_like(pop)
        for g in range(2):
            new[:, g, :] = pop[par[:, g][:, None], hom[:, g, :], cols]
        pop = new
    return pop.reshape(2 * N, L)
