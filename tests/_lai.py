"""The cases tests/test_lai_host.py and tests/test_gpu_lai.py share (geonomics_amd/sim/lai.py,
csrc/gnx_lai.hip).  Every case is a dict of what gnx_lai_paint takes, the phased bits X
[n][L][2] of the population it is painted on, and - computed once - the restatement's result.

A  n = 70 individuals (140 haplotypes: two full waves and 12 lanes), L = 200 (three words and 8
   bits), K = 3, F uniform in [0.05, 0.95], Dirichlet priors, sw = 10^U(-3, 0) with sw = 1 at
   loci 0 and 97 (a break).
B  the same n, L and genomes at K = 1, 2 and 8.
C  case A's model on 61 used loci that skip the whole of word 1, a population of 131 of which 40
   rows are painted in a shuffled order, and `by` with G = 3 and some -1 labels.
D  the planted mosaic: 60 individuals, L = 3000, K = 2, Balding-Nichols frequencies (Fst 0.2
   around p ~ U(0.1, 0.9)), 1 Morgan of uniform map, 10 generations, Dirichlet(1, 1) ancestry.

The genomes reach a device through test_gpu_mmrr._handle, which takes dosages and gives
homologue 0 the bit d >= 1 and homologue 1 the bit d == 2: cases A - C draw dosages and take X
from them in that way.  Case D needs its own phase, so each of its haplotypes is uploaded as a
homozygous individual (dosage 2 x) and homologue 0 of every such individual is read.
"""
import functools

import numpy as np

from geonomics_amd.sim import lai as LAI


def bits_of_dosages(D):
    """the phased bits test_gpu_mmrr._handle uploads for dosages D [n][L] -> uint8 [n][L][2]"""
    return np.stack([D >= 1, D == 2], axis=2).astype(np.uint8)


def _dosages(rng, n, L):
    return rng.binomial(2, rng.uniform(0.1, 0.9, L), size=(n, L))


def _model(rng, n, L_u, K, breaks=(0,)):
    F = rng.uniform(0.05, 0.95, (L_u, K))
    Q = rng.dirichlet(np.ones(K), size=n)
    sw = 10.0 ** rng.uniform(-3.0, 0.0, L_u)
    sw[list(breaks)] = 1.0
    return F, Q, sw, 1.0 - sw


def _finish(case):
    """the restatement over the rows and loci the case paints"""
    X = case['X']
    if case['slots'] is not None:
        X = X[case['slots']]
    if case['loci'] is not None:
        X = X[:, case['loci'], :]
    case['X_used'] = X
    case['ref'] = LAI.brute_paint(X, case['F'], case['sw'], case['stay'], case['Q'], case['by'],
                                  case['n_groups'], want_gamma=True)
    return case


@functools.lru_cache(maxsize=None)
def dosages_a():
    """the dosages of cases A and B [70][200]"""
    return _dosages(np.random.RandomState(41), 70, 200)


@functools.lru_cache(maxsize=None)
def case_a():
    D = dosages_a()
    F, Q, sw, stay = _model(np.random.RandomState(42), 70, 200, 3, breaks=(0, 97))
    return _finish(dict(name='A', D=D, X=bits_of_dosages(D), F=F, Q=Q, sw=sw, stay=stay,
                        slots=None, loci=None, by=None, n_groups=0))


@functools.lru_cache(maxsize=None)
def case_b(K):
    D = dosages_a()
    F, Q, sw, stay = _model(np.random.RandomState(50 + K), 70, 200, K, breaks=(0, 97))
    return _finish(dict(name='B%d' % K, D=D, X=bits_of_dosages(D), F=F, Q=Q, sw=sw, stay=stay,
                        slots=None, loci=None, by=None, n_groups=0))


@functools.lru_cache(maxsize=None)
def case_c():
    rng = np.random.RandomState(43)
    D = _dosages(rng, 131, 200)
    pool = np.r_[np.arange(0, 64), np.arange(128, 200)]        # none of word 1
    loci = np.sort(rng.choice(pool, 61, replace=False)).astype(np.int64)
    assert (loci < 64).any() and (loci >= 128).any()
    slots = rng.permutation(131)[:40].astype(np.int64)
    F, Q, sw, stay = _model(rng, 40, 61, 3, breaks=(0, 30))
    by = rng.randint(-1, 3, 40).astype(np.int32)
    assert set(np.unique(by)) == {-1, 0, 1, 2}
    return _finish(dict(name='C', D=D, X=bits_of_dosages(D), F=F, Q=Q, sw=sw, stay=stay,
                        slots=slots, loci=loci, by=by, n_groups=3))


def planted_mosaic(n=60, L=3000, K=2, fst=0.2, morgans=1.0, gens=10.0, seed=3):
    """frequencies: Balding-Nichols draws around p ~ U(0.1, 0.9); a uniform map of `morgans`;
    per individual a Dirichlet(1) ancestry q; each haplotype's ancestry is drawn from q at locus
    0 and drawn anew from q between loci with probability -expm1(-gens d); alleles are
    Bernoulli(f)
    -> dict(X uint8 [n][L][2], Z uint8 [n][L][2] (the truth), F [L][K], Q [n][K], pos [L], gens)"""
    rng = np.random.RandomState(seed)
    p = rng.uniform(0.1, 0.9, L)
    c = (1.0 - fst) / fst
    F = LAI.clip_freqs(rng.beta(p * c, (1.0 - p) * c, size=(K, L)).T)
    pos = np.linspace(0.0, morgans, L)
    sw, _ = LAI.switch_probs(pos, gens)
    Q = rng.dirichlet(np.ones(K), size=n)
    Z = np.zeros((n, L, 2), np.uint8)
    for i in range(n):
        for h in range(2):
            redraw = rng.random_sample(L) < sw                 # (sw[0] = 1: locus 0 draws)
            fresh = rng.choice(K, size=L, p=Q[i])
            last = np.maximum.accumulate(np.where(redraw, np.arange(L), 0))
            Z[i, :, h] = fresh[last]
    f_z = F[np.arange(L)[None, :, None], Z]
    X = (rng.random_sample((n, L, 2)) < f_z).astype(np.uint8)
    return dict(X=X, Z=Z, F=F, Q=Q, pos=pos, gens=float(gens))


@functools.lru_cache(maxsize=None)
def case_d():
    """the planted mosaic and the restatement's painting of it under the true F, priors and
    gens (ref) and under a uniform prior (ref_uniform)"""
    m = planted_mosaic()
    sw, stay = LAI.switch_probs(m['pos'], m['gens'])
    m.update(sw=sw, stay=stay)
    m['ref'] = LAI.brute_paint(m['X'], m['F'], sw, stay, m['Q'])
    m['ref_uniform'] = LAI.brute_paint(m['X'], m['F'], sw, stay, np.full(m['Q'].shape, 0.5))
    return m


def as_homozygotes(X):
    """the dosages whose upload by _handle puts haplotype t = 2 i + h of X on both homologues of
    individual t -> [2n][L]"""
    n, L, _ = X.shape
    return 2 * X.transpose(0, 2, 1).reshape(2 * n, L).astype(np.int64)


def recovery(res, Z, Q):
    """(share of haplotype-loci called correctly, mean |Q_local - true|) of a painting dict with
    calls [2n][L] and anc_hap [2n][K]; the truth's Q_local is the share of the true mosaic"""
    n, L, _ = Z.shape
    K = Q.shape[1]
    truth = Z.transpose(0, 2, 1).reshape(2 * n, L)
    acc = float((res['calls'] == truth).mean())
    q_local = 0.5 * (res['anc_hap'][0::2] + res['anc_hap'][1::2]) / L
    q_true = np.stack([(Z == k).mean(axis=(1, 2)) for k in range(K)], axis=1)
    return acc, float(np.abs(q_local - q_true).mean())
