"""Genetic PCA's host algorithms (geonomics_amd/sim/pca.py) on the CPU.

The exact method (Gram matrix -> eigh) against the reference's method, sklearn's
PCA(svd_solver='full').fit_transform of the mean genotypes (sim/model.py:2031-2041), or the
same numpy SVD with sklearn's sign rule where sklearn is missing: scores within 1e-9 s_1,
ratios within 1e-12, wherever each of the first n_pcs singular values is at least 1 % away
from its neighbours (asserted on the oracle).  The randomized subspace iteration against the
exact SVD, with numpy products in fp64 and rounded to fp32 (the device's contract), on
planted-structure populations with s_k / s_{k+1} >= 2.5: largest principal-angle sine
<= 1e-5, singular values within 1e-6 relative."""
import numpy as np
import pytest

from geonomics_amd.sim import pca as P


def planted(n, L, demes, fst, seed):
    """dosages int64 [n][L] of a planted-structure population: per-deme allele frequencies
    Beta(p(1-F)/F, (1-p)(1-F)/F) with p ~ U(0.1, 0.9); individual i lives in deme
    i % demes (demes = 1: no structure, frequencies p)"""
    rng = np.random.RandomState(seed)
    p = rng.uniform(0.1, 0.9, L)
    if demes == 1:
        f = np.tile(p, (1, 1))
    else:
        f = rng.beta(p * (1 - fst) / fst, (1 - p) * (1 - fst) / fst, size=(demes, L))
    f = f[np.arange(n) % demes]
    return (rng.rand(n, L) < f).astype(np.int64) + (rng.rand(n, L) < f)


def reference_pca(D, n_pcs):
    """-> scores [n][n_pcs], explained_variance_ratio [n_pcs], all singular values of the
    centred mean genotypes"""
    X = D / 2.0
    U, s, Vt = np.linalg.svd(X - X.mean(axis=0), full_matrices=False)
    try:
        from sklearn.decomposition import PCA
    except ImportError:
        PCA = None
    if PCA is not None:
        pca = PCA(n_components=n_pcs, svd_solver='full')
        return pca.fit_transform(X), pca.explained_variance_ratio_, s
    # sklearn's svd_flip(u_based_decision=False): the largest |loading| of a component > 0
    V = Vt[:n_pcs]
    sg = np.sign(V[np.arange(n_pcs), np.argmax(np.abs(V), axis=1)])
    return U[:, :n_pcs] * s[:n_pcs] * sg, s[:n_pcs] ** 2 / (s ** 2).sum(), s


def assert_gaps(s, n_pcs, rel=0.01):
    """each of the first n_pcs singular values at least `rel` away from its neighbours"""
    for k in range(n_pcs):
        assert s[k] >= (1 + rel) * s[k + 1], ('no gap at component %d: %r' % (k, s[:n_pcs + 1]))


def max_sine(A, B):
    """sine of the largest principal angle between the column spans of A and B"""
    qa = np.linalg.qr(A)[0]
    qb = np.linalg.qr(B)[0]
    return np.linalg.norm(qb - qa @ (qa.T @ qb), 2)


# (n, L, demes, Fst, seed, n_pcs): 3 demes, none (no structure), 4 demes, and the 8192 cap
EXACT_POPS = [(600, 400, 3, 0.05, 1, 3), (300, 200, 1, 0.0, 2, 2),
              (3000, 2000, 4, 0.02, 4, 3), (8192, 300, 4, 0.03, 3, 3)]


@pytest.mark.parametrize('pop', EXACT_POPS, ids=lambda p: '%dx%d_d%d' % p[:3])
def test_pca_from_gram_matches_reference(pop):
    n, L, demes, fst, seed, n_pcs = pop
    D = planted(n, L, demes, fst, seed)
    ref, ref_ratio, s = reference_pca(D, n_pcs)
    assert_gaps(s, n_pcs)
    Df = D.astype(np.float64)
    G = (Df @ Df.T).astype(np.int64)            # exact: integer entries below 2^53
    scores, ratio = P.pca_from_gram(G, n_pcs, rmatmul=lambda U: Df.T @ U)
    err = np.abs(scores - ref).max()
    print('%s: max score error %.3g s_1, ratio error %.3g' % (pop, err / s[0],
                                                              np.abs(ratio - ref_ratio).max()))
    assert err <= 1e-9 * s[0]
    assert np.abs(ratio - ref_ratio).max() <= 1e-12


def _products(D, fp32):
    Df = D.astype(np.float64)
    if not fp32:
        return (lambda M: Df @ M), (lambda Y: Df.T @ Y)
    r = lambda a: np.asarray(a, np.float32).astype(np.float64)      # noqa: E731
    return (lambda M: r(Df @ r(M))), (lambda Y: r(Df.T @ r(Y)))


# (n, L, demes, Fst, seed): n_pcs = demes - 1 planted components
RAND_POPS = [(3000, 2000, 4, 0.05, 5), (20000, 1000, 4, 0.02, 6), (4000, 4096, 3, 0.03, 7)]


@pytest.mark.parametrize('fp32', [False, True], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('pop', RAND_POPS, ids=lambda p: '%dx%d_d%d' % p[:3])
def test_randomized_pca_matches_exact_svd(pop, fp32):
    n, L, demes, fst, seed = pop
    n_pcs = demes - 1
    D = planted(n, L, demes, fst, seed)
    X = D / 2.0
    U, s, _ = np.linalg.svd(X - X.mean(axis=0), full_matrices=False)
    assert s[n_pcs - 1] >= 2.5 * s[n_pcs], s[:n_pcs + 1]
    mm, rm = _products(D, fp32)
    scores, ratio = P.randomized_pca(mm, rm, D.mean(axis=0), n, L, n_pcs, oversample=10,
                                     n_iter=8, seed=0, sumsq=(D * D).sum(axis=0))
    sine = max_sine(U[:, :n_pcs], scores)
    s_got = np.linalg.norm(scores, axis=0)
    rel = np.abs(s_got - s[:n_pcs]) / s[:n_pcs]
    r_err = np.abs(ratio - s[:n_pcs] ** 2 / (s ** 2).sum()).max()
    print('%s fp32=%s: sine %.3g, singular value error %.3g, ratio error %.3g'
          % (pop, fp32, sine, rel.max(), r_err))
    assert sine <= 1e-5
    assert rel.max() <= 1e-6
    # the exact total variance: the ratio carries the singular values' error only
    assert r_err <= 2.0 * rel.max() * ratio.max() + 1e-12


def test_randomized_pca_follows_the_sign_rule():
    D = planted(1500, 800, 4, 0.05, 8)
    mm, rm = _products(D, False)
    scores, _ = P.randomized_pca(mm, rm, D.mean(axis=0), 1500, 800, 3, sumsq=(D * D).sum(0))
    ref, _, s = reference_pca(D, 3)
    assert_gaps(s, 3)
    # same direction as the reference's component (not its mirror image)
    assert ((scores * ref).sum(axis=0) > 0.99 * (ref * ref).sum(axis=0)).all()


def test_argument_validation():
    D = planted(50, 30, 2, 0.05, 9)
    Df = D.astype(np.float64)
    G = (Df @ Df.T).astype(np.int64)
    for bad in (0, -1, 50, 2.5, True):
        with pytest.raises(ValueError):
            P.pca_from_gram(G, bad)
    with pytest.raises(ValueError):
        P.pca_from_gram(G[:, :10], 2)
    mm, rm = _products(D, False)
    mu, sq = D.mean(0), (D * D).sum(0)
    for bad in (0, 31, 55):          # > n_loci, > 64 - oversample
        with pytest.raises(ValueError):
            P.randomized_pca(mm, rm, mu, 50, 30, bad, sumsq=sq)
    with pytest.raises(ValueError):
        P.randomized_pca(mm, rm, mu, 50, 30, 3, oversample=62, sumsq=sq)
    with pytest.raises(ValueError):
        P.randomized_pca(mm, rm, mu, 50, 30, 3)             # no total variance
    with pytest.raises(ValueError):
        P.randomized_pca(mm, rm, mu, 50, 30, 3, n_iter=-1, sumsq=sq)
    P.check_n_pcs(54, 100, 1000, oversample=10)
    with pytest.raises(ValueError):
        P.check_n_pcs(55, 100, 1000, oversample=10)
