"""The cases the association-scan tests share (tests/test_assoc_host.py on the CPU,
tests/test_gpu_assoc.py on the device): the planted landscape-genomic case, the dosages and
columns of the cross-product cases, and a per-locus least-squares fit that knows nothing of
sim/assoc.py.  Everything is generated from seeds; results are cached and must not be changed."""
import functools

import numpy as np

CAUSAL = 13 + 97 * np.arange(6)

# (n, L, m) of the cross-product cases.  With AS_TI = 64 individuals per tile and at most 32
# stretches (include/gnx_hip.h): n = 1 is one ragged tile; 127 and 129 are two and three tiles, a
# stretch each, the last ragged; L = 63, 65, 1025 and 1100 leave padding bits in the last word
# (and 1025, 1100 a second line of 1024 loci); m = 16, 17 and 32 are one block of 16 columns,
# three of 8 and two of 16; n = 5125 at L = 70 is 81 tiles in 27 stretches of 3 tiles (192
# individuals), the last one of 133 individuals
CROSS_SHAPES = [(1, 1, 1), (127, 63, 1), (129, 65, 16), (300, 1025, 17), (257, 1100, 32),
                (5125, 70, 3)]


def random_dosages(n, L, seed):
    rng = np.random.RandomState(seed)
    p = rng.uniform(0.05, 0.95, L)
    return ((rng.uniform(size=(n, L)) < p).astype(np.int64)
            + (rng.uniform(size=(n, L)) < p).astype(np.int64))


def mixed_columns(n, m, seed):
    """Y [n][m]: mixed signs, magnitudes spanning 10^6 within every column, the columns' scales
    differing too, and column m // 2 all zero (when m > 1)"""
    rng = np.random.RandomState(seed)
    Y = rng.standard_normal((n, m)) * 10.0 ** rng.uniform(-3, 3, size=(n, m))
    Y *= 10.0 ** rng.uniform(-2, 2, size=m)
    if m > 1:
        Y[:, m // 2] = 0.0
    return Y


@functools.lru_cache(maxsize=None)
def cross_case(n, L, m):
    """(D [n][L], Y [n][m]) of one shape"""
    D = random_dosages(n, L, 1000 + n + L)
    Y = mixed_columns(n, m, 2000 + n + m)
    D.setflags(write=False)
    Y.setflags(write=False)
    return D, Y


@functools.lru_cache(maxsize=None)
def planted():
    """two demes with drifted frequencies, an environment that differs between them, and six
    loci whose frequency follows the environment
    -> dict(D [400][600], env [400], deme [400], causal)"""
    rng = np.random.RandomState(7)
    n, L = 400, 600
    deme = np.arange(n) % 2
    pa = rng.uniform(0.1, 0.9, L)
    delta = rng.normal(0.0, 0.15, L)
    P = np.clip(pa[None, :] + np.where(deme[:, None] == 1, 1.0, -1.0) * delta[None, :],
                0.02, 0.98)
    env = deme + rng.normal(0.0, 1.0, n)
    for l in CAUSAL:
        P[:, l] = np.clip(pa[l] + 0.22 * (env - env.mean()), 0.02, 0.98)
    D = ((rng.uniform(size=(n, L)) < P).astype(np.int64)
         + (rng.uniform(size=(n, L)) < P).astype(np.int64))
    D.setflags(write=False)
    env.setflags(write=False)
    return dict(D=D, env=env, deme=deme, causal=CAUSAL.copy())


def top_by_abs_t(t, k):
    """the k loci of largest |t| (NaN last), sorted"""
    a = np.where(np.isnan(t), -1.0, np.abs(t))
    return np.sort(np.argsort(-a, kind='stable')[:k])


def lstsq_gwas(D, C, X):
    """per locus and tested variable x: the coefficient of g and its t in the least-squares fit
    of x on [1, C, g] -> (beta [L][r], t [L][r])"""
    return _lstsq(D, C, X, True)


def lstsq_gea(D, C, X):
    """per locus and tested variable x: the coefficient of x and its t in the least-squares fit
    of g on [1, C, x] -> (beta [L][r], t [L][r])"""
    return _lstsq(D, C, X, False)


def _lstsq(D, C, X, g_is_regressor):
    n, L = D.shape
    r = X.shape[1]
    beta, t = np.zeros((L, r)), np.zeros((L, r))
    for l in range(L):
        g = D[:, l].astype(np.float64)
        for k in range(r):
            reg, resp = (g, X[:, k]) if g_is_regressor else (X[:, k], g)
            A = np.column_stack([np.ones(n), C, reg])
            coef = np.linalg.lstsq(A, resp, rcond=None)[0]
            res = resp - A @ coef
            s2 = res @ res / (n - A.shape[1])
            cov = s2 * np.linalg.inv(A.T @ A)
            beta[l, k] = coef[-1]
            t[l, k] = coef[-1] / np.sqrt(cov[-1, -1])
    return beta, t
