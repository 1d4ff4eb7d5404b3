"""The law of every random draw of the step, checked on the oracle's restatement of the device
samplers (oracle/gnx_draws.py: the same Philox words through the same f32 formulas as
csrc/gnx_rng.h), and the checker of tests/_distributions.py itself: it agrees with scipy.stats
where scipy is importable, and it is sharp - a 5 % error of a parameter exceeds the bound.
tests/test_gpu_distributions.py asserts the same of the device's own draws.  No GPU.

STATISTICS (sqrt(n) D_n at n = 50 000, bound 1.95).

On the commit before the fix this file failed in these places and passed everywhere else:
  von Mises kappa = 1e-5, 1e-4, 3.2e-4   all 50 000 angles NaN (rho = 0, s = inf)
  wald (100, 0.1)                        208 distances <= 0, sqrt(n) D = 8.3
  wald (50, 0.01)                        4067 distances <= 0, sqrt(n) D = 43
  births_draws                           lambda = 26.5 accepted
(and, in a first version that tested the dispersal's uniform angles attempt by attempt, one of
those 88 extra tests at 2.04: see test_oracle_distance_follows_its_law).  Passing rows then:
von Mises 0.53 - 1.47 (kappa 0 / 5e-9 / 5e-6 / 1e-3 / 1e-2 / 0.5 / 4 / 50 / 700: 1.11, 0.94, 0.53,
0.68, 0.91, 0.74, 0.73, 0.72, 1.08; (3, 2.5) 1.47, (-3.1, 12) 0.78, (7, 1) 0.73), lognormal 0.59 /
1.27 / 1.46 (dispersal attempts <= 1.83), wald (1.5, 2) 0.92, (0.1, 10) 1.10, (5, 0.1) 0.70,
(30, 0.1) 1.32, levy 0.90; Poisson chi2 / critical 1.8 / 11.2, 3.7 / 16.6, 5.5 / 20.8,
10.1 / 33.1, 20.5 / 52.7, 43.8 / 70.8 for lambda 0.05 ... 26.
With the fix: kappa 1e-5 / 1e-4 / 3.2e-4 / 1e-3 give 0.70 / 1.04 / 1.06 / 0.66, wald (30, 0.1)
1.03, (100, 0.1) 0.48, (50, 0.01) 1.36, levy (2, 5) 0.80; no distance <= 0; the rest unchanged
(the wald rows move in the third digit).  The wrong laws of the sharpness test: 5.67, 19.9, 2.93,
3.79, 2.45, 3.66.
"""
import math
import warnings

import numpy as np
import pytest

import gnx_draws as D
import _distributions as T
from _distributions import (KS_BOUND, N_DRAWS, STEP, VONMISES_CASES, DISTANCE_CASES,
                            POISSON_LAMBDAS, case_seed, case_ids)

IDS = case_ids()


# ------------------------------------------------------------------ a. the checker against scipy
def test_distance_cdfs_agree_with_scipy():
    st = pytest.importorskip('scipy.stats')
    q = np.concatenate([[1e-9, 1e-6], np.linspace(1e-3, 0.999, 500), [1 - 1e-6, 1 - 1e-9]])
    for distr, p1, p2 in DISTANCE_CASES:
        ref = {'lognormal': lambda: st.lognorm(s=p2, scale=math.exp(p1)),
               'wald': lambda: st.invgauss(mu=p1 / p2, scale=p2),
               'levy': lambda: st.levy(loc=p1, scale=p2)}[distr]()
        if distr == 'wald':            # (scipy's wald quantile gives up in the far tails)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)
                x = ref.ppf(q[2:-2])
            x = x[np.isfinite(x) & (x > 0)]
            x = np.concatenate([x[0] * np.array([0.1, 0.3, 0.6]), x, x[-1] * np.array([2, 5, 20])])
        else:
            x = ref.ppf(q)
        x = np.concatenate([x[np.isfinite(x)], [p1 if distr == 'levy' else 0.0, -1.0]])
        err = np.abs(T.distance_cdf(distr, p1, p2)(x) - ref.cdf(x)).max()
        assert err <= 1e-9, (distr, p1, p2, err)


def test_vonmises_cdf_agrees_with_scipy():
    """Below kappa = 50 scipy.stats.vonmises.cdf sums the series and is exact to rounding.  From
    kappa = 50 it switches to Hill's normal approximation, whose own error is 2.7e-6 at
    kappa = 50 and 1.2e-8 at 700 (against adaptive quadrature of scipy's pdf, which the series
    branch at kappa = 49 meets to 1e-13): there the 1e-9 comparison is with that quadrature, and
    scipy's cdf is met to its own error."""
    st = pytest.importorskip('scipy.stats')
    quad = pytest.importorskip('scipy.integrate').quad
    x = np.concatenate([np.linspace(-math.pi, math.pi, 4001),
                        np.random.RandomState(0).uniform(-0.3, 0.3, 2000)])
    xq = np.array([-3.0, -0.5, -0.2, -0.05, -0.01, 0.0, 0.02, 0.1, 0.3, 1.0, 3.1])
    for kappa in sorted({k for _, k in VONMISES_CASES}):
        cdf = T.VonMisesCdf(kappa)
        if kappa == 0:
            ref = (x + math.pi) / (2 * math.pi)
        else:
            ref = st.vonmises(kappa).cdf(x)
        err = np.abs(cdf(x) - ref).max()
        if kappa < 50:
            assert err <= 1e-9, (kappa, err)
            continue
        assert err <= 5e-6, (kappa, err)
        pdf = st.vonmises(kappa).pdf
        cuts = [-4 / math.sqrt(kappa), 0.0, 4 / math.sqrt(kappa)]
        q = np.array([quad(pdf, -math.pi, v, epsabs=1e-13, epsrel=1e-13, limit=400,
                           points=[c for c in cuts if c < v] or None)[0] for v in xq])
        assert np.abs(cdf(xq) - q).max() <= 1e-9, (kappa, np.abs(cdf(xq) - q).max())


def test_poisson_pmf_agrees_with_scipy():
    st = pytest.importorskip('scipy.stats')
    for lam in POISSON_LAMBDAS:
        p = T.poisson_min1_pmf(lam, 64)
        ref = st.poisson(lam).pmf(np.arange(65))
        ref[1] += ref[0]
        ref[0] = 0.0
        ref[64] += st.poisson(lam).sf(64)
        assert np.abs(p - ref).max() <= 1e-9, lam
        assert abs(p.sum() - 1.0) <= 1e-12


def test_wilson_hilferty_critical_value():
    """the tabulated 1e-3 points of chi-square (10.828 / 29.588 / 59.703 at 1 / 10 / 30 degrees
    of freedom): with z = 3.09 the approximation is never below them and at most 3.5 % above (its
    error is largest at one degree of freedom, +3.0 %)"""
    for df, tab in [(1, 10.828), (10, 29.588), (30, 59.703)]:
        pmf = np.full(df + 1, 1.0 / (df + 1))
        _, crit = T.chi2_check(pmf * 1000 * (df + 1), pmf)
        assert tab <= crit <= 1.035 * tab, (df, crit)


# ------------------------------------------------------------------ b. the checker is sharp
@pytest.fixture(scope='module')
def base_draws():
    """the oracle's draws at one mid-grid parameter set per sampler"""
    out = {}
    for k, (distr, (p1, p2)) in enumerate(BASE.items()):
        out[distr] = D.move_draws(case_seed(k), IDS, STEP, distr, p1, p2, 3.0, 2.5)
    return out


BASE = {'lognormal': (0.01, 0.5), 'wald': (1.5, 2.0), 'levy': (0.0, 0.3)}
# what: (sampler, the wrong law's parameters); for the angles (mu, kappa)
WRONG_LAWS = {
    'lognormal mean + 0.03': ('lognormal', (0.04, 0.5)),
    'wald mean and scale swapped': ('wald', (2.0, 1.5)),
    'wald scale x 1.05': ('wald', (1.5, 2.0 * 1.05)),
    'levy scale x 1.05': ('levy', (0.0, 0.3 * 1.05)),
    'von Mises kappa x 1.05': ('theta', (3.0, 2.5 * 1.05)),
    'von Mises mu + 0.02': ('theta', (3.02, 2.5)),
}


def _ks(draws, which, par):
    if which == 'theta':
        theta = draws['lognormal'][0].astype(np.float64)
        return T.ks_scaled(T.wrap(theta - par[0]), T.VonMisesCdf(par[1]))
    return T.ks_scaled(draws[which][1], T.distance_cdf(which, *par))


@pytest.mark.parametrize('what', list(WRONG_LAWS))
def test_checker_rejects_a_wrong_law(base_draws, what):
    """the right law passes and the law with one parameter off exceeds the bound, on the same
    draws"""
    which, par = WRONG_LAWS[what]
    good = _ks(base_draws, which, (3.0, 2.5) if which == 'theta' else BASE[which])
    bad = _ks(base_draws, which, par)
    print('%s: sqrt(n) D = %.3f under the right law, %.3f under the wrong one' % (what, good, bad))
    assert good <= KS_BOUND < bad, (what, good, bad)


def test_checker_rejects_nan_and_a_constant():
    """the two catastrophic outputs: a NaN among the draws, and every angle at mu +- pi"""
    x = T.wrap(D.vonmises(case_seed(0), IDS[:2000], STEP, 0, 0.0, 4.0).astype(np.float64))
    x[7] = np.nan
    assert T.ks_scaled(x, T.VonMisesCdf(4.0)) == float('inf')
    with pytest.raises(AssertionError):
        T.check_angles(np.full(N_DRAWS, -np.float32(math.pi)), 0.0, 1e-4)
    with pytest.raises(AssertionError):
        T.check_distances(np.array([1.0, -0.5, 2.0], np.float32), 'wald', 1.5, 2.0)


def test_chi2_check_pools_and_rejects():
    rng = np.random.RandomState(3)
    pmf = T.poisson_min1_pmf(4.0, 64)
    k = np.maximum(rng.poisson(4.0, N_DRAWS), 1)
    stat, crit = T.chi2_check(np.bincount(k, minlength=65), pmf)
    assert stat <= crit
    k = np.maximum(rng.poisson(4.0 * 1.05, N_DRAWS), 1)
    stat, crit = T.chi2_check(np.bincount(k, minlength=65), pmf)
    assert stat > crit


# ------------------------------------------------------------------ c. the oracle's draws
@pytest.mark.parametrize('case', range(len(VONMISES_CASES)),
                         ids=['mu%g-kappa%g' % c for c in VONMISES_CASES])
def test_oracle_vonmises_follows_its_law(case):
    mu, kappa = VONMISES_CASES[case]
    theta, _ = D.move_draws(case_seed(case), IDS, STEP, 'lognormal', 0.01, 0.5, mu, kappa)
    stat = T.check_angles(theta, mu, kappa)
    print('von Mises(%g, %g): sqrt(n) D = %.3f' % (mu, kappa, stat))


@pytest.mark.parametrize('case', range(len(DISTANCE_CASES)),
                         ids=['%s-%g-%g' % c for c in DISTANCE_CASES])
def test_oracle_distance_follows_its_law(case):
    """the movement's distance and every attempt row of the dispersal's.  The dispersal's
    angles, pi (2 u - 1) of the block's fourth word, are checked as one sample of all eight
    attempts: row by row they were 88 more tests at 1e-3 each on top of the 99 of the distances,
    and one of them duly came out at 2.04 (levy (2, 5), attempt 5) while the 88 statistics
    followed Kolmogorov's law (5.7 % above its 5 % point, 1.1 % above its 1 % point)."""
    distr, p1, p2 = DISTANCE_CASES[case]
    _, dist = D.move_draws(case_seed(case), IDS, STEP, distr, p1, p2, 0.0, 0.0)
    stats = [T.check_distances(dist, distr, p1, p2)]
    th, ds = D.dispersal_draws(case_seed(case), IDS, STEP, distr, p1, p2)
    for a in range(ds.shape[0]):
        stats.append(T.check_distances(ds[a], distr, p1, p2))
    T.check_angles(th.ravel(), 0.0, 0.0)
    print('%s(%g, %g): sqrt(n) D = %.3f (move), <= %.3f (dispersal attempts)' % (
        distr, p1, p2, stats[0], max(stats[1:])))


@pytest.mark.parametrize('case', range(len(POISSON_LAMBDAS)),
                         ids=['lambda%g' % l for l in POISSON_LAMBDAS])
def test_oracle_births_follow_poisson(case):
    """max(Poisson(lambda), 1); the device equals these counts pair by pair
    (test_gpu_draws.py::test_poisson_births_match_oracle), so its law is checked here"""
    lam = POISSON_LAMBDAS[case]
    k = D.births_draws(case_seed(case), IDS, STEP, lam)
    assert k.min() >= 1 and k.max() < 64
    stat, crit = T.chi2_check(np.bincount(k, minlength=65), T.poisson_min1_pmf(lam, 64))
    print('Poisson(%g): chi2 = %.2f, critical %.2f' % (lam, stat, crit))
    assert stat <= crit, (lam, stat, crit)


def test_births_lambda_above_the_limit_is_refused():
    """the Knuth loop has the 64 uniforms of its stream: above lambda = 26 the mass of k >= 64
    (1.0e-9 at 27, 4.4e-3 at 45) would collapse onto 64"""
    assert D.BIRTHS_LAMBDA_MAX == 26
    D.births_draws(1, IDS[:10], STEP, 26.0)
    with pytest.raises(ValueError, match='26'):
        D.births_draws(1, IDS[:10], STEP, 26.5)
