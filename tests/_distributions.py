"""Goodness-of-fit checker for the device samplers (csrc/gnx_rng.h) and their restatement in
oracle/gnx_draws.py: the f64 distribution functions of the laws the samplers claim -
np.random.lognormal / wald / vonmises, scipy.stats.levy, Poisson - a Kolmogorov-Smirnov
statistic and a chi-square check.  numpy and math only: the GPU tests import it, and nothing
they import may need scipy.  tests/test_distributions_host.py compares every function here
with scipy.stats where scipy is importable and shows that the bound catches 5 % errors."""
import math

import numpy as np

# sqrt(n) D_n <= 1.95: Kolmogorov's asymptotic distribution, P(sqrt(n) D_n > t) ~ 2 exp(-2 t^2),
# is 1e-3 at t = 1.95 (D <= 0.0087 at n = 50 000).  Derived, not tuned.
KS_BOUND = 1.95
N_DRAWS = 50000
STEP = 17

# the case grid shared by the oracle (host) and device (GPU) tests; the seed of a case is
# 1000 + its index in its list, the ids are 3 k + 1
VONMISES_CASES = [(0.0, k) for k in (0.0, 5e-9, 5e-6, 1e-5, 1e-4, 3.2e-4, 1e-3, 1e-2, 0.5, 4.0,
                                     50.0, 700.0)] + [(3.0, 2.5), (-3.1, 12.0), (7.0, 1.0)]
DISTANCE_CASES = [('lognormal', 0.01, 0.5), ('lognormal', -1.0, 0.6), ('lognormal', 3.0, 2.0),
                  ('wald', 1.5, 2.0), ('wald', 0.1, 10.0), ('wald', 5.0, 0.1),
                  ('wald', 30.0, 0.1), ('wald', 100.0, 0.1), ('wald', 50.0, 0.01),
                  ('levy', 0.0, 0.3), ('levy', 2.0, 5.0)]
POISSON_LAMBDAS = [0.05, 0.4, 1.0, 4.0, 12.0, 26.0]


def case_seed(index):
    return 1000 + index


def case_ids(n=N_DRAWS):
    return 3 * np.arange(n, dtype=np.int64) + 1


_erfc = np.frompyfunc(math.erfc, 1, 1)
_erf = np.frompyfunc(math.erf, 1, 1)


def _phi(z):
    """standard normal distribution function; erfc keeps the lower tail's relative precision"""
    z = np.asarray(z, np.float64)
    return 0.5 * _erfc(-z / math.sqrt(2.0)).astype(np.float64)


def lognormal_cdf(x, mean, sigma):
    x = np.asarray(x, np.float64)
    out = np.zeros(x.shape)
    pos = x > 0
    z = (np.log(x[pos]) - mean) / (sigma * math.sqrt(2.0))
    out[pos] = 0.5 * (1.0 + _erf(z).astype(np.float64))
    return out


def invgauss_cdf(x, mean, shape):
    """inverse Gaussian (np.random.wald(mean, scale): scale is the shape lambda):
    Phi(sqrt(l/x)(x/m - 1)) + exp(2 l/m) Phi(-sqrt(l/x)(x/m + 1)), the second term in log space
    (2 l/m reaches 200 on the case grid; where Phi underflows the product is < e^-500)"""
    x = np.asarray(x, np.float64)
    out = np.zeros(x.shape)
    pos = x > 0
    xp = x[pos]
    s = np.sqrt(shape / xp)
    first = _phi(s * (xp / mean - 1.0))
    tail = _phi(-s * (xp / mean + 1.0))
    with np.errstate(divide='ignore'):
        second = np.exp(2.0 * shape / mean + np.log(tail))
    out[pos] = np.minimum(first + second, 1.0)
    return out


def levy_cdf(x, loc, scale):
    x = np.asarray(x, np.float64)
    out = np.zeros(x.shape)
    pos = x > loc
    out[pos] = _erfc(np.sqrt(scale / (2.0 * (x[pos] - loc)))).astype(np.float64)
    return out


def wrap(t):
    """an angle onto (-pi, pi]"""
    t = np.asarray(t, np.float64)
    return math.pi - np.mod(math.pi - t, 2.0 * math.pi)


class VonMisesCdf:
    """von Mises(0, kappa) on (-pi, pi]: cumulative trapezoid of f = exp(kappa (cos t - 1)) on
    2^16 + 1 points, each panel with its end-point correction -h^2/12 (f'(b) - f'(a)) (f' is
    known in closed form; the panel error falls from O(h^3 f'') to O(h^5 f'''')), read between
    the grid points by the cubic Hermite interpolant of (F, f).  The law is circular: test
    wrap(theta - mu)."""

    def __init__(self, kappa, log2_points=16):
        self.kappa = float(kappa)
        m = 1 << log2_points
        self.h = 2.0 * math.pi / m
        t = -math.pi + self.h * np.arange(m + 1)
        f = np.exp(self.kappa * (np.cos(t) - 1.0))
        df = -self.kappa * np.sin(t) * f
        panel = 0.5 * self.h * (f[1:] + f[:-1]) - self.h ** 2 / 12.0 * (df[1:] - df[:-1])
        F = np.concatenate([[0.0], np.cumsum(panel)])
        self.norm = F[-1]
        self.F, self.f, self.m = F / self.norm, f / self.norm, m

    def __call__(self, x):
        x = np.asarray(x, np.float64)
        u = (np.clip(x, -math.pi, math.pi) + math.pi) / self.h
        i = np.minimum(u.astype(np.int64), self.m - 1)
        s = u - i
        h00 = (1.0 + 2.0 * s) * (1.0 - s) ** 2
        h10 = s * (1.0 - s) ** 2
        h01 = s * s * (3.0 - 2.0 * s)
        h11 = s * s * (s - 1.0)
        return (h00 * self.F[i] + h01 * self.F[i + 1]
                + self.h * (h10 * self.f[i] + h11 * self.f[i + 1]))


def poisson_min1_pmf(lam, kmax):
    """pmf of max(Poisson(lam), 1) on 0..kmax, the mass above kmax added to the last cell"""
    k = np.arange(kmax + 1)
    logp = k * math.log(lam) - lam - np.array([math.lgamma(j + 1.0) for j in k])
    p = np.exp(logp)
    p[1] += p[0]
    p[0] = 0.0
    p[-1] += max(0.0, 1.0 - p.sum())
    return p


def ks_scaled(x, cdf):
    """sqrt(n) D_n, two-sided, from the sorted sample; inf when a draw is not finite"""
    x = np.asarray(x, np.float64).ravel()
    n = x.size
    if not np.isfinite(x).all():
        return float('inf')
    F = np.asarray(cdf(np.sort(x)), np.float64)
    i = np.arange(1, n + 1)
    D = max((i / n - F).max(), (F - (i - 1) / n).max())
    return math.sqrt(n) * D


def chi2_check(counts, pmf):
    """Pearson's chi-square of the counts against n pmf.  Neighbouring cells are pooled until
    each expects >= 5; the critical value is the 1e-3 point in the Wilson-Hilferty
    approximation, df (1 - 2/(9 df) + 3.09 sqrt(2/(9 df)))^3.  Returns (statistic, critical)."""
    counts = np.asarray(counts, np.float64)
    pmf = np.asarray(pmf, np.float64)
    assert counts.shape == pmf.shape and abs(pmf.sum() - 1.0) < 1e-9
    n = counts.sum()
    obs, exp = [], []
    o = e = 0.0
    for c, p in zip(counts, pmf):
        o += c
        e += n * p
        if e >= 5.0:
            obs.append(o)
            exp.append(e)
            o = e = 0.0
    if e > 0.0 or o > 0.0:                     # the remainder joins the last pooled cell
        obs[-1] += o
        exp[-1] += e
    obs, exp = np.array(obs), np.array(exp)
    df = obs.size - 1
    assert df >= 1, 'fewer than two cells expect 5 counts'
    stat = float(((obs - exp) ** 2 / exp).sum())
    c = 2.0 / (9.0 * df)
    return stat, df * (1.0 - c + 3.09 * math.sqrt(c)) ** 3


def distance_cdf(distr, p1, p2):
    if distr == 'lognormal':
        return lambda x: lognormal_cdf(x, p1, p2)
    if distr == 'wald':
        return lambda x: invgauss_cdf(x, p1, p2)
    return lambda x: levy_cdf(x, p1, p2)


def check_angles(theta, mu, kappa, min_distinct=1000):
    """what both test files assert of a sample of von Mises(mu, kappa) angles; returns the
    statistic.  kappa <= 0.05: at n = 50 000 the KS statistic cannot tell such a von Mises from
    the uniform law (the densities differ by kappa cos t / 2 pi, the distribution functions by
    <= kappa / 2 pi = 0.008 = D's bound), so those rows guard against the catastrophic failure -
    NaN, or every angle at mu +- pi - and not against a slightly wrong kappa."""
    theta = np.asarray(theta)
    assert np.isfinite(theta).all(), 'von Mises(%g, %g): %d angles are not finite' % (
        mu, kappa, int((~np.isfinite(theta)).sum()))
    assert (np.abs(theta) <= np.float32(math.pi)).all(), (mu, kappa)      # f32 pi, no allowance
    stat = ks_scaled(wrap(theta.astype(np.float64) - mu), VonMisesCdf(kappa))
    assert stat <= KS_BOUND, 'von Mises(%g, %g): sqrt(n) D = %.3f' % (mu, kappa, stat)
    if kappa >= 0.5:
        assert np.unique(theta).size >= min_distinct, (mu, kappa)
    return stat


def check_distances(dist, distr, p1, p2):
    dist = np.asarray(dist)
    bad = ~np.isfinite(dist) | ~(dist > (p1 if distr == 'levy' else 0.0))
    assert not bad.any(), '%s(%g, %g): %d of %d distances are not finite or not positive' % (
        distr, p1, p2, int(bad.sum()), dist.size)
    stat = ks_scaled(dist, distance_cdf(distr, p1, p2))
    assert stat <= KS_BOUND, '%s(%g, %g): sqrt(n) D = %.3f' % (distr, p1, p2, stat)
    return stat
