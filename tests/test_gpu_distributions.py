"""The device samplers against the distributions they claim (csrc/gnx_rng.h: gnx_vonmises,
gnx_distance), on what k_move itself draws (op_move_draws): np.random.vonmises(mu, kappa),
np.random.lognormal(mean, sigma), np.random.wald(mean, scale), scipy.stats.levy(loc, scale),
through the f64 distribution functions of tests/_distributions.py (no scipy here;
test_distributions_host.py holds them against scipy and shows the bound is sharp).  The parity
tests compare the device with the oracle's restatement of the same f32 formulas, which is wrong
wherever they are; these do not.  n = 50 000 draws per case, sqrt(n) D_n <= 1.95 (Kolmogorov's
1e-3 point); seeds, ids and step were fixed before anything ran.  The Poisson births equal the
oracle's pair by pair (test_gpu_draws.py), whose law the host test checks.  Needs an MI355X.

STATISTICS (sqrt(n) D_n on an MI355X; the same to three digits as the oracle's in
test_distributions_host.py): von Mises, kappa 0 ... 700 at mu = 0: 1.11, 0.94, 0.53, 0.70, 1.04,
1.06, 0.66, 0.91, 0.74, 0.73, 0.72, 1.08; (3, 2.5) 1.47, (-3.1, 12) 0.78, (7, 1) 0.73; lognormal
0.59, 1.27, 1.46; wald 0.92, 1.10, 0.70, 1.03, 0.48, 1.36; levy 0.90, 0.80; the surface case 0.80.
Before the fix the device returned, for all 50 000 individuals at kappa = 1e-5, 1e-4 and 3.2e-4,
exactly -pi or +pi (two distinct values, half each: the clamp turns the NaN proposal into -1,
acosf gives pi, the sign draw does the rest), and 198 of 50 000 distances <= 0 at wald (100, 0.1)
(sqrt(n) D = 8.3), 4071 at wald (50, 0.01) (43.3).
"""
import numpy as np
import pytest

import _distributions as T
from _distributions import (N_DRAWS, STEP, VONMISES_CASES, DISTANCE_CASES, case_seed, case_ids)
from test_gpu_parity import make_dev, upload_simple, native

pytestmark = pytest.mark.gpu

W = H = 64


def _move_draws(seed, **sp_kw):
    """what k_move draws for N_DRAWS individuals spread over the landscape"""
    rng = np.random.RandomState(seed)
    dev = make_dev(W, H, cap=65536, seed=seed, **sp_kw)
    try:
        upload_simple(dev, rng.rand(N_DRAWS) * W, rng.rand(N_DRAWS) * H, ids=case_ids())
        dev.step_index = STEP
        return dev.op_move_draws()
    finally:
        dev.close()


@pytest.mark.parametrize('case', range(len(VONMISES_CASES)),
                         ids=['mu%g-kappa%g' % c for c in VONMISES_CASES])
def test_device_vonmises_follows_its_law(case):
    """every angle finite and in [-pi, pi], wrap(theta - mu) ~ von Mises(0, kappa); from
    kappa = 0.5 at least 1000 distinct angles.  The rows with kappa <= 0.05 cannot tell the law
    from the uniform one at this n: they guard against NaN and against every angle at mu +- pi,
    what the f32 cancellation of rho gave for 1e-5 <= kappa < 3.24e-4 (T.check_angles)."""
    mu, kappa = VONMISES_CASES[case]
    theta, _ = _move_draws(case_seed(case), dir_mu=mu, dir_kappa=kappa)
    print('von Mises(%g, %g): %d distinct angles, first %s' % (
        mu, kappa, np.unique(theta).size, theta[:4]))
    stat = T.check_angles(theta, mu, kappa)
    print('von Mises(%g, %g): sqrt(n) D = %.3f' % (mu, kappa, stat))


@pytest.mark.parametrize('case', range(len(DISTANCE_CASES)),
                         ids=['%s-%g-%g' % c for c in DISTANCE_CASES])
def test_device_distance_follows_its_law(case):
    """every distance finite and > 0 (levy: > loc), and distributed as its law"""
    distr, p1, p2 = DISTANCE_CASES[case]
    _, dist = _move_draws(case_seed(case), move_distr=native().DIST[distr], move_p1=p1,
                          move_p2=p2)
    print('%s(%g, %g): min %g, %d not finite' % (distr, p1, p2, np.nanmin(dist),
                                                 int((~np.isfinite(dist)).sum())))
    stat = T.check_distances(dist, distr, p1, p2)
    print('%s(%g, %g): sqrt(n) D = %.3f' % (distr, p1, p2, stat))


def test_device_surface_direction_at_small_kappa():
    """SURF_UNIMODAL on a constant raster: away from the border all eight neighbours tie, the
    bearing is their mean pi / 8, and the angle is that plus von Mises(0, 1e-4) - the kappa band
    in which every draw used to be NaN -> pi.  Finite, not all equal, and uniform about the
    bearing to the bound."""
    nat = native()
    rasts = np.stack([np.ones((H, W), np.float32), np.full((H, W), 0.5, np.float32)])
    theta, _ = _move_draws(case_seed(len(VONMISES_CASES)), rasts=rasts,
                           move_surf=nat.SURF_UNIMODAL, move_surf_layer=1, move_surf_kappa=1e-4)
    assert np.isfinite(theta).all()
    assert np.unique(theta).size >= 1000
    rng = np.random.RandomState(case_seed(len(VONMISES_CASES)))     # the positions _move_draws used
    x = (rng.rand(N_DRAWS) * W).astype(np.float32)
    y = (rng.rand(N_DRAWS) * H).astype(np.float32)
    inner = (x >= 1) & (x < W - 1) & (y >= 1) & (y < H - 1)
    loc = np.float32(np.pi / 8)
    stat = T.ks_scaled(T.wrap(theta[inner].astype(np.float64) - loc), T.VonMisesCdf(1e-4))
    print('surface, kappa 1e-4: sqrt(n) D = %.3f over %d inner individuals' % (stat, inner.sum()))
    assert stat <= T.KS_BOUND
