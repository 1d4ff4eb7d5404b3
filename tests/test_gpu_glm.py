"""Model.run_logistic_gea / calc_clines on the device (csrc/gnx_glm.hip, sim/glm.py,
Species._run_logistic_gea / _calc_clines): gnx_glm_sweep against the extended-precision
reference of tests/_glm.py on its shapes, repeated, fit by fit and across batch boundaries, its
refusals, the planted case through the Species methods and a walked Model.  Needs an MI355X.

The sweep.  Per output o = sum_i term_i the device is held to the a priori bound
  |o - o_ref| <= 2^-53 sum_i (stretch + stretches + c + (p + 1) H_i) |term_i|,
  H_i = sum_j |X_ij B_kj|:
stretch + stretches is the ordered summation (within a stretch, then over the stretches),
(p + 1) H_i the rounding of eta carried through the sigmoid, whose derivatives are at most 1,
and c the roundings of exp, log1p, the division and the products.  c is measured, not fitted to
the device: numpy_sweep in fp64 needs c = 0 on these cases (tests/test_glm_host.py: its worst
difference is 0.082 of the bound without c), and the device - another libm, explicit fused
multiply-adds - is given four times that, C_DEVICE = 0.  Outputs whose terms lie below the
normal fp64 range (w x x at |eta| >= 1000) must be exactly zero, and the fits whose every |eta|
is beyond exp's underflow are held to bytes: mu in {0, 1}, w = 0, s = sum max(eta, 0), in the
call's order (tests/_glm.py, huge_expected).
Measured on an MI355X, worst |o - o_ref| / bound per shape (n, m, p), printed by the test:
  (1, 1, 1) 0.0123, (63, 65, 2) 0.0705, (129, 257, 3) 0.0621, (300, 64, 8) 0.0415,
  (4161, 5, 4) 0.0656, (65, 3, 5) 0.0763, (130, 3, 6) 0.0245, (200, 4, 7) 0.0511; the device needs
  c = 0 on every one.

The scans.  The device and the host run the same driver (sim/glm.scan) on sums that differ by
rounding, so the two may stop one Newton step apart; that step is at most tol max(1, |b|) in
the standardised design, and Newton's error after it is of the order of its square.  beta
is held to 2 tol max(1, |beta|) and lrt to 2 tol max(1, |l|)."""
import ctypes as C

import numpy as np
import pytest

import _assoc as ACASES
import _glm as CASES
from test_gpu_assoc import _population, _Spp, _walked_model
from test_gpu_parity import native
from geonomics_amd.sim import assoc as AS
from geonomics_amd.sim import glm as G

pytestmark = pytest.mark.gpu

C_NUMPY = 0.0
C_DEVICE = 4.0 * C_NUMPY
TOL = 1e-8


@pytest.fixture(scope='module')
def dev():
    """a handle without a population: the sweep borrows its stream and nothing else"""
    nat = native()
    d = nat.Device(8, 8, 1, L=64, cap_inds=64, cap_rows=64, seed=1)
    yield d
    d.close()


@pytest.mark.parametrize('shape', CASES.SWEEP_SHAPES, ids=lambda s: 'n%d-m%d-p%d' % s)
def test_sweep_against_extended_precision(dev, shape):
    n, m, p = shape
    X, B = CASES.sweep_case(n, m, p)
    got = dev.glm_sweep(X, B, info=True)
    sums = got['sums']
    assert sums.shape == (m, G.n_cols(p)) and sums.dtype == np.float64
    assert np.isfinite(sums).all() and got['kernel_ms'] > 0
    assert (got['stretch'], got['stretches']) == G.stretch_rule(n)
    worst = CASES.within_bound(sums, n, m, p, C_DEVICE)
    print('(n, m, p) = %s: %d stretches of %d; worst |o - o_ref| / bound %.3g (c = %g); the '
          'device needs c = %g; kernels %.3f ms'
          % (shape, got['stretches'], got['stretch'], worst, C_DEVICE,
             CASES.needed_c(sums, n, m, p), got['kernel_ms']))
    assert worst <= 1.0
    if m >= 2:                                   # every |eta| of the last fit is beyond 1000
        assert sums[-1].tobytes() == CASES.huge_expected(X, B[-1]).tobytes()
    again, ms = dev.glm_sweep(X, B)                                    # a repeated call
    assert again.tobytes() == sums.tobytes() and ms > 0


@pytest.mark.parametrize('shape', CASES.SWEEP_SHAPES, ids=lambda s: 'n%d-m%d-p%d' % s)
def test_beyond_the_underflow_of_exp_both_signs(dev, shape):
    """|eta| > 800 everywhere, in both signs of the coefficient: exactly mu in {0, 1}, w = 0
    and s = max(eta, 0) summed"""
    n, m, p = shape
    X, scale = CASES.design(n, p, 3000 + n + p)
    B = np.stack([CASES.huge_fit(X, scale, 1.0), CASES.huge_fit(X, scale, -1.0)])
    sums, _ = dev.glm_sweep(X, B)
    for k in range(2):
        assert sums[k].tobytes() == CASES.huge_expected(X, B[k]).tobytes(), k
        s, A, I = G.unpack(sums[k:k + 1], p)
        assert (I == 0).all()


def test_a_fit_does_not_depend_on_its_company_or_its_batch(dev):
    """fit k alone, as one of 257, and with the batch boundary before and after it: with a
    budget of one byte a batch is 256 fits, so fit 255 ends a batch and fit 256 begins one"""
    n, m, p = CASES.SWEEP_SHAPES[2]
    X, B = CASES.sweep_case(n, m, p)
    among, _ = dev.glm_sweep(X, B)
    try:
        dev.glm_budget(1)
        cut, _ = dev.glm_sweep(X, B)
        wide = np.tile(B, (3, 1))                                      # 771 fits: four batches
        cut3, _ = dev.glm_sweep(X, wide)
    finally:
        dev.glm_budget(0)
    assert cut.tobytes() == among.tobytes()
    assert cut3.tobytes() == np.tile(among, (3, 1)).tobytes()
    for k in (0, 100, 255, 256):
        alone, _ = dev.glm_sweep(X, B[k:k + 1])
        assert alone.shape == (1, G.n_cols(p))
        assert alone.tobytes() == among[k:k + 1].tobytes(), k
    back, _ = dev.glm_sweep(X, B[::-1])
    assert np.ascontiguousarray(back[::-1]).tobytes() == among.tobytes()
    with pytest.raises(native().GnxError, match=r'gnx_glm_budget: bytes >= 0'):
        dev.glm_budget(-1)


def test_refusals_launch_nothing(dev):
    nat = native()
    n, m, p = CASES.SWEEP_SHAPES[1]
    X, B = CASES.sweep_case(n, m, p)
    before, _ = dev.glm_sweep(X, B)

    def refused(match, X_, B_):
        with pytest.raises(nat.GnxError, match=match):
            dev.glm_sweep(X_, B_)

    refused(r'1 <= p <= 8 columns \(got 0\)', np.zeros((n, 0)), np.zeros((m, 0)))
    refused(r'1 <= p <= 8 columns \(got 9\)', np.zeros((n, 9)), np.zeros((m, 9)))
    refused(r'1\.\.2\^30 individuals \(n = 0\)', np.zeros((0, p)), B)
    refused(r'1\.\.2\^24 fits \(m = 0\)', X, np.zeros((0, p)))
    for bad in (np.nan, np.inf, -np.inf):
        Xb, Bb = X.copy(), B.copy()
        Xb[n - 1, p - 1] = bad
        Bb[m - 2, 0] = bad
        refused(r'X is not finite \(row %d, column %d\)' % (n - 1, p - 1), Xb, B)
        refused(r'B is not finite \(fit %d, column 0\)' % (m - 2), X, Bb)
    with pytest.raises(ValueError, match=r'X \[n\]\[p\] and B \[m\]\[p\]'):
        dev.glm_sweep(X, B[:, :1])
    # null pointers, through the library itself
    dbl = C.POINTER(C.c_double)
    out = np.zeros((m, G.n_cols(p)))
    px, pb, po = (a.ctypes.data_as(dbl) for a in (X, B, out))
    for args in ((None, pb, po), (px, None, po), (px, pb, None)):
        rc = dev.lib.gnx_glm_sweep(dev.h, n, p, args[0], m, args[1], args[2], None, None, None)
        assert rc == 1
        assert dev.lib.gnx_last_error().decode() == 'gnx_glm_sweep: null X, B or sums'
    assert (out == 0).all()
    after, _ = dev.glm_sweep(X, B)                                     # a good call follows
    assert after.tobytes() == before.tobytes()


# ---- through the Species methods ------------------------------------------------------------
def _agree(got, ref, keys=('beta',)):
    """tested, converged and maf equal; beta within 2 tol max(1, |beta|); lrt within 2 tol
    max(1, |l|) (module docstring) -> the worst ratios"""
    for k in ('tested', 'converged', 'maf'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    ok = ref['tested']
    worst = []
    for k in keys:
        a, b = got[k][ok], ref[k][ok]
        assert np.isfinite(a).all(), k
        big = np.maximum(1.0, np.abs(b).reshape(b.shape[0], -1).max(axis=1))
        worst.append(float((np.abs(a - b).reshape(b.shape[0], -1).max(axis=1)
                            / (2 * TOL * big)).max()))
    r_l = np.abs(got['lrt'][ok] - ref['lrt'][ok]) / \
        (2 * TOL * np.maximum(1.0, np.abs(ref['loglik'][ok])))
    worst.append(float(r_l.max()))
    assert max(worst) <= 1.0, worst
    assert np.isnan(got['lrt'][~ok]).all()
    return worst


def test_the_planted_case_through_the_species_methods():
    nat = native()
    c = ACASES.planted()
    D, env, deme = c['D'], c['env'], c['deme'].astype(np.float64)
    n, L = D.shape
    dev = _population(nat, D, 6)
    try:
        spp = _Spp(dev)
        x = dev.download(nat.F_X).astype(np.float64)
        gea = spp._run_logistic_gea(env=env, covars=deme)
        cl = spp._calc_clines(axis='x', sigma=0.5)
        cl45 = spp._calc_clines(axis=45.0, covars=deme, loci=[5, 3])
        y = dev.download(nat.F_Y).astype(np.float64)
    finally:
        dev.close()
    cross = AS.numpy_cross(D)
    ref = G.scan(cross, G.numpy_sweep, n, env, deme)
    worst = _agree(gea, ref)
    np.testing.assert_array_equal(gea['ids'], np.arange(n))
    np.testing.assert_array_equal(gea['loci'], np.arange(L))
    np.testing.assert_array_equal(np.sort(np.argsort(gea['p'], kind='stable')[:6]), c['causal'])
    assert gea['converged'].all() and gea['gif'] < 1.5 and gea['df'] == 1
    assert gea['trait_loci'] is None and gea['kernel_ms'] > 0
    assert gea['n_sweeps'] >= 2 and gea['seconds'] > 0
    assert gea['beta'].shape == (L, 1) and gea['n_iter'].shape == (L,)
    np.testing.assert_allclose(gea['gif'], ref['gif'], rtol=1e-6)
    print('run_logistic_gea on the device: gif %.4g, %d sweeps, kernels %.3f ms; worst '
          'difference / bound: beta %.3g, lrt %.3g'
          % (gea['gif'], gea['n_sweeps'], gea['kernel_ms'], worst[0], worst[1]))
    # clines along x, and along the diagonal with a covariate
    ref_c = G.scan(cross, G.numpy_sweep, n, x)
    ref_c['beta'] = ref_c['coef']
    _agree(cl, ref_c)
    lo, hi = float(x.min()), float(x.max())
    assert cl['axis_range'] == (lo, hi)
    st = G.cline_stats(ref_c['coef'], ref_c['cov'], lo, hi)
    np.testing.assert_array_equal(cl['in_range'], st['in_range'])
    np.testing.assert_allclose(cl['width'], st['width'], rtol=1e-6)
    np.testing.assert_allclose(cl['s_hat'], 8 * 0.25 / cl['width'] ** 2)
    assert np.isfinite(cl['centre'][cl['converged']]).all()
    assert set(cl['concordance']) == {'n_loci', 'median_centre', 'mad_centre', 'median_width',
                                      'mad_width'}
    proj = (x + y) / np.sqrt(2.0)
    ref_d = G.scan(cross, G.numpy_sweep, n, proj, deme - deme.mean())
    np.testing.assert_array_equal(cl45['loci'], [3, 5])
    assert cl45['beta'].shape == (2, 3)
    np.testing.assert_allclose(cl45['beta'], ref_d['coef'][[3, 5]][:, [0, 2, 1]], rtol=1e-6,
                               atol=1e-8)
    np.testing.assert_allclose(cl45['q'], ref_d['q'][[3, 5]], rtol=1e-6)


def test_a_walked_model_agrees_with_the_host_driver():
    mod = _walked_model(21)
    spp = mod.comm[0]
    gea = mod.run_logistic_gea(env_lyrs=[1], covars=('x',))
    cl = mod.calc_clines(axis='x')
    D = np.rint(2.0 * mod.get_genotypes(biallelic=False)).astype(np.int64)
    n, L = D.shape
    e, xy = mod.get_e(), mod.get_coords()
    assert 200 < n < 500 and L == 100
    np.testing.assert_array_equal(gea['ids'], np.array([*spp]))
    x = np.asarray(xy[:, 0], np.float64)
    ref = G.scan(AS.numpy_cross(D), G.numpy_sweep, n, np.asarray(e[:, 1], np.float64), x)
    worst = _agree(gea, ref)
    assert gea['tested'].any() and gea['beta'].shape == (L, 1)
    assert len(gea['trait_loci']) == 1
    print('walked model: n = %d, %d loci tested, %d converged; worst difference / bound: beta '
          '%.3g, lrt %.3g' % (n, gea['tested'].sum(), gea['converged'].sum(), worst[0], worst[1]))
    assert cl['axis_range'] == pytest.approx((float(x.min()), float(x.max())), rel=1e-6)
    assert cl['converged'].any() and np.isfinite(cl['centre'][cl['converged']]).all()
    assert np.isfinite(cl['width'][cl['converged']]).all()
    assert np.isin(spp.gen_arch.traits[0].loci, cl['trait_loci']).all()
    some = np.array([*spp])[::3]
    sub = mod.run_logistic_gea(env_lyrs=1, individs=some[::-1], loci=[60, 5])
    np.testing.assert_array_equal(sub['ids'], some)
    np.testing.assert_array_equal(sub['loci'], [5, 60])
    ref_s = G.scan(AS.numpy_cross(D[::3]), G.numpy_sweep, some.size,
                   np.asarray(e[::3, 1], np.float64))
    _agree(sub, {k: (v[[5, 60]] if isinstance(v, np.ndarray) and v.shape[:1] == (L,) else v)
                 for k, v in ref_s.items()})
    with pytest.raises(ValueError, match='give individs or n, not both'):
        mod.calc_clines(individs=some, n=5)
