"""Per-locus logistic fits on the CPU (geonomics_amd/sim/glm.py with numpy_sweep and a numpy
cross; Species._run_logistic_gea / _calc_clines' request checks on the stand-in Species of
tests/test_analyses_host.py; the prototype of include/gnx_glm.h).  No GPU.

Closed forms hold to 1e-10 relative: the fit stops at a relative step of 1e-8 and Newton's error
after the stopping step is of the order of its square.  The independent optimiser (BFGS) is held
to 1e-6 se: that is BFGS's accuracy at gtol = 1e-10, not the fit's (measured here: at most
1.1e-8 se).  The c of the sweep's bound (tests/_glm.py, sweep_reference): numpy_sweep in fp64 needs
c = 0 against the extended-precision reference on every case - its worst difference is 0.082 of
the bound without c, the summation allowance stretch + stretches >= 65 already covers the few
roundings per element - so the device is given 4 x 0 = 0 as well (tests/test_gpu_glm.py)."""
import ctypes as C

import numpy as np
import pytest
from scipy import optimize

import _assoc as ACASES
import _glm as CASES
from test_analyses_host import NO_GENOMES, UNASSIGNED, _refusal, _Species
from test_assoc_host import check_planted
from geonomics_amd import _native as nat
from geonomics_amd.sim import assoc as AS
from geonomics_amd.sim import glm as G

C_NUMPY = 0.0           # the c numpy_sweep needs (module docstring); the device's is 4 x this


@pytest.fixture(scope='module')
def planted_scan():
    """the planted case with deme as covariate and env tested, and its design"""
    c = ACASES.planted()
    res = G.scan(AS.numpy_cross(c['D']), G.numpy_sweep, 400, c['env'],
                 c['deme'].astype(np.float64))
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def test_stretch_rule_and_unpack():
    assert G.stretch_rule(1) == (64, 1)
    assert G.stretch_rule(64) == (64, 1) and G.stretch_rule(65) == (64, 2)
    assert G.stretch_rule(4096) == (64, 64) and G.stretch_rule(4097) == (128, 33)
    assert G.stretch_rule(4161) == (128, 33)          # 66 tiles: the last stretch 64 + 1
    assert G.stretch_rule(8192) == (128, 64)
    assert G.stretch_rule(10 ** 6) == (15680, 64)
    assert [G.n_cols(p) for p in (1, 2, 8)] == [3, 6, 45]
    s, A, I = G.unpack(np.arange(12.0).reshape(2, 6), 2)
    np.testing.assert_array_equal(s, [0, 6])
    np.testing.assert_array_equal(A, [[1, 2], [7, 8]])
    np.testing.assert_array_equal(I[0], [[3, 4], [4, 5]])
    with pytest.raises(ValueError, match='sums'):
        G.unpack(np.zeros((2, 5)), 2)


@pytest.mark.parametrize('shape', CASES.SWEEP_SHAPES, ids=lambda s: 'n%d-m%d-p%d' % s)
def test_numpy_sweep_needs_no_c_against_extended_precision(shape):
    """the measurement behind C_NUMPY, and the fits beyond exp's underflow: mu in {0, 1}, w = 0"""
    n, m, p = shape
    X, B = CASES.sweep_case(n, m, p)
    sums, ms = G.numpy_sweep(X, B)
    assert sums.shape == (m, G.n_cols(p)) and sums.dtype == np.float64 and ms == 0.0
    need = CASES.needed_c(sums, n, m, p)
    worst = CASES.within_bound(sums, n, m, p, C_NUMPY)
    print('(n, m, p) = %s: numpy_sweep needs c = %g; worst difference / bound %.3g'
          % (shape, need, worst))
    assert need <= C_NUMPY and worst <= 1.0
    if m >= 2:
        s, A, I = G.unpack(sums[-1:], p)
        eta = X[:, 0] * B[-1, 0]
        assert (I == 0).all()
        np.testing.assert_allclose(s[0], np.maximum(eta, 0).sum(), rtol=1e-13)
        np.testing.assert_allclose(A[0], X[eta > 0].sum(axis=0), rtol=1e-12, atol=0)
    ext, _ = G.numpy_sweep(X, B, np.longdouble)
    assert ext.dtype == np.longdouble
    ref = CASES.sweep_reference(n, m, p)[0]
    # two roads to the extended-precision sums: the differences are extended-precision roundings
    T0 = CASES.sweep_reference(n, m, p)[1]
    assert (np.abs(ext - ref) <= 2.0 ** -60 * (n + 8 * p) * T0 + np.finfo(np.float64).tiny).all()


def test_intercept_only_is_the_logit_of_the_frequency():
    D = ACASES.planted()['D']
    n = D.shape[0]
    s1 = D.sum(axis=0).astype(np.float64)
    f = G.fit(G.numpy_sweep, np.ones((n, 1)), s1[:, None])
    ph = s1 / (2.0 * n)
    assert f['converged'].all() and f['n_iter'].max() <= 8
    np.testing.assert_allclose(f['beta'][:, 0], np.log(ph / (1 - ph)), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(np.sqrt(f['cov'][:, 0, 0]), 1 / np.sqrt(2 * n * ph * (1 - ph)),
                               rtol=1e-10)
    ll = s1 * np.log(ph) + (2 * n - s1) * np.log(1 - ph)
    np.testing.assert_allclose(f['loglik'], ll, rtol=1e-12)


def test_one_binary_covariate_is_the_log_odds_ratio():
    """through scan, so the coefficient and its standard error come back in the caller's units"""
    c = ACASES.planted()
    D, g = c['D'], c['deme']
    n = D.shape[0]
    a, b = D[g == 1].sum(axis=0), (2 - D[g == 1]).sum(axis=0)
    cc, e = D[g == 0].sum(axis=0), (2 - D[g == 0]).sum(axis=0)
    assert min(a.min(), b.min(), cc.min(), e.min()) > 0
    res = G.scan(AS.numpy_cross(D), G.numpy_sweep, n, 3.0 * g - 1.0)   # x in {-1, 2}
    assert res['tested'].all() and res['converged'].all() and res['df'] == 1
    log_or = np.log(a * e / (b * cc).astype(np.float64))
    se = np.sqrt(1.0 / a + 1.0 / b + 1.0 / cc + 1.0 / e)
    np.testing.assert_allclose(res['beta'][:, 0], log_or / 3.0, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(res['se'][:, 0], se / 3.0, rtol=1e-10)
    np.testing.assert_allclose(res['coef'][:, 0], np.log(cc / e) + log_or / 3.0,
                               rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(res['z'], res['beta'] / res['se'], rtol=1e-14)
    # the saturated model's likelihood ratio: G = 2 sum O log(O / E) of the 2 x 2 table
    O = np.stack([a, b, cc, e]).astype(np.float64)
    tot, row1, row0, col1 = 2.0 * n, a + b, cc + e, a + cc
    E = np.stack([row1 * col1, row1 * (tot - col1), row0 * col1, row0 * (tot - col1)]) / tot
    np.testing.assert_allclose(res['lrt'], 2.0 * (O * np.log(O / E)).sum(axis=0), rtol=1e-8,
                               atol=1e-9)


def test_an_independent_optimiser_agrees():
    """BFGS with the analytic gradient on the negative log-likelihood written out here"""
    c = ACASES.planted()
    Z = G.design(c['env'], c['deme'].astype(np.float64))['Z']
    worst = 0.0
    for l in (0, 13, 110, 333, 599):
        d = c['D'][:, l].astype(np.float64)
        xtd = Z.T @ d

        def nll(b):
            return -(b @ xtd - 2.0 * np.logaddexp(0.0, Z @ b).sum())

        def grad(b):
            return -(xtd - 2.0 * Z.T @ np.exp(Z @ b - np.logaddexp(0.0, Z @ b)))

        opt = optimize.minimize(nll, np.zeros(3), jac=grad, method='BFGS',
                                options=dict(gtol=1e-10))
        f = G.fit(G.numpy_sweep, Z, xtd[None, :])
        assert f['converged'][0]
        se = np.sqrt(np.diagonal(f['cov'][0]))
        worst = max(worst, float((np.abs(opt.x - f['beta'][0]) / se).max()))
        np.testing.assert_allclose(f['loglik'][0], -opt.fun, rtol=1e-12)
    print('fit against BFGS: worst |difference| / se %.3g' % worst)
    assert worst <= 1e-6


def test_the_planted_loci_are_found(planted_scan):
    res = planted_scan
    causal = ACASES.planted()['causal']
    np.testing.assert_array_equal(np.sort(np.argsort(res['p'], kind='stable')[:6]), causal)
    assert res['tested'].all() and res['converged'].all() and res['n_iter'].max() <= 12
    print('logistic scan of the planted case: gif %.4g, at most %d Newton steps, %d sweeps'
          % (res['gif'], res['n_iter'].max(), res['n_sweeps']))
    # gif where the linear scan's check_planted puts the scan that accounts for the demes
    # (< 1.5), and the uncorrected one where it puts the plain scan (> 5)
    c = ACASES.planted()
    plain = G.scan(AS.numpy_cross(c['D']), G.numpy_sweep, 400, c['env'])
    as_t = lambda r: dict(gif=[r['gif']], t=r['z'])                      # noqa: E731
    check_planted(as_t(plain), as_t(res))
    # the pieces hang together
    np.testing.assert_allclose(res['lrt'], 2 * (res['loglik'] - res['loglik_null']), rtol=0,
                               atol=1e-9)
    assert (res['lrt'] > -1e-9).all() and res['beta'].shape == (600, 1)
    np.testing.assert_array_equal(res['q'], AS.bh_qvalues(res['p']))
    from scipy.stats import chi2
    np.testing.assert_allclose(res['p'], chi2.sf(res['lrt'], 1), rtol=1e-12)
    cal = G.scan(AS.numpy_cross(c['D']), G.numpy_sweep, 400, c['env'],
                 c['deme'].astype(np.float64), calibrate=True)
    np.testing.assert_allclose(cal['p'], chi2.sf(res['lrt'] / res['gif'], 1), rtol=1e-12)


def test_loci_below_min_maf_are_not_fitted():
    c = ACASES.planted()
    D = c['D'].copy()
    D[:, 3] = 0
    D[:, 4] = 2
    D[:, 5] = 0
    D[:7, 5] = 1                                       # maf 7 / 800 < 0.01
    res = G.scan(AS.numpy_cross(D), G.numpy_sweep, 400, c['env'])
    assert not res['tested'][[3, 4, 5]].any() and res['tested'].sum() == 597
    for k in ('beta', 'se', 'z', 'p_wald', 'lrt', 'p', 'q'):
        assert np.isnan(res[k][[3, 4, 5]]).all(), k
    assert not res['converged'][[3, 4, 5]].any() and (res['n_iter'][[3, 4, 5]] == 0).all()
    np.testing.assert_allclose(res['maf'][[3, 4, 5]], [0, 0, 7 / 800.0])
    assert np.isfinite(res['q'][res['tested']]).all()


def test_a_separated_locus_is_reported_and_its_neighbours_do_not_move(planted_scan):
    c = ACASES.planted()
    D = c['D'].copy()
    D[:, 5] = np.where(c['env'] - c['env'].mean() > 0, 2, 0)
    res = G.scan(AS.numpy_cross(D), G.numpy_sweep, 400, c['env'], c['deme'].astype(np.float64))
    assert res['tested'][5] and not res['converged'][5] and res['n_iter'][5] == 25
    for k in ('beta', 'se', 'z', 'p_wald', 'lrt', 'p', 'q'):
        v = np.atleast_1d(res[k][5])
        assert (np.isfinite(v) | np.isnan(v)).all(), k
    print('separated locus: beta %r after %d steps' % (res['beta'][5], res['n_iter'][5]))
    others = np.r_[0:5, 6:600]
    for k in ('beta', 'se', 'z', 'p_wald', 'lrt', 'coef', 'cov', 'loglik', 'loglik_null',
              'converged', 'n_iter', 'maf', 'tested'):
        assert np.ascontiguousarray(res[k][others]).tobytes() == \
            np.ascontiguousarray(planted_scan[k][others]).tobytes(), k
    assert res['converged'][others].all()


def test_a_fit_does_not_depend_on_its_company():
    """alone or among the 600, first or last: the driver's bookkeeping of the active set"""
    c = ACASES.planted()
    Z = G.design(c['env'], c['deme'].astype(np.float64))['Z']
    XtD = c['D'].T.astype(np.float64) @ Z
    among = G.fit(G.numpy_sweep, Z, XtD)
    assert len(set(among['n_iter'])) > 1                 # fits leave the batch at different steps
    for k in (0, 13, 333, 599):
        alone = G.fit(G.numpy_sweep, Z, XtD[k:k + 1])
        for key in ('beta', 'cov', 'loglik', 'converged', 'n_iter'):
            assert alone[key].tobytes() == among[key][k:k + 1].tobytes(), (k, key)
    rev = G.fit(G.numpy_sweep, Z, XtD[::-1])
    for key in ('beta', 'cov', 'loglik', 'converged', 'n_iter'):
        assert np.ascontiguousarray(rev[key][::-1]).tobytes() == among[key].tobytes(), key


def test_fit_reports_what_it_cannot_fit():
    """a singular information matrix stops the fit; max_iter = 1 leaves everything unconverged"""
    X = np.column_stack([np.ones(50), np.ones(50)])
    f = G.fit(G.numpy_sweep, X, np.array([[40.0, 40.0]]))
    assert not f['converged'][0] and f['n_iter'][0] == 0 and np.isnan(f['cov']).all()
    c = ACASES.planted()
    res = G.scan(AS.numpy_cross(c['D'][:, :20]), G.numpy_sweep, 400, c['env'], max_iter=1)
    assert not res['converged'].any() and (res['n_iter'] == 1).all()


def test_clines_recover_the_truth():
    """dosages drawn from known clines (tests/_glm.py, CLINE_SEED): at most 1 of the 40 centres
    and 1 of the 40 widths further than 4 standard errors from the truth (measured with this
    seed: none of either)"""
    c = CASES.clines()
    D, x = c['D'], c['x']
    n, L = D.shape
    res = G.scan(AS.numpy_cross(D), G.numpy_sweep, n, x)
    assert res['tested'].all() and res['converged'].all()
    lo, hi = float(x.min()), float(x.max())
    st = G.cline_stats(res['coef'], res['cov'], lo, hi)
    zc = np.abs(st['centre'] - c['centre']) / st['se_centre']
    zw = np.abs(st['width'] - c['width']) / st['se_width']
    print('clines: worst |centre - truth| / se %.3g, worst |width - truth| / se %.3g'
          % (zc.max(), zw.max()))
    assert (zc > 4).sum() <= 1 and (zw > 4).sum() <= 1
    np.testing.assert_array_equal(st['slope_sign'], c['sign'])
    # against the definitions
    b0, b1 = res['coef'][:, 0], res['coef'][:, 1]
    np.testing.assert_array_equal(st['in_range'], (-b0 / b1 >= lo) & (-b0 / b1 <= hi))
    assert st['in_range'].all()
    p_at = lambda v: 1.0 / (1.0 + np.exp(-(b0 + b1 * v)))                # noqa: E731
    np.testing.assert_allclose(st['delta_p'], p_at(hi) - p_at(lo), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(st['width'], 4 / np.abs(b1))
    assert (np.sign(st['delta_p']) == c['sign']).all()
    # a centre outside the sampled range is flagged
    out = G.cline_stats(np.array([[30.0, -2.0], [1.0, 0.0]]), np.tile(np.eye(2), (2, 1, 1)),
                        0.0, 10.0)
    assert not out['in_range'].any() and out['centre'][0] == 15.0
    con = G.concordance(st['centre'], st['width'], st['in_range'])
    assert con['n_loci'] == L and con['median_centre'] == np.median(st['centre'])
    assert con['mad_width'] == np.median(np.abs(st['width'] - np.median(st['width'])))
    assert np.isnan(G.concordance(st['centre'], st['width'], np.zeros(L, bool))['mad_centre'])


# ---- the request checks, on a Species whose handle has no calls --------------------------------
def test_the_new_analyses_refuse_a_species_without_assigned_genomes():
    for who, method in (('run_logistic_gea', '_run_logistic_gea'), ('calc_clines', '_calc_clines')):
        assert _refusal(getattr(_Species(L=0), method)) == '%s: %s' % (who, NO_GENOMES)
        assert _refusal(getattr(_Species(assigned=False), method)) == '%s: %s' % (who, UNASSIGNED)


def test_requests_are_refused_before_the_device_is_asked():
    spp = _Species()
    rng = np.random.RandomState(3)
    env = rng.standard_normal((4, 2))
    gea, cl = spp._run_logistic_gea, spp._calc_clines
    assert _refusal(gea, env=env, env_lyrs=[0]) == \
        'run_logistic_gea: give env_lyrs or env, not both'
    assert 'env: finite values [n = 4][r]' in _refusal(gea, env=np.zeros((5, 1)))
    # more than 7 columns beside the intercept: tested alone, and tested with covariates
    msg = 'a logistic fit takes at most 7 columns beside the intercept'
    assert msg in _refusal(gea, env=rng.standard_normal((4, 8)))
    assert msg in _refusal(gea, env=env, covars=rng.standard_normal((4, 4)), n_pcs=2)
    assert msg in _refusal(cl, covars=rng.standard_normal((4, 7)))
    # a design that is not of full rank is refused by the column's name
    assert _refusal(gea, env=np.column_stack([env[:, 0], 2 * env[:, 0] + 1])) == \
        'run_logistic_gea: the design is rank-deficient: tested variable 1 is a combination ' \
        'of the intercept and the columns before it'
    assert _refusal(gea, env=env, covars=np.full(4, 3.0)) == \
        'run_logistic_gea: the design is rank-deficient: covariate 0 is constant'
    assert 'tested variable 0 is a combination' in \
        _refusal(cl, axis=env[:, 0], covars=-env[:, :1])
    for who, f, kw in (('run_logistic_gea', gea, dict(env=env)), ('calc_clines', cl, {})):
        for bad in (0, -1e-8, 1, float('nan'), True, 'tight'):
            assert _refusal(f, tol=bad, **kw) == \
                '%s: tol: a relative step in (0, 1) (got %r)' % (who, bad)
        for bad in (0, 2.5, True, None):
            assert _refusal(f, max_iter=bad, **kw) == \
                '%s: max_iter: at least 1 iteration (got %r)' % (who, bad)
    assert 'n_pcs: a number of genetic PCs >= 0' in _refusal(gea, env=env, n_pcs=-1)
    for bad in ('z', ('env',), ('layer', 0), True, float('inf'), np.zeros(5), [1.0, np.nan, 2, 3],
                None):
        assert _refusal(cl, axis=bad).startswith("calc_clines: axis: 'x', 'y', ('env', lyr), ")
    for bad in (0, -1.0, True, float('inf')):
        assert _refusal(cl, sigma=bad) == \
            'calc_clines: sigma: a positive dispersal distance (got %r)' % (bad,)


def test_scan_refuses_what_the_device_would_refuse_later():
    c = ACASES.planted()
    cross = AS.numpy_cross(c['D'])
    with pytest.raises(ValueError, match='at most 7 columns beside the intercept'):
        G.scan(cross, G.numpy_sweep, 400, np.zeros((400, 5)), np.zeros((400, 3)))
    with pytest.raises(ValueError, match='must be finite'):
        G.scan(cross, G.numpy_sweep, 400, np.r_[np.nan, c['env'][1:]])
    with pytest.raises(ValueError, match='no variable to test'):
        G.scan(cross, G.numpy_sweep, 400, np.zeros((400, 0)))


# ---- the C ABI --------------------------------------------------------------------------------
def test_the_prototype_parses_and_the_library_exports_it():
    dbl, i64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    by_hand = {'gnx_glm_sweep': (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, dbl, C.c_int64, dbl,
                                           dbl, i64, i64, dbl]),
               'gnx_glm_budget': (C.c_int, [C.c_void_p, C.c_int64])}
    assert nat.PROTOTYPES_EXT == by_hand
    assert not set(by_hand) & set(nat.PROTOTYPES) and not set(by_hand) & set(nat.EXPORTS)
    lib = nat.load()
    for name, (restype, argtypes) in by_hand.items():
        fn = getattr(lib, name)                       # AttributeError: the library lacks it
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
