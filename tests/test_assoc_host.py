"""The host arithmetic of the association scans (geonomics_amd/sim/assoc.py) and the public
surface of Model.run_gwas / run_lfmm, without a GPU: the scan's statistics against a per-locus
least-squares fit that shares nothing with it, the loci that are not tested, the latent factors
against the dense LFMM2 construction, Benjamini-Hochberg and the inflation factor on vectors
worked by hand, and the planted case of tests/_assoc.py."""
import inspect

import numpy as np
import pytest

import _assoc as CASES
from test_analyses_host import _Species, _refusal
from geonomics_amd.sim import assoc as AS


@pytest.fixture(scope='module')
def fit_case():
    """n = 300, L = 130, 3 covariates, 3 tested variables (correlated with the covariates)"""
    rng = np.random.RandomState(3)
    n, L = 300, 130
    D = CASES.random_dosages(n, L, 5)
    C = rng.standard_normal((n, 3))
    X = rng.standard_normal((n, 3)) + C[:, :1]
    return D, C, X


@pytest.mark.parametrize('kind', ['gwas', 'gea'])
def test_scan_is_the_per_locus_least_squares_fit(fit_case, kind):
    """beta and t of the coefficient of interest in the full design [1, C, g] (GWAS) or
    [1, C, x] with g as response (GEA), to 1e-8 relative: the design is well conditioned, the
    margin only says 'same quantity' (measured: 1.6e-11)"""
    D, C, X = fit_case
    n = D.shape[0]
    res = AS.scan(AS.numpy_cross(D), n, X, C, kind)
    beta, t = (CASES.lstsq_gwas if kind == 'gwas' else CASES.lstsq_gea)(D, C, X)
    assert res['tested'].all() and res['df'] == n - 3 - 2
    worst_b = np.abs(res['beta'] / beta - 1.0).max()
    worst_t = np.abs(res['t'] / t - 1.0).max()
    print('%s: worst relative difference beta %.3g, t %.3g' % (kind, worst_b, worst_t))
    assert worst_b <= 1e-8 and worst_t <= 1e-8
    np.testing.assert_allclose(res['se'], res['beta'] / res['t'], rtol=1e-12)
    from scipy.stats import t as t_dist
    np.testing.assert_allclose(res['p'], 2.0 * t_dist.sf(np.abs(t), n - 5), rtol=1e-6)


def test_the_mutual_scan_conditions_every_variable_on_the_others(fit_case):
    """run_lfmm's design: x_k given C and the other tested variables"""
    D, C, X = fit_case
    res = AS.scan(AS.numpy_cross(D), D.shape[0], X, C, 'gea', mutual=True)
    assert res['df'] == D.shape[0] - 5 - 2
    for k in range(3):
        beta, t = CASES.lstsq_gea(D, np.column_stack([C, np.delete(X, k, axis=1)]),
                                  X[:, k:k + 1])
        assert np.abs(res['beta'][:, k] / beta[:, 0] - 1.0).max() <= 1e-8
        assert np.abs(res['t'][:, k] / t[:, 0] - 1.0).max() <= 1e-8


def test_loci_that_are_not_tested_get_nan(fit_case):
    D, C, X = fit_case
    D = D.copy()
    C = C.copy()
    n = D.shape[0]
    D[:, 4] = 0
    D[:, 9] = 2
    D[:, 20] = 0
    D[:5, 20] = 1                         # maf = 5 / 600 < 0.01
    C[:, 2] = D[:, 33]                    # locus 33 is an exact copy of a covariate
    off = [4, 9, 20, 33]
    # (the ordered restatement: a locus' sums do not depend on the other loci, as on the device)
    res = AS.scan(lambda Y: AS.ordered_cross(D, Y), n, X, C, 'gwas')
    assert not res['tested'][off].any() and res['tested'].sum() == D.shape[1] - 4
    for k in ('beta', 'se', 't', 'p', 'q'):
        assert np.isnan(res[k][off]).all(), k
        assert np.isfinite(np.delete(res[k], off, axis=0)).all(), k
    # they stay out of gif and q: the same numbers as a scan of the other loci alone
    keep = np.setdiff1d(np.arange(D.shape[1]), off)
    sub = AS.scan(lambda Y: AS.ordered_cross(D[:, keep], Y), n, X, C, 'gwas')
    np.testing.assert_array_equal(sub['gif'], res['gif'])
    np.testing.assert_array_equal(sub['q'], res['q'][keep])
    # with min_maf = 0 the rare locus is tested; the all-2 locus is still decided on the integers
    res0 = AS.scan(AS.numpy_cross(D), n, X, C, 'gwas', min_maf=0.0)
    assert res0['tested'][20] and not res0['tested'][[4, 9, 33]].any()


@pytest.mark.parametrize('K', [1, 3])
def test_latent_factors_span_the_dense_construction(K):
    """n = 120, L = 400: the factors from the Gram matrix against Q_x diag(1 / d) times the top-K
    left singular vectors of the dense diag(d) Q_x^T H D: cosines of the principal angles"""
    rng = np.random.RandomState(10 + K)
    n, L = 120, 400
    grp = rng.randint(0, K + 1, n)
    shift = rng.normal(0.0, 0.2, size=(K + 1, L))
    P = np.clip(rng.uniform(0.2, 0.8, L)[None, :] + shift[grp], 0.02, 0.98)
    D = ((rng.uniform(size=(n, L)) < P).astype(np.int64)
         + (rng.uniform(size=(n, L)) < P).astype(np.int64))
    X = np.column_stack([grp + rng.standard_normal(n), rng.standard_normal(n)])
    U = AS.latent_factors(D @ D.T, X, K, lam=1e-5)
    assert U.shape == (n, K)
    Qx, d = AS.lfmm_weights(X, 1e-5)
    assert (d[:2] < 1e-3).all() and (d[2:] == 1.0).all()
    Dc = D - D.mean(axis=0)
    u = np.linalg.svd((Qx * d[None, :]).T @ Dc, full_matrices=False)[0][:, :K]
    ref = (Qx / d[None, :]) @ u
    cos = np.linalg.svd(np.linalg.qr(U)[0].T @ np.linalg.qr(ref)[0], compute_uv=False)
    print('K = %d: 1 - smallest cosine %.3g' % (K, 1.0 - cos.min()))
    assert cos.min() >= 1.0 - 1e-9
    assert AS.latent_factors(D @ D.T, X, 0).shape == (n, 0)


def test_bh_qvalues_by_hand():
    """four tests among six entries: sorted p 0.01, 0.03, 0.04, 0.5 times 4 / rank = 0.04, 0.06,
    0.0533.., 0.5; the running minimum from the right gives 0.04, 0.0533.., 0.0533.., 0.5"""
    p = np.array([0.01, np.nan, 0.04, 0.03, np.nan, 0.5])
    q = AS.bh_qvalues(p)
    assert np.isnan(q[[1, 4]]).all()
    np.testing.assert_allclose(q[[0, 2, 3, 5]], [0.04, 0.16 / 3, 0.16 / 3, 0.5], rtol=1e-15)
    assert np.isnan(AS.bh_qvalues(np.full(3, np.nan))).all()
    q2 = AS.bh_qvalues(np.column_stack([p, p[::-1]]))
    np.testing.assert_array_equal(q2[:, 0], q)
    np.testing.assert_array_equal(q2[:, 1], q[::-1])
    np.testing.assert_array_equal(AS.bh_qvalues(np.array([0.9, 0.8])), [0.9, 0.9])


def test_genomic_inflation_of_a_known_median():
    from scipy.stats import chi2
    med = chi2.ppf(0.5, 1)
    t = np.array([np.nan, -3.0, 0.1, np.sqrt(2.0 * med), np.nan, -0.2, 5.0])
    assert abs(AS.genomic_inflation(t) - 2.0) <= 4e-16 * 2.0
    two = AS.genomic_inflation(np.column_stack([t, t / np.sqrt(2.0)]))
    np.testing.assert_allclose(two, [2.0, 1.0], rtol=1e-15)
    # calibrated p: t^2 / gif against chi-square with 1 df
    np.testing.assert_allclose(AS.calibrated_p(np.array([np.sqrt(2.0 * med)]), 2.0), [0.5],
                               rtol=1e-12)


def planted_scans(cross):
    """the plain scan and the scan with one latent factor of the planted case"""
    c = CASES.planted()
    D, env = c['D'], c['env']
    n = D.shape[0]
    plain = AS.scan(cross, n, env, None, 'gea', True)
    U = AS.latent_factors(D @ D.T, env, 1)
    return plain, AS.scan(cross, n, env, U, 'gea', True, calibrate=True), U


def check_planted(plain, lfmm):
    """the three conditions of the planted case: computed on the CPU, gif 14.2 and 1.12"""
    causal = CASES.planted()['causal']
    assert plain['gif'][0] > 5.0
    assert lfmm['gif'][0] < 1.5
    for res in (plain, lfmm):
        np.testing.assert_array_equal(CASES.top_by_abs_t(res['t'][:, 0], 6), causal)


def test_the_planted_loci_are_found_and_one_factor_removes_the_inflation():
    c = CASES.planted()
    plain, lfmm, U = planted_scans(AS.numpy_cross(c['D']))
    corr = abs(np.corrcoef(U[:, 0], c['deme'])[0, 1])
    print('gif %.4g plain, %.4g with K = 1; |corr(U, deme)| %.4g'
          % (plain['gif'][0], lfmm['gif'][0], corr))
    check_planted(plain, lfmm)
    assert plain['tested'].all() and lfmm['df'] == plain['df'] - 1


def test_stretch_rule_and_the_ordered_restatement():
    """the order is a function of (n, L); the ordered restatement meets the any-order bound"""
    assert AS.stretch_rule(1, 1) == (64, 1)
    assert AS.stretch_rule(129, 65) == (64, 3)
    assert AS.stretch_rule(5125, 70) == (192, 27)
    assert AS.stretch_rule(8192, 100000) == (448, 19)
    assert AS.stretch_rule(10 ** 6, 10 ** 5) == (50048, 20)
    assert AS.stretch_rule(10 ** 6, 3 * 10 ** 6) == (10 ** 6, 1)
    D, Y = CASES.cross_case(129, 65, 16)
    got = AS.ordered_cross(D, Y)
    exact, s1, s2, ab = AS.brute_cross(D, Y)
    np.testing.assert_array_equal(got['s1'], s1)
    np.testing.assert_array_equal(got['s2'], s2)
    assert (np.abs(got['DtY'] - exact) <= 128 * 2.0 ** -53 * ab).all()
    assert (got['DtY'][:, 8] == 0.0).all()


def test_public_surface():
    from geonomics_amd import _native
    from geonomics_amd.sim.model import Model
    from geonomics_amd.structs.species import Species
    from geonomics_amd.structs.tiled import _NOT_TILED, TiledSpecies
    assert str(inspect.signature(Model.run_gwas)) == \
        '(self, trt=0, spp=0, y=None, covars=(), n_pcs=0, individs=None, n=None, loci=None, ' \
        'min_maf=0.01, calibrate=False)'
    assert str(inspect.signature(Model.run_lfmm)) == \
        '(self, K, spp=0, env_lyrs=None, lam=1e-05, individs=None, n=None, loci=None, ' \
        'min_maf=0.01, calibrate=True)'
    assert 'gnx_assoc_cross' in _native.EXPORTS and callable(_native.Device.assoc_cross)
    for name in ('_run_gwas', '_run_lfmm'):
        assert name in _NOT_TILED and callable(getattr(Species, name))
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            getattr(TiledSpecies, name)(object())


def test_the_requests_are_refused_before_the_device_is_asked():
    """the stand-in's handle has no calls: a check behind a device call would fail differently"""
    assert _refusal(_Species(L=0)._run_gwas) == \
        'run_gwas: the Species has no genomes (no gen_arch)'
    assert _refusal(_Species(L=0)._run_lfmm, 1) == \
        'run_lfmm: the Species has no genomes (no gen_arch)'
    assert _refusal(_Species(assigned=False)._run_gwas) == \
        'run_gwas: genomes are assigned at the end of the burn-in; burn the model in first'
    assert _refusal(_Species(assigned=False)._run_lfmm, 1) == \
        'run_lfmm: genomes are assigned at the end of the burn-in; burn the model in first'
    # more than 32 columns: 32 covariates and one response; 29 factors and two layers twice
    assert 'at most 32 columns' in _refusal(_Species()._run_gwas, y=np.arange(4.0),
                                            covars=np.ones((4, 32)))
    assert 'at most 32 columns' in _refusal(_Species()._run_gwas, y=np.arange(4.0), n_pcs=3,
                                            covars=[np.ones((4, 20)), np.ones((4, 9))])
    assert 'at most 32 columns' in _refusal(_Species()._run_lfmm, 29, env=np.ones((4, 2)))
    assert 'no Trait 5' in _refusal(_Species()._run_gwas, 5)
    assert 'covars' in _refusal(_Species()._run_gwas, y=np.arange(4.0), covars='z')
    assert 'y: finite values [n = 4]' in _refusal(_Species()._run_gwas, y=np.arange(5.0))
    assert 'K: a number of latent factors' in _refusal(_Species()._run_lfmm, -1)

    class _Many(_Species):
        def _geno_sample(self, individs):
            return np.arange(8193, dtype=np.int64), np.arange(8193, dtype=np.int64)

    msg = _refusal(_Many()._run_lfmm, 2)
    assert msg.startswith('run_lfmm: at most 8192 individuals') and 'n=' in msg and \
        'individs=' in msg
