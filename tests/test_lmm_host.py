"""The host algebra of the mixed-model association scan (geonomics_amd/sim/assoc.py: lmm_rotation,
lmm_design, lmm_table, lmm_scan_stats, lmm_scan) with numpy standing in for the two device calls
(numpy_cross, numpy_quad), against the dense brute force of tests/_lmm.py.  No GPU."""
import numpy as np
import pytest

import _lmm as LT
from geonomics_amd.sim import assoc as A

N, L = 120, 300


@pytest.fixture(scope='module')
def sample():
    """a two-deme sample with full sibs, its relationship matrix and eigendecomposition, two
    covariates and a response with a deme effect, three causal loci and noise"""
    rng = np.random.RandomState(20)
    D, deme = LT.structured_sample(rng, N, L, fst=0.1)
    G = LT.grm_dense(D)
    evals, U = np.linalg.eigh(G)
    C = np.column_stack([rng.standard_normal(N), rng.rand(N) + 0.3 * deme])
    y = 0.8 * deme + D[:, [5, 100, 222]] @ np.array([0.4, -0.3, 0.5]) + rng.standard_normal(N)
    return dict(D=D, deme=deme, G=G, evals=evals, U=U, C=C, y=y)


def _scan(s, delta, C=None, **kw):
    X = np.column_stack([np.ones(N)] + ([] if C is None else [C]))
    M = A.lmm_rotation(s['evals'], s['U'], delta)
    return A.lmm_scan(A.numpy_cross(s['D']), A.numpy_quad(s['D']), N, s['y'], X, M, **kw)


@pytest.mark.parametrize('with_covars', [False, True])
@pytest.mark.parametrize('delta', [0.1, 1.0, 10.0])
def test_scan_equals_the_dense_brute_force(sample, delta, with_covars):
    """both sides fp64.  Largest relative gaps measured over the six cases: beta 3.5e-12,
    se 1.3e-13, t 9.3e-14 (of max(|t|, 1)), p 1.9e-13; the tolerance is ten times the largest,
    3.5e-11"""
    s = sample
    C = s['C'] if with_covars else None
    res = _scan(s, delta, C)
    ref = LT.lmm_brute(s['D'], s['y'], C, s['G'], delta)
    assert res['df'] == ref['df'] == N - (3 if with_covars else 1) - 1
    tested = res['tested']
    assert tested.sum() > 250 and res['t'].shape == (L, 1)
    gaps = {}
    for k in ('beta', 'se', 't', 'p'):
        a, b = res[k][tested, 0], ref[k][tested]
        scale = np.maximum(np.abs(b), 1.0) if k == 't' else np.abs(b)
        gaps[k] = float((np.abs(a - b) / scale).max())
    print('lmm host delta %g covars %s: ' % (delta, with_covars)
          + ', '.join('%s %.3g' % kv for kv in gaps.items()))
    assert all(v <= 3.5e-11 for v in gaps.values()), gaps


def test_a_large_delta_gives_the_ols_scan(sample):
    """V = delta (I + G / delta): at delta = 10^12 the whitened model is the ordinary one up to a
    relative change of at most lambda_max / delta in every inner product of two columns.  t is a
    ratio of products of such inner products after the covariates are projected out, which
    multiplies the change by the conditioning of that projection; 100 covers four factors and a
    conditioning of 25 (a dosage that keeps 4 % of its variance beside the covariates)"""
    s = sample
    delta = 1e12
    tol = 100.0 * s['evals'].max() / delta
    for C in (None, s['C']):
        res = _scan(s, delta, C)
        ols = A.scan(A.numpy_cross(s['D']), N, s['y'], C)
        assert res['df'] == ols['df']
        np.testing.assert_array_equal(res['tested'], ols['tested'])
        tt = res['tested']
        gap = np.abs(res['t'][tt] - ols['t'][tt]) / np.maximum(np.abs(ols['t'][tt]), 1.0)
        print('lmm host delta 1e12: gap %.3g, tolerance %.3g' % (gap.max(), tol))
        assert gap.max() <= tol
        assert res['gif'][0] == pytest.approx(ols['gif'][0], rel=10 * tol)


def test_nan_rules(sample):
    s = sample
    D = s['D'].copy()
    D[:, 0] = 0                                  # monomorphic
    D[:, 1] = 2
    D[:, 2] = 1                                  # every individual heterozygous: no variance
    D[:, 3] = 0
    D[7, 3] = 1                                  # maf = 1 / 240 < 0.01
    C = np.column_stack([s['C'], D[:, 9]])       # locus 9 is a covariate: collinear
    X = np.column_stack([np.ones(N), C])
    M = A.lmm_rotation(s['evals'], s['U'], 1.0)
    res = A.lmm_scan(A.numpy_cross(D), A.numpy_quad(D), N, s['y'], X, M)
    bad = np.array([0, 1, 2, 3, 9])
    assert not res['tested'][bad].any() and res['tested'].sum() == L - bad.size
    for k in ('beta', 'se', 't', 'p', 'q'):
        assert np.isnan(res[k][bad]).all() and np.isfinite(res[k][res['tested']]).all(), k
    assert res['maf'][3] == pytest.approx(1 / 240) and res['maf'][2] == 0.5
    tt = res['tested']
    assert res['gif'][0] == A.genomic_inflation(res['t'][tt, 0])
    np.testing.assert_array_equal(res['q'][tt, 0], A.bh_qvalues(res['p'][tt, 0]))
    # the table is zero where nothing is tested, and the loci quad is asked for are the
    # integers' choice
    use, _ = A.lmm_testable(D.sum(0), (D * D).sum(0), N)
    assert not use[[0, 1, 2, 3]].any() and use[9]
    val = A.lmm_table(D.sum(0), N, use)
    assert val.dtype == np.float32 and val.shape == (L, 3) and not val[[0, 1, 2, 3]].any()
    c9 = A.lmm_centre(D[:, 9].sum(), N)
    assert abs(c9 - D[:, 9].mean()) <= 2.0 ** -21
    np.testing.assert_array_equal(val[9].astype(np.float64), np.arange(3.0) - c9)   # exact
    # with min_maf = 0 the rare locus is tested
    res0 = A.lmm_scan(A.numpy_cross(D), A.numpy_quad(D), N, s['y'], X, M, min_maf=0.0)
    assert res0['tested'][3] and not res0['tested'][[0, 1, 2, 9]].any()
    # calibrate: p from t^2 / gif
    resc = A.lmm_scan(A.numpy_cross(D), A.numpy_quad(D), N, s['y'], X, M, calibrate=True)
    np.testing.assert_allclose(resc['p'][tt, 0],
                               A.calibrated_p(res['t'][tt, 0], res['gif'][0]), rtol=1e-12)


def test_refusals(sample):
    s = sample
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='delta: a positive, finite'):
            A.lmm_rotation(s['evals'], s['U'], bad)
    with pytest.raises(ValueError, match=r'evals \[n\] and U'):
        A.lmm_rotation(s['evals'][:-1], s['U'], 1.0)
    M = A.lmm_rotation(s['evals'], s['U'], 1.0)
    X = np.column_stack([np.ones(N), s['C']])
    with pytest.raises(ValueError, match='combination of the covariates'):
        A.lmm_design(X @ np.array([1.0, 2.0, -3.0]), X, M)
    with pytest.raises(ValueError, match='combination of the covariates'):
        A.lmm_design(np.full(N, 4.0), X, M)
    with pytest.raises(ValueError, match='one response'):
        A.lmm_design(np.ones((N, 2)), X, M)
    with pytest.raises(ValueError, match='must be finite'):
        A.lmm_design(np.where(np.arange(N) == 3, np.nan, s['y']), X, M)
    dsn = A.lmm_design(s['y'], X, M)
    assert dsn['rank'] == 3 and dsn['A'].shape == (N, 4) and dsn['xx'] > 0
    # a duplicated covariate does not change the rank, and so not df
    assert A.lmm_design(s['y'], np.column_stack([X, X[:, 1]]), M)['rank'] == 3
    # negative eigenvalues (rounding of a singular G) are clamped at 0
    np.testing.assert_array_equal(A.lmm_rotation([-1e-12, 2.0], np.eye(2), 0.5),
                                  np.diag(1.0 / np.sqrt([0.5, 2.5])))


def test_the_mixed_model_calibrates_a_structured_sample():
    """a phenotype with a deme effect and no causal locus in two demes at Fst = 0.1 (n = 240,
    L = 600, seed 4): the OLS scan's gif is 8.13, the mixed model's 0.91 at the REML delta 2.11"""
    from geonomics_amd.sim import quantgen as Q
    rng = np.random.RandomState(4)
    n, Lc = 240, 600
    D, deme = LT.structured_sample(rng, n, Lc, fst=0.1)
    y = 1.0 * deme + rng.standard_normal(n)
    ols = A.scan(A.numpy_cross(D), n, y)
    evals, U = np.linalg.eigh(LT.grm_dense(D))
    X = np.ones((n, 1))
    fit = Q.reml(evals, U, y, X)
    res = A.lmm_scan(A.numpy_cross(D), A.numpy_quad(D), n, y, X,
                     A.lmm_rotation(evals, U, fit['delta']))
    print('calibration: gif OLS %.3f, LMM %.3f at delta %.3g (h2 %.3f)'
          % (ols['gif'][0], res['gif'][0], fit['delta'], fit['h2']))
    assert ols['gif'][0] > 1.5
    assert abs(res['gif'][0] - 1.0) < abs(ols['gif'][0] - 1.0)


def test_the_symbol_is_declared_and_bound():
    from geonomics_amd import _native
    assert 'gnx_assoc_quad' in _native.EXPORTS and callable(_native.Device.assoc_quad)
