"""The host arithmetic of the quantitative-genetics analyses (geonomics_amd/sim/quantgen.py) and
the Species' request checks, against the dense brute force of tests/_quantgen.py.  No device:
the Species' calls run over a numpy stand-in of the handle."""
import inspect
import types

import numpy as np
import pytest

import _quantgen as QT
from geonomics_amd import _native as nat
from geonomics_amd.sim import quantgen as Q
from geonomics_amd.structs.analyses import SpeciesAnalyses

N, L = 300, 1500


# ------------------------------------------------------------------ grm_values
def _counts(rng, n, L):
    """random counts with every edge: absent, fixed, singletons, near 0 and 1, at min_maf"""
    c1 = rng.randint(0, 2 * n + 1, L)
    c1[:12] = [0, 2 * n, 1, 2 * n - 1, 2, 2 * n - 2, 5, 6, 7, 2 * n - 5, 2 * n - 6, 2 * n - 7]
    return c1


@pytest.mark.parametrize('kind,method,alpha', [('additive', 'gcta', -1.0),
                                               ('additive', 'vanraden', -1.0),
                                               ('additive', 'alpha', -0.25),
                                               ('additive', 'alpha', 0.5),
                                               ('dominance', 'gcta', -1.0)])
@pytest.mark.parametrize('min_maf', [0.0, 0.01, 0.2])
def test_grm_values_against_the_direct_formula(kind, method, alpha, min_maf):
    rng = np.random.RandomState(3)
    n = 300                                     # min_maf 0.01 = 6 / 600: counts 5, 6, 7 straddle it
    c1 = _counts(rng, n, 400)
    val, used = Q.grm_values(c1, n, kind, method, alpha, min_maf)
    ref, ref_used = QT.table_direct(c1, n, kind, method, alpha, min_maf)
    assert val.dtype == np.float32 and val.shape == (400, 3)
    np.testing.assert_array_equal(used, ref_used)
    assert not used[0] and not used[1]          # monomorphic
    assert used[2] == used[3] == (min_maf <= 1 / 600)
    assert used[6] == used[9] == (min_maf <= 5 / 600)       # 5 / 600 is out at 0.01,
    assert used[7] == used[10] == (min_maf <= 0.01)         # 6 / 600 is in: the edge counts
    assert used[8] == used[11] == (min_maf <= 7 / 600)
    assert (val[~used] == 0).all()
    np.testing.assert_allclose(val, ref, rtol=2.0 ** -23, atol=0)   # one rounding to fp32
    if kind == 'additive' and method == 'alpha' and alpha == -0.25:
        a1 = Q.grm_values(c1, n, 'additive', 'alpha', -1.0, min_maf)[0]
        np.testing.assert_array_equal(a1, Q.grm_values(c1, n, min_maf=min_maf)[0])
        a0 = Q.grm_values(c1, n, 'additive', 'alpha', 0.0, min_maf)[0]
        np.testing.assert_allclose(a0, Q.grm_values(c1, n, method='vanraden', min_maf=min_maf)[0],
                                   rtol=2.0 ** -22)


def test_values_have_mean_zero_and_the_matrix_a_unit_diagonal_under_hardy_weinberg():
    rng = np.random.RandomState(4)
    n = 500
    c1 = _counts(rng, n, 300)
    p = c1 / (2.0 * n)
    hw = np.stack([(1 - p) ** 2, 2 * p * (1 - p), p ** 2], 1)
    for kind in ('additive', 'dominance'):
        val, used = QT.table_direct(c1, n, kind)
        m = used.sum()
        mean = (hw * val).sum(1)
        var = (hw * val ** 2).sum(1)
        assert np.abs(mean[used]).max() < 1e-14 * np.abs(val).max()
        np.testing.assert_allclose(var[used] * m, 1.0, rtol=1e-12)     # E diag G = 1
        got = Q.grm_values(c1, n, kind)[0].astype(np.float64)
        assert np.abs((hw * got).sum(1)).max() < 2.0 ** -22 * np.abs(val).max()


def test_subset_and_weights():
    rng = np.random.RandomState(5)
    c1 = _counts(rng, 100, 200)
    subset = rng.rand(200) < 0.5
    w = rng.rand(200) + 0.5
    val, used = Q.grm_values(c1, 100, subset=subset, weights=w)
    ref, ref_used = QT.table_direct(np.where(subset, c1, 0), 100)
    np.testing.assert_array_equal(used, ref_used)
    np.testing.assert_allclose(val, ref * w[:, None], rtol=2.0 ** -23)


# ------------------------------------------------------------------ reml, he, gblup
@pytest.fixture(scope='module')
def sample():
    """n = 300 individuals at 1500 loci, their GCTA matrix and its eigendecomposition"""
    rng = np.random.RandomState(11)
    p = rng.uniform(0.05, 0.95, L)
    D = (rng.rand(N, L, 2) < p[None, :, None]).sum(2)
    G, used, Z = QT.grm_from_dosages(D, fp32=False)
    evals, U = Q.eig_grm(G)
    u = rng.standard_normal(L)
    g = Z @ u
    g = g / g.std()
    e = rng.standard_normal(N)
    X2 = np.column_stack([np.ones(N), rng.standard_normal((N, 2))])
    return dict(G=G, Z=Z, evals=evals, U=U, g=g, e=e / e.std(), X1=np.ones((N, 1)), X2=X2,
                bX=X2 @ np.array([0.7, -1.3, 0.4]))


def _response(s, h2, covars):
    if h2 == 0:
        y = s['e'].copy()
    elif h2 == 1:
        y = s['g'].copy()
    else:
        y = np.sqrt(h2) * s['g'] + np.sqrt(1 - h2) * s['e']
    return (y + s['bX'], s['X2']) if covars else (y, s['X1'])


@pytest.mark.parametrize('covars', [False, True], ids=['intercept', 'two_covars'])
@pytest.mark.parametrize('h2', [0, 0.5, 1])
def test_reml_against_the_dense_brute_force(sample, h2, covars):
    s = sample
    y, X = _response(s, h2, covars)
    got = Q.reml(s['evals'], s['U'], y, X)
    ref = QT.reml_brute(s['G'], y, X)
    print('h2 %s covars %s: reml %.9f brute %.9f  logL %.10f %.10f  x %.6f boundary %s se %s'
          % (h2, covars, got['h2'], ref['h2'], got['logL'], ref['logL'], np.log10(got['delta']),
             got['at_boundary'], got['se_h2']))
    assert abs(got['logL'] - ref['logL']) <= 1e-8 * abs(ref['logL'])
    assert abs(got['logL0'] - ref['logL0']) <= 1e-8 * abs(ref['logL0'])
    assert abs(got['h2'] - ref['h2']) <= 1e-6
    assert got['at_boundary'] == ref['at_boundary']
    # the dense likelihood at the returned components is the returned maximum
    dense = QT.reml_logl_dense(s['G'], y, X, got['Vg'], got['Ve'])
    assert abs(dense - got['logL']) <= 1e-8 * abs(dense)
    assert got['logL'] >= got['logL0'] - 1e-8 * abs(got['logL0'])
    from scipy.stats import chi2
    assert got['lrt_p'] == pytest.approx(0.5 * chi2.sf(max(2 * (got['logL'] - got['logL0']), 0), 1))
    Vi = np.linalg.inv(got['Vg'] * s['G'] + got['Ve'] * np.eye(N))
    beta = np.linalg.solve(X.T @ Vi @ X, X.T @ Vi @ y)
    np.testing.assert_allclose(got['beta'], beta, rtol=1e-7, atol=1e-9)
    if h2 == 1:
        assert got['h2'] > 0.5 and got['lrt_p'] < 1e-3
    elif h2 == 0.5:
        assert not got['at_boundary'] and 0.2 < got['h2'] < 0.8
        se = QT.se_h2_numeric(s['G'], y, X, got['Vg'], got['Ve'])
        print('se_h2 %.8f numeric %.8f' % (got['se_h2'], se))
        assert abs(got['se_h2'] - se) <= 1e-4 * se
        assert got['lrt_p'] < 1e-3
    if covars and h2 == 0.5:
        np.testing.assert_allclose(got['beta'], [0.7, -1.3, 0.4], atol=0.3)


def test_reml_reaches_the_lower_boundary(sample):
    """a response whose variance along the eigenvectors grows faster than their eigenvalues (as
    s^2, where sg2 G alone gives s): the likelihood rises as delta falls, down to the end of the
    interval"""
    s = sample
    rng = np.random.RandomState(6)
    y = s['U'] @ (rng.standard_normal(N) * s['evals'].clip(0))
    got = Q.reml(s['evals'], s['U'], y, s['X1'])
    ref = QT.reml_brute(s['G'], y, s['X1'])
    assert got['at_boundary'] and ref['at_boundary'] and got['delta'] == 1e-10
    assert got['h2'] > 1 - 1e-9 and got['lrt_p'] < 1e-10
    assert abs(got['logL'] - ref['logL']) <= 1e-8 * abs(ref['logL'])


def test_reml_reaches_the_upper_boundary(sample):
    """noise shaped against G, with more variance along the small eigenvalues than white noise
    has: the likelihood rises with delta up to the end of the interval, where it meets the fit
    without a genetic component"""
    s = sample
    rng = np.random.RandomState(2)
    y = s['U'] @ (rng.standard_normal(N) / np.sqrt(1.0 + 3.0 * s['evals'].clip(0)))
    got = Q.reml(s['evals'], s['U'], y, s['X1'])
    ref = QT.reml_brute(s['G'], y, s['X1'])
    assert got['at_boundary'] and ref['at_boundary'] and got['delta'] == 1e10
    assert got['h2'] < 1e-9 and got['lrt_p'] == pytest.approx(0.5, abs=1e-6)
    assert abs(got['logL'] - ref['logL']) <= 1e-8 * abs(ref['logL'])
    assert abs(got['logL'] - got['logL0']) <= 1e-6


def test_he_regression(sample):
    s = sample
    for h2, covars in ((0.5, False), (0.5, True), (0, False)):
        y, X = _response(s, h2, covars)
        got = Q.he_regression(s['G'], y, X)
        assert got == pytest.approx(QT.he_dense(s['G'], y, X), rel=1e-9, abs=1e-12)
    assert np.isnan(Q.he_regression(np.eye(5), np.arange(5.0)))


@pytest.mark.parametrize('covars', [False, True], ids=['intercept', 'two_covars'])
def test_gblup_against_the_dense_blup_and_the_marker_effect_form(sample, covars):
    s = sample
    y, X = _response(s, 0.5, covars)
    for delta in (0.3, 1.0, 7.0):
        got = Q.gblup(s['evals'], s['U'], y, X, delta=delta)
        ref, beta = QT.blup_dense(s['G'], y, X, delta)
        scale = np.abs(ref).max()
        assert np.abs(got['g_hat'] - ref).max() <= 1e-9 * scale
        np.testing.assert_allclose(got['beta'], beta, rtol=1e-9, atol=1e-12)
        mk = QT.blup_marker(s['Z'], y, X, delta, beta)
        assert np.abs(got['g_hat'] - mk).max() <= 1e-9 * scale
        np.testing.assert_allclose(got['y_hat'], X @ beta + ref, rtol=1e-9, atol=1e-9 * scale)
        assert got['fit'] is None
    fitted = Q.gblup(s['evals'], s['U'], y, X)
    assert fitted['delta'] == Q.reml(s['evals'], s['U'], y, X)['delta']


def test_gblup_predicts_the_untrained_from_a_fit_on_the_trained(sample):
    s = sample
    y, X = _response(s, 0.5, True)
    rng = np.random.RandomState(8)
    train = np.sort(rng.choice(N, 200, replace=False))
    rest = np.setdiff1d(np.arange(N), train)
    y_in = y.copy()
    y_in[rest] = np.nan                              # never read
    got = Q.gblup(s['evals'], s['U'], y_in, X, train=train)
    sub = QT.reml_brute(s['G'][np.ix_(train, train)], y[train], X[train])
    assert abs(got['fit']['h2'] - sub['h2']) <= 1e-6
    ref, beta = QT.blup_dense(s['G'], y, X, got['delta'], train)
    assert np.abs(got['g_hat'] - ref).max() <= 1e-9 * np.abs(ref).max()
    np.testing.assert_allclose(got['beta'], beta, rtol=1e-8)
    assert np.isfinite(got['g_hat']).all() and np.isfinite(got['y_hat']).all()
    assert np.corrcoef(got['g_hat'][rest], s['g'][rest])[0, 1] > 0
    for bad in ([0], [0, 0, 1], [0, N], [-1, 2]):
        with pytest.raises(ValueError, match='train'):
            Q.gblup(s['evals'], s['U'], y, X, train=bad)


def test_argument_checks_of_the_pure_functions(sample):
    s = sample
    with pytest.raises(ValueError, match="kind: 'additive' or 'dominance'"):
        Q.grm_values(np.ones(4), 4, kind='epistatic')
    with pytest.raises(ValueError, match="method: 'gcta', 'vanraden' or 'alpha'"):
        Q.grm_values(np.ones(4), 4, method='yang')
    with pytest.raises(ValueError, match='min_maf'):
        Q.grm_values(np.ones(4), 4, min_maf=0.5)
    with pytest.raises(ValueError, match='alpha'):
        Q.grm_values(np.ones(4), 4, method='alpha', alpha=np.nan)
    with pytest.raises(ValueError, match='counts outside'):
        Q.grm_values(np.array([9]), 4)
    with pytest.raises(ValueError, match='of one n'):
        Q.reml(s['evals'], s['U'], np.ones(N - 1), np.ones((N, 1)))
    with pytest.raises(ValueError, match='evals'):
        Q.reml(s['evals'], s['U'], np.arange(N - 1.0), None)
    with pytest.raises(ValueError, match='full rank'):
        Q.reml(s['evals'], s['U'], s['e'], np.ones((N, 2)))
    with pytest.raises(ValueError, match='evals'):
        Q.reml(s['evals'][:-1], s['U'], s['e'])


# ------------------------------------------------------------------ the Species' calls
class _NumpyDevice:
    """the calls of the handle that the analyses make, in numpy"""

    def __init__(self, D):
        self.D = np.asarray(D, dtype=np.int64)
        self.L = self.D.shape[1]
        self.W64 = (self.L + 63) // 64
        self.cfg = types.SimpleNamespace(n_layers=2, device=0)
        self.calls = 0

    def stats_group_counts(self, slots, group_start):
        assert list(group_start) == [0, len(slots)]
        d = self.D[slots]
        return d.sum(0)[None].astype(np.int32), (d == 1).sum(0)[None].astype(np.int32)

    def grm(self, val, slots, mask):
        assert val.dtype == np.float32 and val.shape == (self.L, 3)
        bits = np.unpackbits(mask.view(np.uint8), bitorder='little')[:self.L].astype(bool)
        Z = QT.expand(val.astype(np.float64), self.D[slots])[:, bits]
        self.calls += 1
        return Z @ Z.T

    def grm_info(self):
        return dict(tiles=1, k_chunks=1, kernel_ms=0.25)


class _Over(SpeciesAnalyses):
    """a Species stand-in: the real analysis methods over the numpy device"""

    def __init__(self, D, ids, z, e):
        self._dev = _NumpyDevice(D)
        self.ids, self.z, self.e = np.asarray(ids), z, e
        trt = types.SimpleNamespace(lyr_num=1, loci=np.array([2, 5]), name='trait_0')
        self.gen_arch = types.SimpleNamespace(traits={0: trt})
        self._genomes_assigned = True

    def __len__(self):
        return self.ids.size

    def _field(self, f):
        return {nat.F_ID: self.ids, nat.F_Z: self.z[None], nat.F_E: self.e.T}[f]


@pytest.fixture(scope='module')
def species():
    rng = np.random.RandomState(21)
    n, L_ = 120, 700
    p = rng.uniform(0.02, 0.98, L_)
    D = (rng.rand(n, L_, 2) < p[None, :, None]).sum(2)
    ids = rng.permutation(n) * 2 + 5
    z = (D[:, :40] @ rng.standard_normal(40)) * 0.1 + 0.5
    e = rng.rand(n, 2)
    return _Over(D, ids, z, e), D, ids, z, e


def test_species_calls_over_a_numpy_device(species):
    spp, D, ids, z, e = species
    order = np.argsort(ids)
    res = spp._calc_grm()
    G, used, Z = QT.grm_from_dosages(D[order])
    np.testing.assert_array_equal(res['ids'], ids[order])
    np.testing.assert_array_equal(res['loci_used'], np.flatnonzero(used))
    assert res['n_loci'] == used.sum() and res['kernel_ms'] == 0.25
    np.testing.assert_array_equal(res['p'], D.sum(0)[used] / (2.0 * len(ids)))
    np.testing.assert_allclose(res['G'], G, rtol=0, atol=1e-12)
    assert abs(np.diag(res['G']).mean() - 1) < 0.1
    # a subset of individuals and loci, dominance, weights
    sub, loci = ids[:50], np.arange(100, 600)
    w = np.random.RandomState(1).rand(700) + 0.5
    res2 = spp._calc_grm(individs=sub, loci=loci, kind='dominance', weights=w)
    o2 = np.argsort(sub)
    Ds = D[:50][o2]
    val, u2 = QT.table_direct(np.where(np.isin(np.arange(700), loci), Ds.sum(0), 0), 50, 'dominance')
    val = (val * w[:, None]).astype(np.float32).astype(np.float64)
    Z2 = QT.expand(val, Ds)
    np.testing.assert_allclose(res2['G'], Z2 @ Z2.T, rtol=0, atol=1e-12)
    assert res2['loci_used'].min() >= 100 and res2['loci_used'].max() < 600
    # heritability of the Trait's z, of a given y with covariates, and with a shared matrix
    X1 = np.ones((len(ids), 1))
    h = spp._calc_heritability(0)
    ref = QT.reml_brute(G, z[order], X1)
    assert abs(h['h2'] - ref['h2']) <= 1e-6 and h['n_loci'] == used.sum()
    assert h['he_h2'] == pytest.approx(QT.he_dense(G, z[order], X1), rel=1e-8)
    np.testing.assert_array_equal(h['ids'], ids[order])
    rng = np.random.RandomState(3)
    y = z[order] + 0.3 * rng.standard_normal(len(ids)) + 2.0 * e[order, 1]
    calls = spp._dev.calls
    shared = spp._calc_grm()
    h1 = spp._calc_heritability(y=y, covars=[('env', 0), 'env'], grm=shared)
    h2 = spp._calc_heritability(y=y + 1, covars=[('env', 0), 'env'], grm=shared)
    assert spp._dev.calls == calls + 1 and 'eig' in shared
    fresh = spp._calc_heritability(y=y, covars=[('env', 0), 'env'])
    X = np.column_stack([np.ones(len(ids)), e[order, 0], e[order, 1]])
    refy = QT.reml_brute(G, y, X)
    for k in ('h2', 'se_h2', 'Vg', 'Ve', 'logL', 'he_h2'):
        assert h1[k] == fresh[k] or (np.isnan(h1[k]) and np.isnan(fresh[k])), k
        assert h2[k] == pytest.approx(h1[k], rel=1e-6, nan_ok=True), k    # a shift is absorbed
    assert abs(h1['h2'] - refy['h2']) <= 1e-6
    # breeding values: everybody trained, then two thirds
    pb = spp._predict_breeding_values(0)
    ref_g, _ = QT.blup_dense(G, z[order], X1, pb['delta'])
    assert np.abs(pb['g_hat'] - ref_g).max() <= 1e-8 * np.abs(ref_g).max()
    assert np.isnan(pb['accuracy']) and pb['h2'] == h['h2']
    np.testing.assert_array_equal(pb['train'], ids[order])
    train = np.sort(ids)[::3]
    train = np.setdiff1d(np.sort(ids), train)
    pt = spp._predict_breeding_values(0, train=train[::-1], grm=shared)
    tix = np.searchsorted(ids[order], train)
    ref_t, _ = QT.blup_dense(G, z[order], X1, pt['delta'], tix)
    assert np.abs(pt['g_hat'] - ref_t).max() <= 1e-8 * np.abs(ref_t).max()
    rest = np.setdiff1d(np.arange(len(ids)), tix)
    assert pt['accuracy'] == pytest.approx(np.corrcoef(pt['g_hat'][rest], z[order][rest])[0, 1])
    np.testing.assert_array_equal(pt['train'], train)
    yn = y.copy()
    yn[rest] = np.nan
    py = spp._predict_breeding_values(y=yn, train=train, grm=shared)
    assert 'accuracy' not in py and np.isfinite(py['g_hat']).all()


def _refusal(f, *a, **kw):
    with pytest.raises(ValueError) as err:
        f(*a, **kw)
    return str(err.value)


def test_request_checks(species):
    spp, D, ids, z, e = species
    n = len(ids)
    assert "kind: 'additive' or 'dominance'" in _refusal(spp._calc_grm, kind='both')
    assert "method: 'gcta', 'vanraden' or 'alpha'" in _refusal(spp._calc_grm, method='ldak')
    assert 'calc_heritability: method' in _refusal(spp._calc_heritability, method='x')
    assert 'min_maf' in _refusal(spp._calc_grm, min_maf=0.7)
    assert 'weights: finite values [L = 700]' in _refusal(spp._calc_grm, weights=np.ones(3))
    assert 'no locus of the request' in _refusal(spp._calc_grm, min_maf=0.499, loci=[0, 1])
    assert 'y: finite values [n = %d]' % n in _refusal(spp._calc_heritability, y=np.ones(n - 1))
    assert 'y: finite values' in _refusal(spp._calc_heritability, y=np.full(n, np.nan))
    assert 'y: finite values' in _refusal(spp._predict_breeding_values, y=np.ones((n, 2)))
    assert 'no Trait 3' in _refusal(spp._calc_heritability, 3)
    assert 'n_pcs' in _refusal(spp._calc_heritability, n_pcs=-1)
    assert 'covars' in _refusal(spp._calc_heritability, covars='depth')
    assert 'not alive' in _refusal(spp._calc_grm, individs=[4])
    assert 'train: at least 2' in _refusal(spp._predict_breeding_values, train=[ids[0]])
    assert 'train: individuals outside the sample' in _refusal(
        spp._predict_breeding_values, train=[ids[0], ids[1]], individs=ids[2:40])
    # a matrix of other individuals
    other = spp._calc_grm(individs=ids[:60])
    assert 'grm: its ids are not the individuals' in _refusal(
        spp._calc_heritability, individs=ids[:61], grm=other)
    assert 'grm: the dict calc_grm returns' in _refusal(spp._calc_heritability, grm=other['G'])
    assert spp._calc_heritability(grm=other)['ids'].size == 60      # its own individuals
    # more than 8192 individuals: before the device is asked
    big = _Over(D, ids, z, e)
    big._geno_sample = lambda individs: (np.arange(8193), np.arange(8193))
    big._dev = types.SimpleNamespace(L=700, W64=11)
    for f in (big._calc_grm, big._calc_heritability, big._predict_breeding_values):
        msg = _refusal(f)
        assert 'at most 8192 individuals' in msg and 'n=...' in msg and 'got 8193' in msg
    # no genomes
    none = _Over(D, ids, z, e)
    none._dev = types.SimpleNamespace(L=0)
    for f in (none._calc_grm, none._calc_heritability, none._predict_breeding_values):
        assert 'the Species has no genomes' in _refusal(f)


def test_the_model_calls_take_a_sample_and_the_tiled_species_refuses():
    from geonomics_amd.sim.model import Model
    from geonomics_amd.structs.tiled import TiledSpecies
    for name, spp_name in (('calc_grm', '_calc_grm'), ('calc_heritability', '_calc_heritability'),
                           ('predict_breeding_values', '_predict_breeding_values')):
        sig = inspect.signature(getattr(Model, name))
        spp_sig = inspect.signature(getattr(SpeciesAnalyses, spp_name))
        assert {'spp', 'individs', 'n', 'loci', 'method', 'alpha', 'min_maf'} <= set(sig.parameters)
        for k in ('method', 'alpha', 'min_maf', 'kind', 'weights', 'grm', 'covars', 'n_pcs'):
            if k in spp_sig.parameters:
                assert sig.parameters[k].default == spp_sig.parameters[k].default, (name, k)
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            getattr(TiledSpecies, spp_name)(object())
    assert 'no environmental deviation' in Model.calc_heritability.__doc__
    sig = inspect.signature(Model.calc_grm)
    assert (sig.parameters['kind'].default, sig.parameters['method'].default,
            sig.parameters['alpha'].default, sig.parameters['min_maf'].default) == \
        ('additive', 'gcta', -1.0, 0.01)
