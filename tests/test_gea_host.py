"""Model.run_gea's host side (geonomics_amd/sim/gea.py, Species._run_cca, Model.run_gea) on the
CPU, with numpy cross-products in place of the device's.

The fit from cross-products against the reference's own Species._run_cca (sklearn's
CCA(n_components=3) on the N x L table) as recorded in tests/golden/g18_gea.npz (N = 400,
L = 96, one monomorphic locus, one pair of identical loci), and against a live sklearn CCA
where sklearn imports: each of ind_df, loci_df and var_df within 1e-9 of its largest |entry|
(the bar test_genetic_pca_host.py sets for scores).  Then the warnings and the argument rules
of the public calls, on a stand-in Species whose products are numpy's."""
import inspect
import os
import types
import warnings

import numpy as np
import pytest

from geonomics_amd.sim import gea as G
from geonomics_amd.structs.analyses import SpeciesAnalyses

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g18_gea.npz')
BAR = 1e-9
OUTPUTS = ('ind_df', 'loci_df', 'var_df')


def host_cca(D, Z):
    """the host path with numpy products: D dosages [N][n_loci], Z [N][3]"""
    Df = np.asarray(D, np.float64)
    return G.cca_from_cross_products(*G.numpy_cross_products(D, Z), D.shape[0],
                                     lambda M: Df @ M)


def rel_errors(got, ref):
    return {k: np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max() for k in OUTPUTS}


def synthetic(n, L, seed):
    """dosages with an environmental cline at the first 5 loci, a monomorphic locus and a
    duplicated pair; predictors [env, lat, long]"""
    rng = np.random.RandomState(seed)
    p = rng.uniform(0.1, 0.9, L)
    x, y = rng.rand(n) * 24, rng.rand(n) * 24
    e = x / 24 + rng.randn(n) * 0.05
    f = np.clip(p[None, :] + 0.3 * (e[:, None] - 0.5) * (np.arange(L) < 5), 0.02, 0.98)
    D = (rng.rand(n, L) < f).astype(np.int64) + (rng.rand(n, L) < f)
    D[:, 7] = 0
    D[:, 9] = D[:, 8]
    return D, np.column_stack([e, x, y])


def test_host_path_matches_the_reference_fixture():
    """measured on the committed fixture: ind_df 1.4e-12, loci_df 1.1e-12, var_df 4.7e-12 of
    the largest |entry| (bar 1e-9); 25, 14 and 2 iterations, smallest kept eigenvalue 4.1e-4
    of the largest"""
    f = np.load(GOLDEN)
    D = f['dosages'].astype(np.int64)
    N, L = D.shape
    assert N > L + 3
    assert (D[:, 17] == 0).all() and (D[:, 41] == D[:, 40]).all()
    Z = np.column_stack([f['e'][:, int(f['lyr_num'])], f['x'], f['y']])
    with warnings.catch_warnings():
        warnings.simplefilter('error')                   # neither degenerate nor capped
        got = host_cca(D, Z)
    err = rel_errors(got, f)
    print('fixture: ' + ', '.join('%s %.3g' % kv for kv in err.items()),
          'iterations %s, smallest kept eigenvalue ratio %.3g'
          % (got['n_iter'].tolist(), got['min_kept_ratio']))
    assert got['loci_df'].shape == (L, 3) and got['var_df'].shape == (3, 3)
    for k in OUTPUTS:
        assert err[k] <= BAR, (k, err[k])


@pytest.mark.parametrize('shape', [(400, 60, 1), (1000, 200, 2)], ids=lambda s: '%dx%d' % s[:2])
def test_host_path_matches_live_sklearn(shape):
    cd = pytest.importorskip('sklearn.cross_decomposition')
    n, L, seed = shape
    D, Z = synthetic(n, L, seed)
    cca = cd.CCA(n_components=3)
    X = D / 2.0
    cca.fit(X, Z)
    ref = dict(ind_df=cca.transform(X), loci_df=cca.x_loadings_, var_df=cca.y_loadings_)
    err = rel_errors(host_cca(D, Z), ref)
    print('%s: ' % (shape,) + ', '.join('%s %.3g' % kv for kv in err.items()))
    for k in OUTPUTS:
        assert err[k] <= BAR, (k, err[k])


def test_scaled_cross_products_are_the_blocks_own():
    D, Z = synthetic(300, 40, 3)
    Sxx, Sxy, Syy, xm, xs, ym, ys = G.scaled_cross_products(*G.numpy_cross_products(D, Z), 300)
    X = D / 2.0
    sd = X.std(axis=0, ddof=1)
    sd[sd == 0] = 1.0
    Xs = (X - X.mean(axis=0)) / sd
    Ys = (Z - Z.mean(axis=0)) / Z.std(axis=0, ddof=1)
    np.testing.assert_allclose(Sxx, Xs.T @ Xs, rtol=0, atol=1e-10 * 300)
    np.testing.assert_allclose(Sxy, Xs.T @ Ys, rtol=0, atol=1e-10 * 300)
    np.testing.assert_allclose(Syy, Ys.T @ Ys, rtol=0, atol=1e-10 * 300)
    assert xs[7] == 1.0 and (Sxx[7] == 0).all()          # the monomorphic locus
    np.testing.assert_array_equal(Sxx[8], Sxx[9])        # the twins: bit-equal rows


def test_degenerate_warning_fires_at_n_le_loci_plus_3():
    D, Z = synthetic(150, 300, 4)
    with pytest.warns(G.DegenerateGEAWarning, match='degenerate'):
        got = host_cca(D, Z)
    assert np.isfinite(got['ind_df']).all() and got['loci_df'].shape == (300, 3)
    for n, L, warns in ((63, 60, True), (64, 60, False)):       # the boundary: N = L + 3
        D, Z = synthetic(n, L, 5)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            host_cca(D, Z)
        assert any(issubclass(i.category, G.DegenerateGEAWarning) for i in w) == warns, (n, L)


def test_iteration_cap_warns(monkeypatch):
    D, Z = synthetic(400, 60, 1)
    monkeypatch.setattr(G, 'MAX_ITER', 2)
    with pytest.warns(G.GEAConvergenceWarning, match='iterations'):
        host_cca(D, Z)


def test_cutoff_is_a_named_constant():
    assert G.PINV_CUTOFF == 1e6 * np.finfo(np.float64).eps
    S_, r = G.sym_pinv(np.diag([4.0, 1.0, 1e-12]))
    np.testing.assert_allclose(S_, np.diag([0.25, 1.0, 0.0]), atol=1e-15)
    assert r == 0.25


# ------------------------------------------------------------------ the public calls
class _Dev:
    def __init__(self, L):
        self.L, self.W64 = L, (L + 1023) // 1024 * 16


class _Species(SpeciesAnalyses):
    """a Species stand-in: the real _run_cca / _geno_loci over numpy products"""

    def __init__(self, D, Z2, ids, L=None):
        self.D, self.e, self.ids = D, Z2, np.asarray(ids)
        self._dev = _Dev(D.shape[1] if L is None else L)
        trt = types.SimpleNamespace(lyr_num=1, loci=np.array([2, 5, 11]), name='trait_0')
        self.gen_arch = types.SimpleNamespace(traits={0: trt})
        self._genomes_assigned = True
        self.name = 'spp_0'

    def _geno_sample(self, individs):
        order = np.argsort(self.ids)
        if individs is None:
            return self.ids[order], order
        ids = np.sort(np.asarray(individs))
        return ids, order[np.searchsorted(self.ids[order], ids)]

    def _gea_products(self, slots, loci, lyr_num):
        D = self.D[slots][:, loci]
        Z = self.e[slots][:, [lyr_num, 2, 3]]
        Df = D.astype(np.float64)
        return G.numpy_cross_products(D, Z) + (lambda M: Df @ M,)


def _model(spp):
    from geonomics_amd.sim.model import Model
    mod = types.SimpleNamespace(comm={0: spp})
    for name in ('_get_spp_num', '_get_trt_num', 'run_gea'):
        setattr(mod, name, types.MethodType(getattr(Model, name), mod))
    return mod


def _pop(n=300, L=40, seed=6):
    D, Z = synthetic(n, L, seed)
    rng = np.random.RandomState(seed)
    ids = rng.permutation(n) * 3 + 1                       # slot order is not id order
    cols = np.column_stack([np.ones(n), Z])                # e layers 0 and 1, then x, y
    return _Species(D, cols, ids), D, Z, ids


def test_run_gea_returns_the_reference_keys_and_warns_that_it_does_not_plot():
    spp, D, Z, ids = _pop()
    mod = _model(spp)
    with pytest.warns(UserWarning, match='does not plot'):
        res = mod.run_gea()                                 # the default call: plot=True
    assert sorted(res) == ['ids', 'ind_df', 'loci_df', 'trait_loci', 'var_df']
    order = np.argsort(ids)
    np.testing.assert_array_equal(res['ids'], ids[order])
    np.testing.assert_array_equal(res['trait_loci'], [2, 5, 11])
    ref = host_cca(D[order], Z[order])
    for k in OUTPUTS:
        assert np.abs(res[k] - ref[k]).max() <= BAR * np.abs(ref[k]).max(), k
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        quiet = mod.run_gea(plot=False, scale=7, sd=1, plot_sd=False)
    for k in OUTPUTS:
        np.testing.assert_array_equal(quiet[k], res[k])


def test_run_gea_individs_and_loci_restrict_rows_and_columns():
    spp, D, Z, ids = _pop()
    mod = _model(spp)
    some = np.sort(ids)[::2][::-1]
    loci = [30, 3, 4, 5, 20, 21, 3]
    res = mod.run_gea(plot=False, individs=some, loci=loci)
    np.testing.assert_array_equal(res['ids'], np.sort(some))
    rows = np.argsort(ids)[::2]
    ref = host_cca(D[rows][:, np.unique(loci)], Z[rows])
    assert res['loci_df'].shape == (6, 3) and res['ind_df'].shape == (some.size, 3)
    for k in OUTPUTS:
        assert np.abs(res[k] - ref[k]).max() <= BAR * np.abs(ref[k]).max(), k


def test_argument_rules():
    spp, D, Z, ids = _pop()
    mod = _model(spp)
    for bad in ('rda', 'lfmm', '', None, 3):
        with pytest.raises(ValueError, match='Valid methods include: cca'):
            mod.run_gea(method=bad, plot=False)
    mod.run_gea(method='CCA', plot=False)                   # the reference lower-cases it
    for bad in (1, -1, 7, True):
        with pytest.raises(ValueError, match='no Trait'):
            mod.run_gea(trt=bad, plot=False)
    with pytest.raises(ValueError, match='at most 8192 loci.*loci='):
        _model(_Species(D, spp.e, ids, L=8193)).run_gea(plot=False)
    with pytest.raises(ValueError, match='at most 8192 loci'):
        _model(_Species(D, spp.e, ids, L=20000)).run_gea(plot=False, loci=np.arange(8193))
    with pytest.raises(ValueError, match='loci'):
        mod.run_gea(plot=False, loci=[0, D.shape[1]])
    no_genomes = _Species(D, spp.e, ids)
    no_genomes.gen_arch = None
    with pytest.raises(ValueError, match='no genomes'):
        _model(no_genomes).run_gea(plot=False)
    no_genomes = _Species(D, spp.e, ids, L=0)
    with pytest.raises(ValueError, match='no genomes'):
        _model(no_genomes).run_gea(plot=False)
    unassigned = _Species(D, spp.e, ids)
    unassigned._genomes_assigned = False
    with pytest.raises(ValueError, match='burn'):
        _model(unassigned).run_gea(plot=False)
    no_traits = _Species(D, spp.e, ids)
    no_traits.gen_arch.traits = None
    with pytest.raises(ValueError, match='no Traits'):
        _model(no_traits).run_gea(plot=False)


def test_run_gea_has_the_reference_signature():
    from geonomics_amd.sim.model import Model
    sig = inspect.signature(Model.run_gea)
    assert list(sig.parameters) == ['self', 'method', 'spp', 'trt', 'plot', 'plot_sd', 'scale',
                                    'sd', 'individs', 'loci', 'gea_df']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['method'], d['spp'], d['trt'], d['plot'], d['plot_sd'], d['scale'], d['sd']) == \
        ('cca', 0, 0, True, True, 3, 3)
    assert d['individs'] is None and d['loci'] is None and d['gea_df'] is False
    assert 'N x L' in Model.run_gea.__doc__                 # the one download is documented


def test_a_tiled_species_refuses():
    from geonomics_amd.structs.tiled import TiledSpecies
    with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
        TiledSpecies._run_cca(object())


def test_the_binding_exports_the_cross_products():
    from geonomics_amd import _native as nat
    assert 'gnx_geno_locus_gram' in nat.EXPORTS and 'gnx_geno_locus_cross' in nat.EXPORTS
    assert callable(nat.Device.geno_locus_gram) and callable(nat.Device.geno_locus_cross)
