"""Model.run_mmrr / run_mantel's host side (geonomics_amd/sim/mmrr.py, Species._run_mmrr /
_run_mantel, the Model calls) on the CPU, with numpy cross-sums in place of the device's.

The statistics from cross-sums and moments against the reference's own MMRR(Y, [env, geo],
nperm=199) as recorded in tests/golden/g20_mmrr.npz (case A: a structured sample, n = 131;
case B: the null sample of g18, n = 400) with its recorded permutations: coefficients, t, F and
R^2 within 1e-9 of the largest |entry| of their group (the bar of test_gea_host.py), p-values
exactly.  The p-values are counts of comparisons `permuted >= observed`, so they are compared
for equality only after asserting that no permuted statistic lies within 1e-8 (relative) of the
observed one.  Then the same against a per-permutation numpy lstsq on explicitly permuted
matrices, Mantel's r against numpy.corrcoef and the partial r against the correlation of
lstsq residuals, the permutation generator against np.random.seed + shuffle, and the argument
rules of the public calls on a stand-in Species whose cross-sums are numpy's."""
import inspect
import os
import types

import numpy as np
import pytest

from geonomics_amd.sim import mmrr as M
from geonomics_amd.structs.analyses import SpeciesAnalyses

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g20_mmrr.npz')
BAR = 1e-9
GAP = 1e-8
F_X, F_Y, F_E, F_Z = 0, 1, 5, 6


def fixture_case(tag):
    """(dosages, x, y, e, ids, rows, reference outputs as a dict) of case 'a' or 'b'"""
    f = np.load(GOLDEN)
    out = dict(zip(f[tag + '_keys'].tolist(), f[tag + '_out'].tolist()))
    return (f[tag + '_dosages'].astype(np.int64), f[tag + '_x'], f[tag + '_y'], f[tag + '_e'],
            f[tag + '_ids'], f[tag + '_rows'].astype(np.int64), out)


def fixture_matrices(D, x, y, e):
    return M.genetic_distances(D), [M.euclid(e[:, 1]), M.euclid(np.column_stack([x, y]))]


GROUPS = (('coefficients', ['Intercept', 'env', 'geo']),
          ('t', ['Intercept(t)', 'env(t)', 'geo(t)']), ('F', ['F-statistic']), ('R^2', ['R^2']))
P_KEYS = ['Intercept(p)', 'env(p)', 'geo(p)', 'F p-value']


def smallest_gap(sums, mom):
    """the smallest relative distance of a permuted |t| or F from the observed one"""
    obs = M.ols_from_sums(np.asarray(mom['sxy']), mom)
    per = M.ols_from_sums(sums, mom)
    gt = (np.abs(np.abs(per['t']) - np.abs(obs['t'])) / np.abs(obs['t'])).min()
    gf = (np.abs(per['F'] - obs['F']) / np.abs(obs['F'])).min()
    return min(gt, gf)


def assert_matches_reference(got, ref, sums, mom, label):
    """the comparison every test of the fixture makes, here and on the GPU"""
    assert list(got) == list(ref)                           # the reference's keys, in its order
    for name, keys in GROUPS:
        g = np.array([got[k] for k in keys])
        r = np.array([ref[k] for k in keys])
        err = np.abs(g - r).max() / np.abs(r).max()
        print('%s %s: %.3g of the largest entry' % (label, name, err))
        assert err <= BAR, (label, name, err)
    gap = smallest_gap(sums, mom)
    print('%s: smallest relative gap of a permuted statistic from the observed %.3g'
          % (label, gap))
    assert gap > GAP, (label, gap)
    for k in P_KEYS:
        assert got[k] == ref[k], (label, k, got[k], ref[k])


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_host_path_matches_the_reference_fixture(tag):
    """measured on the committed fixture: every group below 1e-11 of its largest entry; the
    smallest gap 0.18 (case A) and 1.8e-6 (case B, at the intercept's t)"""
    D, x, y, e, ids, rows, ref = fixture_case(tag)
    Y, Xs = fixture_matrices(D, x, y, e)
    assert rows.shape == (199, D.shape[0])
    assert (np.sort(rows, axis=1) == np.arange(D.shape[0])).all()
    sums, mom = M.numpy_perm_sums(Y, Xs, rows), M.numpy_moments(Y, Xs)
    got = M.mmrr(sums, mom, ['env', 'geo'])
    assert_matches_reference(got, ref, sums, mom, 'case ' + tag.upper())
    if tag == 'a':
        assert all(ref[k] == 1 / 200 for k in P_KEYS)       # the structure is found
    else:
        assert all(0.5 < ref[k] <= 1 for k in P_KEYS)       # the null sample


def test_fixture_columns_are_what_a_device_holds():
    """x, y and e of the fixture are exact fp32 values: uploading them loses nothing"""
    for tag in 'ab':
        D, x, y, e, ids, rows, ref = fixture_case(tag)
        for col in (x, y, e):
            np.testing.assert_array_equal(col, col.astype(np.float32).astype(np.float64))
        assert D.min() >= 0 and D.max() <= 2 and (np.diff(ids) > 0).all()


def small_sample(n=40, L=30, seed=3):
    rng = np.random.RandomState(seed)
    x, y = rng.rand(n) * 10, rng.rand(n) * 10
    e = np.column_stack([x / 10 + rng.randn(n) * 0.1, rng.rand(n)])
    z = np.column_stack([e[:, 0] + rng.randn(n) * 0.2])
    p = np.clip(0.2 + 0.6 * e[:, :1] * (np.arange(L) < 12) + 0.3 * (np.arange(L) >= 12), 0.05, 0.95)
    D = rng.binomial(2, p)
    return D, x, y, e, z


def lstsq_fit(y, X):
    """textbook OLS of y on [1, X]: coefficients, t, F, R^2"""
    A = np.column_stack([np.ones(y.size), X])
    m, k = A.shape
    beta = np.linalg.lstsq(A, y, rcond=None)[0]
    res = y - A @ beta
    ssr, tss = res @ res, ((y - y.mean()) ** 2).sum()
    s2 = ssr / (m - k)
    t = beta / np.sqrt(s2 * np.diag(np.linalg.inv(A.T @ A)))
    return beta, t, ((tss - ssr) / (k - 1)) / s2, 1 - ssr / tss


def test_every_permutation_matches_a_refit_on_permuted_matrices():
    D, x, y, e, z = small_sample()
    Y = M.genetic_distances(D)
    Xs = [M.euclid(np.column_stack([x, y])), M.euclid(e), M.euclid(z)]
    rows = M.draw_row_shuffles(40, 60, seed=11)
    mom = M.numpy_moments(Y, Xs)
    Xu = np.column_stack([M.unfold_tril(X) for X in Xs])
    fits = [lstsq_fit(M.unfold_tril(Y[r][:, r]), Xu) for r in [np.arange(40)] + list(rows)]
    S_all = np.vstack([mom['sxy'], M.numpy_perm_sums(Y, Xs, rows)])
    got = M.ols_from_sums(S_all, mom)
    for i, key in enumerate(('coef', 't', 'F', 'r2')):
        ref = np.array([f[i] for f in fits])
        err = np.abs(got[key] - ref).max() / np.abs(ref).max()
        print('%s: %.3g of the largest entry' % (key, err))
        assert err <= BAR, (key, err)
    res = M.mmrr(S_all[1:], mom, ['geo', 'env', 'phn'])
    assert smallest_gap(S_all[1:], mom) > GAP
    t = np.array([f[1] for f in fits])
    F = np.array([f[2] for f in fits])
    tp = (1 + (np.abs(t[1:]) >= np.abs(t[0])).sum(axis=0)) / 61
    for k, name in enumerate(['Intercept', 'geo', 'env', 'phn']):
        assert res[name + '(p)'] == tp[k]
        assert abs(res[name] - fits[0][0][k]) <= BAR * np.abs(fits[0][0]).max()
    assert res['F p-value'] == (1 + (F[1:] >= F[0]).sum()) / 61
    assert list(res) == ['R^2', 'Intercept', 'geo', 'env', 'phn', 'Intercept(t)', 'geo(t)',
                         'env(t)', 'phn(t)', 'Intercept(p)', 'geo(p)', 'env(p)', 'phn(p)',
                         'F-statistic', 'F p-value']
    assert list(M.mmrr(S_all[1:], mom))[2:5] == ['X1', 'X2', 'X3']      # the reference's default


def test_mantel_r_is_pearsons_and_the_partial_r_the_residuals():
    D, x, y, e, z = small_sample(seed=4)
    Y = M.genetic_distances(D)
    Xs = [M.euclid(e), M.euclid(np.column_stack([x, y]))]
    rows = M.draw_row_shuffles(40, 50, seed=2)
    sums, mom = M.numpy_perm_sums(Y, Xs, rows), M.numpy_moments(Y, Xs)
    x1, x2 = (M.unfold_tril(X) for X in Xs)

    def resid(v, g):
        A = np.column_stack([np.ones(g.size), g])
        return v - A @ np.linalg.lstsq(A, v, rcond=None)[0]

    plain = M.mantel(sums, mom, 0)
    part = M.mantel(sums, mom, 0, 1)
    ys = [M.unfold_tril(Y)] + [M.unfold_tril(Y[r][:, r]) for r in rows]
    r_ref = np.array([np.corrcoef(v, x1)[0, 1] for v in ys])
    p_ref = np.array([np.corrcoef(resid(v, x2), resid(x1, x2))[0, 1] for v in ys])
    for got, ref in ((plain, r_ref), (part, p_ref)):
        assert abs(got['r'] - ref[0]) <= 1e-12
        assert np.abs(got['perm_r'] - ref[1:]).max() <= 1e-12
        assert np.abs(ref[1:] - ref[0]).min() > GAP
        assert got['p'] == (1 + (ref[1:] >= ref[0]).sum()) / 51
        assert got['nperm'] == 50 and sorted(got) == ['nperm', 'p', 'perm_r', 'r']
    # the other way round: x given nothing is symmetric in the predictor's index
    assert abs(M.mantel(sums, mom, 1)['r'] - np.corrcoef(ys[0], x2)[0, 1]) <= 1e-12


@pytest.mark.parametrize('seed', [0, 3, 2 ** 31])
def test_the_permutations_replay_the_references_shuffles(seed):
    rows = M.draw_row_shuffles(57, 9, seed=seed)
    np.random.seed(seed)
    rownums = [*range(57)]                                   # MMRR.py shuffles a list
    for p in range(9):
        np.random.shuffle(rownums)
        np.testing.assert_array_equal(rows[p], rownums)
    # a generator handed in is advanced, a seed leaves it alone
    rng = np.random.RandomState(5)
    a = M.draw_row_shuffles(10, 2, rng=rng)
    b = M.draw_row_shuffles(10, 2, rng=rng)
    ref = np.random.RandomState(5)
    for got in (a, b):                                       # each call starts from 0..n-1
        rownums = [*range(10)]
        for p in range(2):
            ref.shuffle(rownums)
            np.testing.assert_array_equal(got[p], rownums)
    assert not np.array_equal(a, b)
    with pytest.raises(ValueError, match='nperm'):
        M.draw_row_shuffles(10, 0)


def test_inverted_rows_are_the_librarys_convention():
    """sum_{i>j} Y[r_i][r_j] X[i][j] = sum_{a>b} Y[a][b] X[q_a][q_b], q = r^-1"""
    D, x, y, e, z = small_sample(n=23)
    Y, X = M.genetic_distances(D), M.euclid(np.column_stack([x, y]))
    rows = M.draw_row_shuffles(23, 5, seed=1)
    perm = M.invert_rows(rows)
    assert perm.dtype == np.int32
    for r, q in zip(rows, perm):
        np.testing.assert_array_equal(q[r], np.arange(23))
        lib = M.unfold_tril(Y) @ M.unfold_tril(X[q][:, q])
        ref = M.numpy_perm_sums(Y, [X], [r])[0, 0]
        assert abs(lib - ref) <= 1e-12 * abs(ref)


def test_degrees_of_freedom():
    D, x, y, e, z = small_sample(n=3)
    Y, Xs = M.genetic_distances(D), [M.euclid(x), M.euclid(y)]
    mom = M.numpy_moments(Y, Xs)                             # 3 pairs, 3 coefficients
    with pytest.raises(ValueError, match='degrees of freedom'):
        M.mmrr(M.numpy_perm_sums(Y, Xs, [np.arange(3)]), mom)


# ------------------------------------------------------------------ the public calls
class _Dev:
    """the device's dist_perm_sums in numpy, on columns kept in slot order"""

    def __init__(self, D, x, y, e, z, L=None):
        self.D, self.x, self.y, self.e, self.z = D, x, y, e, z
        self.L = D.shape[1] if L is None else L
        self.W64 = (self.L + 1023) // 1024 * 16
        self.cfg = types.SimpleNamespace(n_layers=e.shape[1])
        self.calls = []

    def dist_perm_sums(self, predictors, perm, slots=None, locus_mask=None):
        self.calls.append((predictors, perm.copy(), slots, locus_mask))
        slots = np.arange(self.D.shape[0]) if slots is None else slots
        loci = np.arange(self.D.shape[1])
        if locus_mask is not None:
            loci = loci[(locus_mask[loci >> 6] >> (loci & 63).astype(np.uint64)) & np.uint64(1) == 1]
        src = {F_X: lambda i: self.x, F_Y: lambda i: self.y, F_E: lambda i: self.e[:, i],
               F_Z: lambda i: self.z[:, i]}
        Y = M.genetic_distances(self.D[slots][:, loci])
        Xs = [M.euclid(np.column_stack([src[f](i)[slots] for f, i in cols]))
              for cols in predictors]
        sums = np.array([[M.unfold_tril(Y) @ M.unfold_tril(X[q][:, q]) for X in Xs]
                         for q in perm])
        return sums, M.numpy_moments(Y, Xs)


class _Species(SpeciesAnalyses):
    """a Species stand-in: the real _run_mmrr / _run_mantel over numpy cross-sums"""

    def __init__(self, D, x, y, e, z, ids, L=None):
        self._dev = _Dev(D, x, y, e, z, L)
        self.ids = np.asarray(ids)
        trt = types.SimpleNamespace(lyr_num=1, loci=np.array([2, 5]), name='trait_0')
        self.gen_arch = types.SimpleNamespace(traits={0: trt})
        self._genomes_assigned = True
        self._rng = np.random.RandomState(77)
        self.name = 'spp_0'

    def _geno_sample(self, individs):
        order = np.argsort(self.ids)
        if individs is None:
            return self.ids[order], order
        ids = np.sort(np.asarray(individs))
        return ids, order[np.searchsorted(self.ids[order], ids)]

    def __iter__(self):
        return iter(np.sort(self.ids).tolist())

    def _get_individs(self, ids):                  # what _get_adhoc_sample returns the sample as
        return {int(i): None for i in ids}


def _model(spp):
    from geonomics_amd.sim.model import Model
    mod = types.SimpleNamespace(comm={0: spp}, _rng=np.random.RandomState(9))
    for name in ('_get_spp_num', '_test_sample', 'run_mmrr', 'run_mantel'):
        setattr(mod, name, types.MethodType(getattr(Model, name), mod))
    return mod


def _pop(n=60, L=30, seed=8):
    D, x, y, e, z = small_sample(n, L, seed)
    ids = np.random.RandomState(seed).permutation(n) * 3 + 1       # slot order is not id order
    return _Species(D, x, y, e, z, ids), D, x, y, e, z, ids


def test_run_mmrr_is_the_host_path_on_the_sample_in_id_order():
    spp, D, x, y, e, z, ids = _pop()
    mod = _model(spp)
    res = mod.run_mmrr(seed=3, nperm=99)
    o = np.argsort(ids)
    Y = M.genetic_distances(D[o])
    Xs = [M.euclid(np.column_stack([x, y])[o]), M.euclid(e[o, 1])]   # 'env': the Trait's layer
    rows = M.draw_row_shuffles(60, 99, seed=3)
    ref = M.mmrr(M.numpy_perm_sums(Y, Xs, rows), M.numpy_moments(Y, Xs), ['geo', 'env'])
    assert list(res) == list(ref)
    for k in ref:
        assert abs(res[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), k
    cols, perm, slots, mask = spp._dev.calls[-1]
    assert cols == [[(F_X, 0), (F_Y, 0)], [(F_E, 1)]] and mask is None
    np.testing.assert_array_equal(slots, o)
    np.testing.assert_array_equal(perm, M.invert_rows(rows))
    # the selections: individs, loci, layers, traits, and the sample of n
    some = np.sort(ids)[::2][::-1]
    sub = mod.run_mmrr(predictors=('env', 'phn', 'geo'), env_lyrs=[0, 1], trts=0, individs=some,
                       loci=[3, 4, 9, 9, 20], nperm=20, seed=1)
    cols, perm, slots, mask = spp._dev.calls[-1]
    assert cols == [[(F_E, 0), (F_E, 1)], [(F_Z, 0)], [(F_X, 0), (F_Y, 0)]]
    np.testing.assert_array_equal(slots, o[::2])
    assert mask[0] == sum(1 << l for l in (3, 4, 9, 20)) and perm.shape == (20, 30)
    assert [k for k in sub if k.endswith('(p)')] == ['Intercept(p)', 'env(p)', 'phn(p)', 'geo(p)']
    mod.run_mmrr(n=25, nperm=5, seed=1)
    assert spp._dev.calls[-1][1].shape == (5, 25)
    # without a seed the Species' generator supplies the shuffles, and moves on
    a = mod.run_mantel(nperm=9)
    b = mod.run_mantel(nperm=9)
    assert a['r'] == b['r'] and not np.array_equal(a['perm_r'], b['perm_r'])


def test_run_mantel_plain_and_partial():
    spp, D, x, y, e, z, ids = _pop()
    mod = _model(spp)
    o = np.argsort(ids)
    Y = M.genetic_distances(D[o])
    Xs = [M.euclid(e[o, 1]), M.euclid(np.column_stack([x, y])[o])]
    rows = M.draw_row_shuffles(60, 99, seed=3)
    sums, mom = M.numpy_perm_sums(Y, Xs, rows), M.numpy_moments(Y, Xs)
    for given, ref in ((None, M.mantel(sums, mom, 0)), ('geo', M.mantel(sums, mom, 0, 1))):
        got = mod.run_mantel('env', given=given, seed=3, nperm=99)
        assert abs(got['r'] - ref['r']) <= 1e-12 and got['nperm'] == 99
        assert np.abs(got['perm_r'] - ref['perm_r']).max() <= 1e-12
        assert got['p'] == ref['p']


def test_argument_rules():
    spp, D, x, y, e, z, ids = _pop()
    mod = _model(spp)
    for call in (lambda **kw: mod.run_mmrr(**kw), lambda **kw: mod.run_mantel('env', **kw)):
        for bad in (0, -1, 2.5, True):
            with pytest.raises(ValueError, match='nperm'):
                call(nperm=bad)
        with pytest.raises(ValueError, match='not both'):
            call(individs=ids[:20], n=10)
        with pytest.raises(ValueError, match='env_lyrs'):
            call(env_lyrs=[2], nperm=5)
        with pytest.raises(ValueError, match='loci'):
            call(loci=[0, D.shape[1]], nperm=5)
    with pytest.raises(ValueError, match="unknown predictor 'gen'"):
        mod.run_mmrr(predictors=('geo', 'gen'))
    with pytest.raises(ValueError, match='unknown predictor'):
        mod.run_mantel('env', given='elevation')
    with pytest.raises(ValueError, match='listed twice'):
        mod.run_mantel('env', given='env')
    with pytest.raises(ValueError, match='trts'):
        mod.run_mmrr(predictors=('phn',), trts=[1])
    with pytest.raises(ValueError, match='no predictors'):
        mod.run_mmrr(predictors=())
    with pytest.raises(ValueError, match='degrees of freedom'):
        mod.run_mmrr(individs=np.sort(ids)[:3], nperm=5)        # 3 pairs, 3 coefficients
    mod.run_mmrr(individs=np.sort(ids)[:4], nperm=5)            # 6 pairs: enough
    with pytest.raises(ValueError, match='degrees of freedom'):
        mod.run_mantel(individs=np.sort(ids)[:2], nperm=5)
    big = _Species(np.zeros((8193, 4), np.int64), np.zeros(8193), np.zeros(8193),
                   np.zeros((8193, 2)), np.zeros((8193, 1)), np.arange(8193))
    for call in (_model(big).run_mmrr, _model(big).run_mantel):
        with pytest.raises(ValueError, match='at most 8192 individuals.*n='):
            call(nperm=5)
    no_genomes = _Species(D, x, y, e, z, ids)
    no_genomes.gen_arch = None
    with pytest.raises(ValueError, match='no genomes'):
        _model(no_genomes).run_mmrr()
    with pytest.raises(ValueError, match='no genomes'):
        _model(_Species(D, x, y, e, z, ids, L=0)).run_mantel()
    unassigned = _Species(D, x, y, e, z, ids)
    unassigned._genomes_assigned = False
    with pytest.raises(ValueError, match='burn'):
        _model(unassigned).run_mmrr()
    # a Species without Traits: 'env' is every layer, 'phn' has nothing to offer
    no_traits = _Species(D, x, y, e, z, ids)
    no_traits.gen_arch.traits = None
    _model(no_traits).run_mantel('env', nperm=5, seed=1)
    assert no_traits._dev.calls[-1][0] == [[(F_E, 0), (F_E, 1)]]
    with pytest.raises(ValueError, match='trts'):
        _model(no_traits).run_mantel('phn', nperm=5)


def test_the_public_calls_have_the_documented_signatures():
    from geonomics_amd.sim.model import Model
    sig = inspect.signature(Model.run_mmrr)
    assert list(sig.parameters) == ['self', 'spp', 'predictors', 'env_lyrs', 'trts', 'individs',
                                    'n', 'loci', 'nperm', 'seed']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['spp'], d['predictors'], d['nperm']) == (0, ('geo', 'env'), 999)
    assert all(d[k] is None for k in ('env_lyrs', 'trts', 'individs', 'n', 'loci', 'seed'))
    sig = inspect.signature(Model.run_mantel)
    assert list(sig.parameters)[:3] == ['self', 'x', 'given']
    assert set(sig.parameters) == {'self', 'x', 'given', 'spp', 'env_lyrs', 'trts', 'individs',
                                   'n', 'loci', 'nperm', 'seed'}
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['x'], d['given'], d['spp'], d['nperm']) == ('geo', None, 0, 999)


def test_a_tiled_species_refuses():
    from geonomics_amd.structs.tiled import TiledSpecies
    for name in ('_run_mmrr', '_run_mantel'):
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            getattr(TiledSpecies, name)(object())


def test_the_binding_exports_the_cross_sums():
    from geonomics_amd import _native as nat
    assert 'gnx_dist_perm_sums' in nat.EXPORTS
    assert callable(nat.Device.dist_perm_sums)
    assert (nat.F_X, nat.F_Y, nat.F_E, nat.F_Z) == (F_X, F_Y, F_E, F_Z)
