"""Model.run_mmrr / run_mantel on the device (csrc/gnx_mantel.hip, sim/mmrr.py,
Species._run_mmrr / _run_mantel): gnx_dist_perm_sums against numpy fp64 on the downloaded
genomes and columns, and the whole tests against the reference's recorded MMRR outputs
(tests/golden/g20_mmrr.npz) and against the host path (tests/test_mmrr_host.py, which ties that
path to the reference and to per-permutation lstsq fits).  Needs an MI355X.

Bounds.  A cross-sum is S = sum over the m = n (n - 1) / 2 pairs of y x, every term >= 0.
y = 0.5 sqrt(integer) is correctly rounded on both sides (IEEE sqrt of the same exact integer,
an exact halving): no discrepancy.  x = sqrt(sum of D squared differences): a difference of
fp32 columns is exact in fp64 or rounded once (its square carries that twice, and its own
rounding: 3), the D - 1 additions (D - 1), and sqrt halves that and rounds once: each side
within (D + 2) / 2 + 1 roundings of the exact value, the two sides within D + 4 of each other;
the product y x rounds once on each side (2).  Terms therefore differ by at most
(D + 6) 2^-53 relatively - 8 for the predictors of up to 2 columns compared here (the library
is built without FMA contraction; a contracted product would round once less) - and two sums
of m such terms in any order by m 2^-53 sum|y||x| more, the any-order bound test_gpu_gea.py
uses:

    |S - S_ref| <= (m + 8) 2^-53 sum |y| |x|

The same bound holds for the moments sum y, sum y^2, sum x_k and sum y x_k; the terms x_k x_l of
sum x_k x_l carry both predictors' roundings, 2 (D + 4) + 2 = 14: (m + 16).  Measured on an
MI355X: the worst error is 1.2e-2 of its bound (n = 65), 2.7e-5 of it at n = 1031.  The
statistics of the end-to-end tests must meet 1e-9 of the largest |entry| of their group
(coefficients, t, F, R^2), the host test's bar (measured: below 3e-12).  p-values are counts of comparisons `permuted >= observed`; they are compared for
equality only because no permuted statistic of the host restatement lies within the propagated
bound of the observed one: every such test computes the smallest relative gap on the host and
asserts that it exceeds 1e-8 first (measured: 0.18 on case A, 1.8e-6 on case B)."""
import numpy as np
import pytest

from test_gpu_parity import native
from test_mmrr_host import (BAR, GAP, assert_matches_reference, fixture_case, fixture_matrices,
                            smallest_gap)
from geonomics_amd.sim import mmrr as M

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
GEO = [(0, 0), (1, 0)]                  # (GNX_F_X, 0), (GNX_F_Y, 0)
ENV1 = [(5, 1)]                         # layer 1 of GNX_F_E
ENV01 = [(5, 0), (5, 1)]
ENV12 = [(5, 1), (5, 2)]
PHN = [(6, 0), (6, 1)]                  # both traits of GNX_F_Z


def _handle(nat, D, x, y, ids, rasts, traits=(), seed=20):
    """a population with dosages D [n][L] at (x, y) on a handle over the given rasters"""
    import gnx_oracle as O
    n, L = D.shape
    H, W = rasts.shape[1:]
    dev = nat.Device(W, H, rasts.shape[0], L=L, n_traits=len(traits), cap_inds=n + 64,
                     cap_rows=n + 64, seed=seed)
    dev.upload_rasters(rasts.astype(np.float32))
    dev.set_species_params(nat.default_species_params())
    for t, (loci, alpha, layer) in enumerate(traits):
        dev.set_trait(t, loci, alpha, layer, 0.3, 1.0, False)
    dev.upload_population(x.astype(np.float32), y.astype(np.float32), np.zeros(n), np.zeros(n),
                          ids)
    dev.upload_genomes(O.pack_genomes(np.stack([D >= 1, D == 2], axis=2).astype(np.uint8)))
    if traits:
        dev.set_z()
    return dev


def _g18_rasters():
    return np.stack([np.ones((24, 24)), np.tile(np.linspace(0, 1, 24), (24, 1))])


@pytest.fixture(scope='module')
def cases():
    """cases A (n = 131) and B (n = 400, the population of g18) of g20_mmrr.npz, each on a
    handle over g18's 24 x 24 landscape, with the fixture's matrices"""
    nat = native()
    out = {}
    for tag in 'ab':
        D, x, y, e, ids, rows, ref = fixture_case(tag)
        dev = _handle(nat, D, x, y, ids, _g18_rasters())
        out[tag] = (dev, D, x, y, e, rows, ref)
    yield nat, out
    for v in out.values():
        v[0].close()


@pytest.fixture(scope='module')
def big():
    """a random population, n = 1031 (17 tiles of 64: 153 tiles in more units than one, the
    last tile 7 rows), L = 200, three random layers and two traits"""
    nat = native()
    rng = np.random.RandomState(31)
    n, L = 1031, 200
    D = rng.binomial(2, rng.uniform(0.1, 0.9, L), size=(n, L))
    rasts = np.stack([np.ones((20, 28)), rng.rand(20, 28), rng.rand(20, 28)])
    traits = [(np.array([3, 70, 150]), np.array([0.2, -0.1, 0.15]), 1),
              (np.array([9, 64, 199]), np.array([0.1, 0.1, -0.2]), 2)]
    dev = _handle(nat, D, rng.uniform(0, 28, n), rng.uniform(0, 20, n), np.arange(n), rasts,
                  traits)
    yield nat, dev, D
    dev.close()


def _columns(dev, nat, slots=None):
    """the columns (field, index) -> float64 [n] as the device holds them, in slot order"""
    e, z = dev.download(nat.F_E), dev.download(nat.F_Z) if dev.n_traits else None
    s = slice(None) if slots is None else slots

    def col(f, i):
        a = {nat.F_X: lambda: dev.download(nat.F_X), nat.F_Y: lambda: dev.download(nat.F_Y),
             nat.F_E: lambda: e[i], nat.F_Z: lambda: z[i]}[f]()
        return a.astype(np.float64)[s]
    return col


def _reference(D, col, predictors, perm):
    """Y, Xs and the cross-sums [n_perm][K] in numpy: sum_{a>b} Y[a][b] X_k[perm a][perm b]"""
    Y = M.genetic_distances(D)
    Xs = [M.euclid(np.column_stack([col(f, i) for f, i in p])) for p in predictors]
    y = M.unfold_tril(Y)
    S = np.array([[y @ M.unfold_tril(X[q][:, q]) for X in Xs] for q in perm])
    return Y, Xs, S


def _perms(n, n_perm, seed):
    rng = np.random.RandomState(seed)
    return np.stack([np.arange(n)] + [rng.permutation(n) for _ in range(n_perm - 1)]) \
        .astype(np.int32)


def _check(dev, nat, D, predictors, perm, slots=None, mask=None, loci=None, label=''):
    """one call against numpy within the bounds of the module's docstring, twice bit-equal,
    and permutation 0 (the identity) against the moments' sum y x_k"""
    Dn = D if slots is None else D[slots]
    Dn = Dn if loci is None else Dn[:, loci]
    n = Dn.shape[0]
    m = n * (n - 1) // 2
    sums, mom = dev.dist_perm_sums(predictors, perm, slots, mask)
    Y, Xs, S_ref = _reference(Dn, _columns(dev, nat, slots), predictors, perm)
    ref = M.numpy_moments(Y, Xs)
    assert sums.shape == S_ref.shape == (perm.shape[0], len(predictors))
    worst = 0.0

    def within(got, want, absum, c, what):
        nonlocal worst
        err, bound = np.abs(got - want), (m + c) * U53 * absum
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (label, what, err.max(), np.min(bound))

    within(sums, S_ref, S_ref, 8, 'sums')
    assert mom['m'] == m
    for k in ('sy', 'syy', 'sx', 'sxy'):
        within(np.asarray(mom[k]), np.asarray(ref[k]), np.asarray(ref[k]), 8, k)
    within(mom['sxx'], ref['sxx'], ref['sxx'], 16, 'sxx')
    assert (perm[0] == np.arange(n)).all()
    within(sums[0], mom['sxy'], ref['sxy'], 8, 'identity')
    print('%s: n = %d, %d permutations, %d predictors: worst error / bound %.3g'
          % (label, n, perm.shape[0], len(predictors), worst))
    sums2, mom2 = dev.dist_perm_sums(predictors, perm, slots, mask)      # fixed order
    np.testing.assert_array_equal(sums2, sums)
    for k in mom:
        np.testing.assert_array_equal(mom2[k], mom[k])
    return sums, mom


@pytest.mark.parametrize('n', [2, 3, 63, 64, 65, 131, 400])
def test_sums_and_moments_at_every_tile_edge(cases, n):
    nat, c = cases
    dev, D = c['b'][:2]
    slots = None if n == 400 else \
        np.random.RandomState(n).choice(400, n, replace=False).astype(np.int64)
    _check(dev, nat, D, [ENV1, GEO], _perms(n, 65, n), slots, label='n')


@pytest.mark.parametrize('n_perm', [1, 63, 64, 65, 199])
def test_sums_at_every_block_edge_of_permutations(cases, n_perm):
    nat, c = cases
    dev, D = c['a'][:2]
    _check(dev, nat, D, [GEO, ENV1], _perms(131, n_perm, n_perm), label='n_perm')


def test_several_units_and_a_short_last_tile(big):
    nat, dev, D = big
    _check(dev, nat, D, [GEO, ENV12], _perms(1031, 65, 1), label='n = 1031')


@pytest.mark.parametrize('predictors', [[ENV12], [PHN, GEO], [GEO, ENV12, PHN],
                                        [ENV1, GEO, [(5, 2)], [(6, 1)]]],
                         ids=['1', '2', '3', '4'])
def test_one_to_four_predictors_with_two_layer_env_and_phn(big, predictors):
    nat, dev, D = big
    slots = np.random.RandomState(4).choice(1031, 150, replace=False).astype(np.int64)
    z = dev.download(nat.F_Z)
    assert z.shape == (2, 1031) and np.ptp(z[0]) > 0 and np.ptp(z[1]) > 0
    _check(dev, nat, D, predictors, _perms(150, 70, 2), slots, label='predictors')


def test_a_locus_mask_and_slots_in_descending_order(cases):
    nat, c = cases
    dev, D = c['b'][:2]
    loci = np.sort(np.random.RandomState(2).choice(96, 30, replace=False))
    loci[-1] = 95
    mask = np.zeros(dev.W64, np.uint64)
    np.bitwise_or.at(mask, loci >> 6, np.uint64(1) << (loci & 63).astype(np.uint64))
    down = np.arange(399, 199, -1).astype(np.int64)
    a, _ = _check(dev, nat, D, [ENV01, GEO], _perms(200, 20, 3), down, mask, loci, 'mask, down')
    # all-ones layer 0 adds nothing to the env distance
    b, _ = dev.dist_perm_sums([ENV1, GEO], _perms(200, 20, 3), down, mask)
    np.testing.assert_array_equal(a, b)


def test_refusals_leave_the_handle_as_it_was(cases):
    nat, c = cases
    dev, D = c['a'][:2]
    perm = _perms(131, 5, 9)
    before = dev.dist_perm_sums([GEO, ENV1], perm)
    ok = np.arange(131, dtype=np.int32)[None, :]
    with pytest.raises(nat.GnxError, match='8192'):
        dev.dist_perm_sums([GEO], np.zeros((1, 0), np.int32), np.zeros(0, np.int64))
    with pytest.raises(nat.GnxError, match='8192'):
        dev.dist_perm_sums([GEO], np.zeros((1, 8193), np.int32), np.arange(8193) % 131)
    for bad in (131, -1, 2 ** 31 - 1):
        p = perm.copy()
        p[3, 77] = bad
        with pytest.raises(nat.GnxError, match=r'perm\[3\]\[77\]'):
            dev.dist_perm_sums([GEO], p)
    for cols in ([(5, 2)], [(5, -1)], [(6, 0)], [(0, 1)], [(4, 0)]):     # layer, trait, field
        with pytest.raises(nat.GnxError, match='GNX_F_E'):
            dev.dist_perm_sums([GEO, cols], ok)
    with pytest.raises(nat.GnxError, match='predictors'):
        dev.dist_perm_sums([], ok)
    with pytest.raises(nat.GnxError, match='predictors'):
        dev.dist_perm_sums([GEO] * 5, ok)
    with pytest.raises(nat.GnxError, match='column|predictors'):
        dev.dist_perm_sums([[]], ok)
    with pytest.raises(nat.GnxError, match='column'):
        dev.dist_perm_sums([ENV01 * 2, ENV01 * 2, [(0, 0)]], ok)         # 9 columns
    with pytest.raises(nat.GnxError, match='permutations'):
        dev.dist_perm_sums([GEO], np.zeros((0, 131), np.int32))
    with pytest.raises(nat.GnxError, match='slot out of range'):
        dev.dist_perm_sums([GEO], np.zeros((1, 2), np.int32), np.array([0, dev.N]))
    with pytest.raises(ValueError, match='perm'):
        dev.dist_perm_sums([GEO], np.zeros((1, 130), np.int32))
    after = dev.dist_perm_sums([GEO, ENV1], perm)
    np.testing.assert_array_equal(after[0], before[0])
    for k in before[1]:
        np.testing.assert_array_equal(after[1][k], before[1][k])
    # a handle without genomes, and one holding ghost records
    empty = nat.Device(16, 16, 1, L=96, cap_inds=256, cap_rows=256, seed=1)
    empty.upload_rasters(np.ones((1, 16, 16), np.float32))
    empty.set_species_params(nat.default_species_params())
    empty.upload_population(np.ones(10), np.ones(10), np.zeros(10), np.zeros(10), np.arange(10))
    with pytest.raises(nat.GnxError, match='genomes not assigned'):
        empty.dist_perm_sums([GEO], np.arange(10, dtype=np.int32)[None, :])
    empty.close()
    tile = _handle(nat, D[:10], np.ones(10), np.ones(10), np.arange(10), _g18_rasters())
    rec = np.zeros(1, nat.IND_REC)
    rec['x'], rec['y'], rec['id'] = 1.0, 1.0, 10 ** 6
    tile.tile_import_ghosts(rec)
    with pytest.raises(nat.GnxError, match='ghost records'):
        tile.dist_perm_sums([GEO], np.arange(10, dtype=np.int32)[None, :],
                            np.arange(10, dtype=np.int64))
    tile.close()


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_the_references_mmrr_from_device_sums(cases, tag):
    """gnx_dist_perm_sums with the fixture's recorded permutations, through sim/mmrr.py: the
    reference's recorded MMRR(Y, [env, geo], nperm=199)"""
    nat, c = cases
    dev, D, x, y, e, rows, ref = c[tag]
    col = _columns(dev, nat)
    np.testing.assert_array_equal(col(nat.F_X, 0), x)       # the handle holds the fixture's
    np.testing.assert_array_equal(col(nat.F_Y, 0), y)       # columns exactly
    np.testing.assert_array_equal(col(nat.F_E, 1), e[:, 1])
    sums, mom = dev.dist_perm_sums([ENV1, GEO], M.invert_rows(rows))
    got = M.mmrr(sums, mom, ['env', 'geo'])
    Y, Xs = fixture_matrices(D, x, y, e)
    host_sums, host_mom = M.numpy_perm_sums(Y, Xs, rows), M.numpy_moments(Y, Xs)
    assert_matches_reference(got, ref, host_sums, host_mom, 'case ' + tag.upper())


# ------------------------------------------------------------------ the public calls
def _small_model(seed):
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    mod = gnx.make_model(small_params(seed=seed))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(5, 'main', verbose=False)
    return mod


def test_model_run_mmrr_and_run_mantel_match_the_host_path():
    mod = _small_model(5)
    spp = mod.comm[0]
    ids = np.array([*spp])
    n = ids.size
    res = mod.run_mmrr(seed=3, nperm=99)                     # 'geo' and 'env' = layers 0 and 1
    par = mod.run_mantel('env', given='geo', seed=3, nperm=99)
    # the same inputs, downloaded: dosages and columns in ascending-id order
    D = np.rint(mod.get_genotypes() * 2).astype(np.int64)
    xy = np.column_stack([mod.get_x(), mod.get_y()])
    e = mod.get_e()
    assert D.shape[0] == n and e.shape == (n, 2)
    Y = M.genetic_distances(D)
    rows = M.draw_row_shuffles(n, 99, seed=3)
    Xs = [M.euclid(xy), M.euclid(e)]
    sums, mom = M.numpy_perm_sums(Y, Xs, rows), M.numpy_moments(Y, Xs)
    ref = M.mmrr(sums, mom, ['geo', 'env'])
    assert list(res) == list(ref)
    gap = smallest_gap(sums, mom)
    print('model: smallest relative gap %.3g' % gap)
    assert gap > GAP
    groups = (['Intercept', 'geo', 'env'], ['Intercept(t)', 'geo(t)', 'env(t)'],
              ['F-statistic'], ['R^2'])
    for keys in groups:
        r = np.array([ref[k] for k in keys])
        err = np.abs(np.array([res[k] for k in keys]) - r).max() / np.abs(r).max()
        print('%s: %.3g of the largest entry' % (keys[-1], err))
        assert err <= BAR, (keys, err)
    for k in ('Intercept(p)', 'geo(p)', 'env(p)', 'F p-value'):
        assert res[k] == ref[k], k
    # the partial Mantel test: env given geo
    sums2 = sums[:, ::-1]
    mom2 = dict(mom, sx=mom['sx'][::-1], sxy=mom['sxy'][::-1], sxx=mom['sxx'][::-1, ::-1])
    pref = M.mantel(sums2, mom2, 0, 1)
    assert np.abs(pref['perm_r'] - pref['r']).min() > GAP * abs(pref['r'])
    assert abs(par['r'] - pref['r']) <= BAR and par['nperm'] == 99
    assert np.abs(par['perm_r'] - pref['perm_r']).max() <= BAR
    assert par['p'] == pref['p']
    # the selections reach the device call; a sample of n is drawn from the model's generator
    some = ids[::3][::-1]
    sub = mod.run_mmrr(predictors=('phn', 'geo'), trts=[0], individs=some, loci=np.arange(8, 40),
                       nperm=19, seed=1)
    z = mod.get_z()[::3, :1]
    Ys = M.genetic_distances(D[::3, 8:40])
    Xz = [M.euclid(z), M.euclid(xy[::3])]
    r19 = M.draw_row_shuffles(some.size, 19, seed=1)
    want = M.mmrr(M.numpy_perm_sums(Ys, Xz, r19), M.numpy_moments(Ys, Xz), ['phn', 'geo'])
    for k in want:
        if not k.endswith('(p)') and k != 'F p-value':
            assert abs(sub[k] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), k
    assert mod.run_mantel(n=50, nperm=9)['perm_r'].shape == (9,)
    with pytest.raises(ValueError, match='not alive'):
        mod.run_mmrr(individs=[ids[-1] + 1000], nperm=5)
    from geonomics_amd.structs.tiled import TiledSpecies
    for name in ('_run_mmrr', '_run_mantel'):
        with pytest.raises(NotImplementedError):
            getattr(TiledSpecies, name)(spp)


def test_the_tests_leave_the_model_as_it_was():
    """genotypes, columns and the next walk step: byte-identical with and without the calls"""
    a, b = _small_model(7), _small_model(7)
    a.run_mmrr(nperm=9, seed=1)
    a.run_mantel('env', given='geo', nperm=9, seed=1)
    for step in range(2):
        np.testing.assert_array_equal(np.array([*a.comm[0]]), np.array([*b.comm[0]]))
        assert a.get_genotypes(biallelic=True).tobytes() == b.get_genotypes(biallelic=True).tobytes()
        assert a.get_x().tobytes() == b.get_x().tobytes()
        assert a.get_e().tobytes() == b.get_e().tobytes()
        a.walk(1, 'main', verbose=False)
        b.walk(1, 'main', verbose=False)
