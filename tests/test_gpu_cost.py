"""Least-cost distances and matrix predictors on the device (csrc/gnx_cost.hip,
gnx_dist_perm_sums_mat in csrc/gnx_mantel.hip, Model.calc_cost_distances and the 'cost'
predictor of run_mmrr / run_mantel).  Needs an MI355X.

The yardstick of the solver is the host restatement (sim/cost.py: scipy's Dijkstra on the graph
with the same fp64 edge expression).  The distances are the fixed point of a monotone
relaxation, so a correct solver reaches the same values whatever its order; the bound allows one
rounding per edge of a path no longer than the raster,

    |d - d_ref| <= n_cells 2^-52 d_ref,        the inf pattern equal.

Measured on an MI355X: the worst |d - d_ref| / bound is 0 in every case of this file: all
surfaces and matrices were bit-equal to the restatement.  The serpentine raster (14 sources, 6
tiles) took 19 rounds and 4.5 ms of kernel time with square cells, 17 rounds and 3.2 ms with
2 x 0.5 cells; its 300-cell matrix 19 rounds in one batch, 2384 rounds in 150 batches of two.

The cross-sums with matrix predictors are held to the bounds of test_gpu_mmrr.py:
|S - S_ref| <= (m + 8) 2^-53 sum |y| |x| for the sums and the moments sum y, sum y^2, sum x_k,
sum y x_k (a gathered matrix entry carries no rounding of its own, so the bound of a
two-column predictor covers it), (m + 16) for sum x_k x_l.  The statistics of the end-to-end
tests meet 1e-9 of the largest |entry| of their group; p-values are compared for equality only
after the host-side smallest-gap check.  Measured: the worst error is 3.3e-5 of its bound at
n = 1031 (2.2e-5 for a Euclidean matrix against numpy, 1.2e-5 against the old entry), 1.7e-2 of
it at n = 65; the model's statistics are within 6e-13 of the largest entry of their group, the
smallest relative gap of a permuted statistic from the observed one 2.6e-4."""
import numpy as np
import pytest

from test_gpu_parity import native
from test_mmrr_host import BAR, GAP, smallest_gap
from geonomics_amd.sim import cost as K
from geonomics_amd.sim import mmrr as M

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
INF = np.inf
GEO = [(0, 0), (1, 0)]                  # (GNX_F_X, 0), (GNX_F_Y, 0)
ENV1 = [(5, 1)]                         # layer 1 of GNX_F_E


# ------------------------------------------------------------------ the solver
def _device(nat, H, W):
    dev = nat.Device(W, H, 1)
    dev.upload_rasters(np.ones((1, H, W), np.float32))
    return dev


def serpentine():
    """70 x 133 (2 x 3 ragged tiles of 64): R = 1 / max(U(0, 1), 0.05); impassable columns at
    x = 10, 22, ... with a gap of 3 cells at alternating ends, so that a path crosses the tile
    borders back and forth; a block of barrier cells with a passable 2 x 2 pocket inside"""
    H, W = 70, 133
    R = 1.0 / np.maximum(np.random.RandomState(5).rand(H, W), 0.05)
    for k, x in enumerate(range(10, W, 12)):
        R[:, x] = INF
        if k % 2 == 0:
            R[:3, x] = 1.0 + k
        else:
            R[-3:, x] = 1.0 + k
    R[30:34, 40:44] = INF
    R[31:33, 41:43] = 2.0
    src = [0, H * W - 1, W - 1, (H - 1) * W,                 # the corners
           31 * W + 41,                                      # inside the pocket
           20 * W + 22,                                      # on a barrier cell
           63 * W + 5, 64 * W + 70, 5 * W + 63, 40 * W + 64, 66 * W + 127, 3 * W + 128,
           63 * W + 63, 64 * W + 128]                        # tile corners
    return R, np.array(src, np.int32)


_REF = {}


def _ref_surfaces(key, R, res, src):
    """the restatement, computed once per case"""
    if key not in _REF:
        _REF[key] = K.numpy_cost_surfaces(R, res, src)
    return _REF[key]


def _compare(got, ref, label):
    assert got.shape == ref.shape and got.dtype == np.float64
    np.testing.assert_array_equal(np.isinf(got), np.isinf(ref))
    assert not np.isnan(got).any()
    ok = np.isfinite(ref)
    n_cells = ref.shape[-1] * ref.shape[-2]
    err, bound = np.abs(got[ok] - ref[ok]), n_cells * 2.0 ** -52 * ref[ok]
    worst = float((err / np.maximum(bound, 1e-300)).max()) if ok.any() else 0.0
    print('%s: %d sources, %d finite, %d inf, worst error / bound %.3g, bit-equal: %s'
          % (label, ref.shape[0], ok.sum(), (~ok).sum(), worst, bool((got[ok] == ref[ok]).all())))
    assert (err <= bound).all(), (label, worst)
    return worst


@pytest.fixture(scope='module')
def snake():
    nat = native()
    R, src = serpentine()
    dev = _device(nat, *R.shape)
    yield nat, dev, R, src
    dev.close()


@pytest.mark.parametrize('res', [(1.0, 1.0), (2.0, 0.5)], ids=['square', 'res_2_0.5'])
def test_surfaces_on_the_serpentine_raster(snake, res):
    nat, dev, R, src = snake
    got = dev.cost_surfaces(R, res, src)
    ref = _ref_surfaces(('snake', res), R, res, src)
    _compare(got, ref, 'serpentine %s' % (res,))
    H, W = R.shape
    assert (got[np.arange(src.size), src // W, src % W] == 0).all()        # d(s, s) = 0
    pocket, wall = got[4], got[5]
    assert np.isfinite(pocket).sum() == 4 and np.isfinite(wall).sum() == 1
    assert np.isinf(got[0][31:33, 41:43]).all() and np.isfinite(got[0][-1, -1])
    info = dev.cost_info()
    print('info: %s' % info)
    # the far corner is reached only by crossing the tile borders again and again
    assert info['rounds'] > 6 and info['batches'] == 1 and info['launches'] >= 2 * info['rounds']
    assert info['kernel_ms'] > 0
    again = dev.cost_surfaces(R, res, src)
    np.testing.assert_array_equal(again, got)


@pytest.mark.parametrize('H,W', [(24, 24), (1, 200), (64, 64), (65, 129), (1, 1), (130, 3)],
                         ids=lambda v: str(v))
def test_surfaces_at_every_tile_edge(H, W):
    """smaller than a tile, one row, exactly one tile, one cell past the tiles, one cell"""
    nat = native()
    rng = np.random.RandomState(H * 1000 + W)
    R = 1.0 / np.maximum(rng.rand(H, W), 0.05)
    if H * W > 4:
        shut = rng.choice(H * W, H * W // 10, replace=False)
        R.ravel()[shut] = INF
    src = np.unique(np.concatenate([[0, H * W - 1, (H // 2) * W + W // 2],
                                    rng.choice(H * W, min(4, H * W))])).astype(np.int32)
    dev = _device(nat, H, W)
    try:
        for res in ((1.0, 1.0), (0.5, 3.0)):
            _compare(dev.cost_surfaces(R, res, src), K.numpy_cost_surfaces(R, res, src),
                     '%d x %d %s' % (H, W, res))
    finally:
        dev.close()


def test_cost_matrix_of_300_cells(snake):
    nat, dev, R, src = snake
    H, W = R.shape
    cells = np.random.RandomState(7).choice(H * W, 300, replace=False).astype(np.int32)
    dev.cost_budget(0)
    D = dev.cost_matrix(R, (1.0, 1.0), cells)
    base = dev.cost_info()
    ref = K.numpy_cost_matrix(R, (1.0, 1.0), cells)
    _compare(D[None], ref[None], 'matrix of 300 cells')
    np.testing.assert_array_equal(D, D.T)
    assert (np.diag(D) == 0).all() and np.isinf(D).any()     # some cells lie on a barrier
    np.testing.assert_array_equal(dev.cost_matrix(R, (1.0, 1.0), cells), D)      # repeated
    # two sources' rasters per batch: 150 batches, the same bits
    dev.cost_budget(2 * H * W * 8)
    D2 = dev.cost_matrix(R, (1.0, 1.0), cells)
    info = dev.cost_info()
    print('default budget: %s; two sources per batch: %s' % (base, info))
    assert base['batches'] == 1 and info['batches'] == 150
    np.testing.assert_array_equal(D2, D)
    dev.cost_budget(0)
    # one cell, and the order of the cells is the order of the rows
    np.testing.assert_array_equal(dev.cost_matrix(R, (1.0, 1.0), cells[:1]), [[0.0]])
    flip = dev.cost_matrix(R, (1.0, 1.0), cells[::-1].copy())
    ok = np.isfinite(D)
    assert (np.isfinite(flip[::-1, ::-1]) == ok).all()
    assert (np.abs(flip[::-1, ::-1][ok] - D[ok]) <= H * W * 2.0 ** -52 * D[ok]).all()


def test_refusals(snake):
    nat, dev, R, src = snake
    H, W = R.shape
    ok = np.array([0, 5, 9], np.int32)
    before = dev.cost_matrix(R, (1.0, 1.0), ok)
    for bad in ([0, 5, 5], [0, -1], [0, H * W]):
        with pytest.raises(nat.GnxError, match='listed twice|not a cell'):
            dev.cost_matrix(R, (1.0, 1.0), np.array(bad, np.int32))
    for bad in ([-1], [H * W]):
        with pytest.raises(nat.GnxError, match='not a cell'):
            dev.cost_surfaces(R, (1.0, 1.0), np.array(bad, np.int32))
    with pytest.raises(nat.GnxError, match='at least one source'):
        dev.cost_surfaces(R, (1.0, 1.0), np.zeros(0, np.int32))
    with pytest.raises(nat.GnxError, match='cells'):
        dev.cost_matrix(R, (1.0, 1.0), np.zeros(0, np.int32))
    with pytest.raises(nat.GnxError, match='bytes >= 0'):
        dev.cost_budget(-1)
    with pytest.raises(nat.GnxError, match="below one source's raster"):
        dev.cost_budget(H * W * 8 - 1)
    dev.cost_budget(H * W * 8)                               # one source per batch is enough
    np.testing.assert_array_equal(dev.cost_matrix(R, (1.0, 1.0), ok), before)
    assert dev.cost_info()['batches'] == 3
    dev.cost_budget(0)
    for v in (0.0, -1.0, np.nan, -INF):
        bad_R = R.copy()
        bad_R[3, 4] = v
        with pytest.raises(nat.GnxError, match='must be > 0'):
            dev.cost_surfaces(bad_R, (1.0, 1.0), ok)
    for res in ((0.0, 1.0), (1.0, -1.0), (INF, 1.0), (np.nan, 1.0)):
        with pytest.raises(nat.GnxError, match='res_x and res_y'):
            dev.cost_matrix(R, res, ok)
    with pytest.raises(ValueError, match='R'):
        dev.cost_surfaces(R[:, :-1], (1.0, 1.0), ok)
    np.testing.assert_array_equal(dev.cost_matrix(R, (1.0, 1.0), ok), before)
    # a handle that holds ghost records
    tile = _device(nat, 8, 8)
    tile.set_species_params(nat.default_species_params())
    tile.upload_population(np.ones(4), np.ones(4), np.zeros(4), np.zeros(4), np.arange(4))
    rec = np.zeros(1, nat.IND_REC)
    rec['x'], rec['y'], rec['id'] = 1.0, 1.0, 10 ** 6
    tile.tile_import_ghosts(rec)
    for call in (lambda: tile.cost_surfaces(np.ones((8, 8)), (1.0, 1.0), ok),
                 lambda: tile.cost_matrix(np.ones((8, 8)), (1.0, 1.0), ok)):
        with pytest.raises(nat.GnxError, match='ghost records'):
            call()
    bad = np.array([-1], np.int32)                           # the ghosts are what is reported
    for call in (lambda: tile.cost_surfaces(np.ones((8, 8)), (1.0, 1.0), bad),
                 lambda: tile.cost_matrix(np.ones((8, 8)), (1.0, 1.0), bad),
                 lambda: tile.cost_budget(0), lambda: tile.cost_info()):
        with pytest.raises(nat.GnxError, match='ghost records'):
            call()
    tile.close()


# ------------------------------------------------------------------ matrix predictors
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


@pytest.fixture(scope='module')
def big():
    """a random population, n = 1031 (17 tiles of 64: 153 tiles in more units than one, the
    last tile 7 rows), L = 200, three random layers; its genetic distances and a random
    symmetric matrix with a zero diagonal"""
    nat = native()
    rng = np.random.RandomState(31)
    n, L = 1031, 200
    D = rng.binomial(2, rng.uniform(0.1, 0.9, L), size=(n, L))
    rasts = np.stack([np.ones((20, 28)), rng.rand(20, 28), rng.rand(20, 28)])
    dev = _handle(nat, D, rng.uniform(0, 28, n), rng.uniform(0, 20, n), np.arange(n), rasts)
    A = rng.uniform(0.5, 30.0, (n, n))
    A = np.triu(A, 1) + np.triu(A, 1).T
    x, y, e = (dev.download(f).astype(np.float64) for f in (nat.F_X, nat.F_Y, nat.F_E))
    host = dict(Y=M.genetic_distances(D), geo=M.euclid(np.column_stack([x, y])),
                env=M.euclid(e[1]), A=A)
    yield nat, dev, host
    dev.close()


def _within(got, want, absum, m, c, what, worst):
    err, bound = np.abs(np.asarray(got) - np.asarray(want)), (m + c) * U53 * np.asarray(absum)
    worst.append(float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (what, err.max(), np.min(bound))


def _check_mat(dev, host, cols, col_keys, mat_keys, n_perm, seed, slots=None, label=''):
    """one call against numpy_perm_sums / numpy_moments on the host's matrices, twice bit-equal"""
    s = np.arange(host['Y'].shape[0]) if slots is None else slots
    n = s.size
    m = n * (n - 1) // 2
    sub = {k: v[np.ix_(s, s)] for k, v in host.items()}
    rows = M.draw_row_shuffles(n, n_perm, seed=seed)
    perm = M.invert_rows(rows)
    mats = np.stack([sub[k] for k in mat_keys]) if mat_keys else np.zeros((0, n, n))
    sums, mom = dev.dist_perm_sums_mat(cols, mats, perm, slots)
    Xs = [sub[k] for k in col_keys + mat_keys]
    S_ref, ref = M.numpy_perm_sums(sub['Y'], Xs, rows), M.numpy_moments(sub['Y'], Xs)
    assert sums.shape == S_ref.shape == (n_perm, len(Xs)) and mom['m'] == m
    worst = []
    _within(sums, S_ref, S_ref, m, 8, 'sums', worst)
    for k in ('sy', 'syy', 'sx', 'sxy'):
        _within(mom[k], ref[k], ref[k], m, 8, k, worst)
    _within(mom['sxx'], ref['sxx'], ref['sxx'], m, 16, 'sxx', worst)
    print('%s: n = %d, %d permutations, %d + %d predictors: worst error / bound %.3g'
          % (label, n, n_perm, len(col_keys), len(mat_keys), max(worst)))
    sums2, mom2 = dev.dist_perm_sums_mat(cols, mats, perm, slots)
    np.testing.assert_array_equal(sums2, sums)
    for k in mom:
        np.testing.assert_array_equal(mom2[k], mom[k])
    return sums, mom, perm


def test_a_euclidean_matrix_reproduces_the_column_predictor(big):
    nat, dev, host = big
    sums, mom, perm = _check_mat(dev, host, [], [], ['geo'], 65, 1, label='geo as a matrix')
    old_s, old_m = dev.dist_perm_sums([GEO], perm)
    m = 1031 * 1030 // 2
    worst = []
    _within(sums, old_s, old_s, m, 8, 'sums', worst)
    for k in ('sy', 'syy', 'sx', 'sxy'):
        _within(mom[k], old_m[k], old_m[k], m, 8, k, worst)
    _within(mom['sxx'], old_m['sxx'], old_m['sxx'], m, 16, 'sxx', worst)
    np.testing.assert_array_equal(mom['sy'], old_m['sy'])    # Y is the same Gram matrix
    print('matrix entry against the old entry: worst error / bound %.3g' % max(worst))


def test_a_random_matrix_alone_and_behind_columns(big):
    nat, dev, host = big
    _check_mat(dev, host, [], [], ['A'], 65, 2, label='random matrix')
    sums, mom, perm = _check_mat(dev, host, [GEO, ENV1], ['geo', 'env'], ['A', 'geo'], 130, 3,
                                 label='2 columns + 2 matrices')
    # the column predictors in front are the old entry's, term by term
    old_s, old_m = dev.dist_perm_sums([GEO, ENV1], perm)
    m = 1031 * 1030 // 2
    worst = []
    _within(sums[:, :2], old_s, old_s, m, 8, 'sums', worst)
    _within(mom['sxx'][:2, :2], old_m['sxx'], old_m['sxx'], m, 16, 'sxx', worst)


ENV012 = [(5, 0), (5, 1), (5, 2)]
WIDE = [ENV012[:2] * 2, ENV012[1:] * 2]                 # 8 columns: stripes of 8, not 16


def _assert_same_bits(got, want, k):
    """the sums and every moment of the first k predictors of `got` are those of `want`"""
    (s, mom), (s0, mom0) = got, want
    np.testing.assert_array_equal(s[:, :k], s0)
    for key in ('m', 'sy', 'syy'):
        np.testing.assert_array_equal(mom[key], mom0[key])
    for key in ('sx', 'sxy'):
        np.testing.assert_array_equal(mom[key][:k], mom0[key])
    np.testing.assert_array_equal(mom['sxx'][:k, :k], mom0['sxx'])


@pytest.mark.parametrize('sample', [None, 65], ids=['all', 'slots65'])
@pytest.mark.parametrize('cols', [[GEO, ENV1], WIDE], ids=['D3_stripes16', 'D8_stripes8'])
def test_no_matrix_is_the_column_call(big, cols, sample):
    """the matrix entry without a matrix takes the column path: the bits of dist_perm_sums, at
    both stripe widths"""
    nat, dev, host = big
    slots = None if sample is None else \
        np.random.RandomState(7).choice(1031, sample, replace=False).astype(np.int64)
    n = 1031 if sample is None else sample
    perm = M.invert_rows(M.draw_row_shuffles(n, 65, seed=5))
    got = dev.dist_perm_sums_mat(cols, np.zeros((0, n, n)), perm, slots)
    assert got[0].shape == (65, len(cols))
    _assert_same_bits(got, dev.dist_perm_sums(cols, perm, slots), len(cols))


def test_wide_columns_in_front_of_a_matrix_are_the_column_call(big):
    """with more than 4 columns the column-only call works in stripes of 8 as the matrix path
    does, so a column predictor's terms are added in the same order: the same bits (with 4
    columns or fewer the widths differ, and the bound asserted in
    test_a_random_matrix_alone_and_behind_columns is what holds)"""
    nat, dev, host = big
    slots = np.random.RandomState(8).choice(1031, 131, replace=False).astype(np.int64)
    cols = [GEO, ENV012]
    perm = M.invert_rows(M.draw_row_shuffles(131, 65, seed=6))
    got = dev.dist_perm_sums_mat(cols, host['A'][np.ix_(slots, slots)][None], perm, slots)
    assert got[0].shape == (65, 3)
    _assert_same_bits(got, dev.dist_perm_sums(cols, perm, slots), 2)


@pytest.mark.parametrize('n', [2, 65])
def test_a_sample_of_slots(big, n):
    nat, dev, host = big
    slots = np.random.RandomState(n).choice(1031, n, replace=False).astype(np.int64)
    _check_mat(dev, host, [ENV1], ['env'], ['A'], 70, 4, slots, label='n = %d' % n)


def test_bad_matrices_are_refused(big):
    nat, dev, host = big
    slots = np.arange(40, dtype=np.int64)
    A = host['A'][:40, :40].copy()
    perm = np.arange(40, dtype=np.int32)[None, :]
    before = dev.dist_perm_sums_mat([GEO], A[None], perm, slots)
    for (i, j, v), match in (((3, 7, A[3, 7] + 1e-9), 'not symmetric'),
                             ((7, 3, np.nan), 'non-finite'), ((3, 7, INF), 'non-finite'),
                             ((5, 5, 1e-300), 'diagonal')):
        B = A.copy()
        B[i, j] = v
        with pytest.raises(nat.GnxError, match=match):
            dev.dist_perm_sums_mat([GEO], np.stack([A, B]), perm, slots)
    with pytest.raises(nat.GnxError, match='predictors'):
        dev.dist_perm_sums_mat([], np.zeros((0, 40, 40)), perm, slots)
    with pytest.raises(nat.GnxError, match='predictors'):
        dev.dist_perm_sums_mat([GEO, ENV1], np.stack([A] * 3), perm, slots)
    with pytest.raises(ValueError, match='mats'):
        dev.dist_perm_sums_mat([GEO], A[None, :39, :39], perm, slots)
    bad = perm.copy()
    bad[0, 9] = 40
    with pytest.raises(nat.GnxError, match=r'perm\[0\]\[9\]'):
        dev.dist_perm_sums_mat([], A[None], bad, slots)
    after = dev.dist_perm_sums_mat([GEO], A[None], perm, slots)
    np.testing.assert_array_equal(after[0], before[0])


# ------------------------------------------------------------------ the public calls
def _cost_model(seed):
    """the 24 x 24 two-layer landscape of the other Model tests (all ones; a west-east gradient
    from 0 to 1), the Species moving along layer 1 as its move_surf"""
    import geonomics_amd as gnx
    from geonomics_amd.sim import params as P
    d = P.default_params_dict(layers=[{'type': 'defined'}, {'type': 'defined'}],
                              species=[{'genomes': True, 'n_traits': 1,
                                        'movement_surface': True}])
    d['landscape']['main']['dim'] = (24, 24)
    d['landscape']['layers']['lyr_0']['init']['defined']['rast'] = np.ones((24, 24))
    d['landscape']['layers']['lyr_1']['init']['defined']['rast'] = \
        np.tile(np.linspace(0, 1, 24), (24, 1))
    s = d['comm']['species']['spp_0']
    s['init'].update({'N': 250, 'K_factor': 0.5})
    s['mating'].update({'mating_radius': 4})
    s['movement']['move_surf'].update({'layer': 'lyr_1'})
    s['gen_arch'].update({'L': 64, 'n_recomb_sims': 200, 'use_tskit': False})
    s['gen_arch']['traits']['trait_0'].update({'layer': 'lyr_1', 'n_loci': 4})
    d['model'].update({'T': 12, 'burn_T': 30, 'seed': {'num': seed}})
    mod = gnx.make_model(gnx.make_params_dict(d, 'cost_test'))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(5, 'main', verbose=False)
    return mod


def test_model_calls_match_the_host_composition():
    mod = _cost_model(5)
    spp = mod.comm[0]
    ids = np.array([*spp])
    cells = mod.get_cells()
    rast = np.tile(np.linspace(0, 1, 24), (24, 1))
    R = K.resistance_raster(rast)                            # column 0 has conductance 0
    lin = cells[:, 1] * 24 + cells[:, 0]
    uniq, inv = np.unique(lin, return_inverse=True)
    want = K.expand(K.numpy_cost_matrix(R, (1, 1), uniq), inv)
    res = mod.calc_cost_distances()
    np.testing.assert_array_equal(res['ids'], ids)
    np.testing.assert_array_equal(res['cells'], cells)
    _compare(res['dist'][None], want[None], 'calc_cost_distances, n = %d' % ids.size)
    np.testing.assert_array_equal(res['dist'], res['dist'].T)
    surf = mod.calc_cost_surface([3.5, 20.1], [4.2, 23.9])
    _compare(surf, K.numpy_cost_surfaces(R, (1, 1), [4 * 24 + 3, 23 * 24 + 20]),
             'calc_cost_surface')
    # the tests on the individuals that a path joins (nobody of column 0)
    some = ids[cells[:, 0] >= 1]
    sel = np.isin(ids, some)
    n = some.size
    assert n >= 30                                           # 435 pairs for 3 coefficients
    got = mod.run_mmrr(predictors=('geo', 'cost'), individs=some, nperm=199, seed=3)
    par = mod.run_mantel('cost', given='geo', individs=some, nperm=199, seed=3)
    D = np.rint(mod.get_genotypes() * 2).astype(np.int64)[sel]
    xy = np.column_stack([mod.get_x(), mod.get_y()])[sel]
    Y = M.genetic_distances(D)
    Xs = [M.euclid(xy), want[np.ix_(sel, sel)]]
    rows = M.draw_row_shuffles(n, 199, seed=3)
    sums, mom = M.numpy_perm_sums(Y, Xs, rows), M.numpy_moments(Y, Xs)
    ref = M.mmrr(sums, mom, ['geo', 'cost'])
    assert list(got) == list(ref)
    gap = smallest_gap(sums, mom)
    print('model: smallest relative gap %.3g' % gap)
    assert gap > GAP
    for keys in (['Intercept', 'geo', 'cost'], ['Intercept(t)', 'geo(t)', 'cost(t)'],
                 ['F-statistic'], ['R^2']):
        r = np.array([ref[k] for k in keys])
        err = np.abs(np.array([got[k] for k in keys]) - r).max() / np.abs(r).max()
        print('%s: %.3g of the largest entry' % (keys[-1], err))
        assert err <= BAR, (keys, err)
    for k in ('Intercept(p)', 'geo(p)', 'cost(p)', 'F p-value'):
        assert got[k] == ref[k], k
    sums2 = sums[:, ::-1]
    mom2 = dict(mom, sx=mom['sx'][::-1], sxy=mom['sxy'][::-1], sxx=mom['sxx'][::-1, ::-1])
    pref = M.mantel(sums2, mom2, 0, 1)
    assert np.abs(pref['perm_r'] - pref['r']).min() > GAP * abs(pref['r'])
    assert abs(par['r'] - pref['r']) <= BAR and par['nperm'] == 199
    assert np.abs(par['perm_r'] - pref['perm_r']).max() <= BAR
    assert par['p'] == pref['p']
    # everybody: somebody stands in column 0 sooner or later, and is refused by number
    n_inf = int(np.isinf(want[np.tril_indices(ids.size, -1)]).sum())
    if n_inf:
        with pytest.raises(ValueError, match='%d pairs .*infinite cost' % n_inf):
            mod.run_mmrr(predictors=('geo', 'cost'), nperm=9, seed=1)
    # the default call is the old entry's, bit for bit
    a = mod.run_mmrr(nperm=49, seed=2)
    _, slots = spp._geno_sample(None)
    sums_old, mom_old = spp._dev.dist_perm_sums(
        [GEO, ENV1], M.invert_rows(M.draw_row_shuffles(ids.size, 49, seed=2)), slots)
    b = M.mmrr(sums_old, mom_old, ['geo', 'env'])
    assert list(a) == list(b) and all(a[k] == b[k] for k in b)
