"""Least-cost distances and the 'cost' predictor on the CPU (geonomics_amd/sim/cost.py,
Species._calc_cost_distances / _calc_cost_surface, the 'cost' entries of run_mmrr / run_mantel),
with numpy in place of the device.

The resistance raster from a layer (the three kinds, barriers, every refusal); the restatement
(scipy's Dijkstra on the pinned graph) against costs worked out by hand; the public calls on a
stand-in Species whose device is the restatement: de-duplication and expansion of the cells, the
parsing of 'cost' predictors, the reordering of the library's column-then-matrix order back to
the caller's, and the refusals.  A hand-computed cost is one fp64 expression evaluated in the
path's order, so the restatement must equal it exactly."""
import inspect
import types

import numpy as np
import pytest

from geonomics_amd.sim import cost as K
from geonomics_amd.sim import mmrr as M
from geonomics_amd.structs.analyses import SpeciesAnalyses
from geonomics_amd.structs.landscape import Landscape, Layer
from test_mmrr_host import BAR, GAP, lstsq_fit, small_sample, smallest_gap

F_X, F_Y, F_E, F_Z = 0, 1, 5, 6
INF = np.inf
R2 = np.sqrt(2.0)


# ------------------------------------------------------------------ the resistance raster
def test_conductance_is_inverted_and_closed_at_the_barrier():
    v = np.array([[1.0, 0.5, 0.0], [0.25, 0.1, 0.2]])
    np.testing.assert_array_equal(K.resistance_raster(v), [[1, 2, INF], [4, 1 / 0.1, 1 / 0.2]])
    np.testing.assert_array_equal(K.resistance_raster(v, kind='conductance', barrier=0.2),
                                  [[1, 2, INF], [4, INF, INF]])
    # a negative barrier opens nothing: 1 / 0 is no resistance
    assert K.resistance_raster(v, barrier=-1.0)[0, 2] == INF
    assert K.resistance_raster(v).dtype == np.float64


def test_resistance_is_taken_as_it_is():
    v = np.array([[1.0, 0.5], [3.0, 0.25]])
    np.testing.assert_array_equal(K.resistance_raster(v, kind='resistance'), v)
    np.testing.assert_array_equal(K.resistance_raster(v, kind='resistance', barrier=1.0),
                                  [[INF, 0.5], [INF, 0.25]])
    with pytest.raises(ValueError, match='passable value must be > 0'):
        K.resistance_raster(np.array([[1.0, 0.0]]), kind='resistance')
    # a zero lies below every barrier: it stays passable, and is refused
    with pytest.raises(ValueError, match='> 0'):
        K.resistance_raster(np.array([[1.0, 0.0]]), kind='resistance', barrier=0.5)
    np.testing.assert_array_equal(
        K.resistance_raster(np.array([[1.0, INF]]), kind='resistance'), [[1.0, INF]])


def test_an_explicit_cost_raster_overrides_the_layer():
    v = np.ones((2, 3))
    c = np.array([[1.0, np.nan, 2.0], [INF, 0.5, 7.0]])
    got = K.resistance_raster(v, kind='resistance', barrier=0.1, cost=c)
    np.testing.assert_array_equal(got, [[1, INF, 2], [INF, 0.5, 7]])
    assert np.isnan(c[0, 1])                                 # the caller's array is left alone
    np.testing.assert_array_equal(K.resistance_raster(cost=c, shape=(2, 3)), got)
    with pytest.raises(ValueError, match='shape'):
        K.resistance_raster(v, cost=np.ones((3, 2)))
    with pytest.raises(ValueError, match='shape'):
        K.resistance_raster(cost=np.ones(6), shape=(2, 3))
    for bad in (0.0, -1.0, -INF):
        with pytest.raises(ValueError, match='passable entry must be > 0'):
            K.resistance_raster(v, cost=np.array([[1.0, bad, 1.0], [1.0, 1.0, 1.0]]))


def test_the_other_refusals():
    with pytest.raises(ValueError, match='kind'):
        K.resistance_raster(np.ones((2, 2)), kind='friction')
    with pytest.raises(ValueError, match='no layer'):
        K.resistance_raster()
    with pytest.raises(ValueError, match='raster'):
        K.resistance_raster(np.ones(4))
    with pytest.raises(ValueError, match='nan'):
        K.resistance_raster(np.array([[1.0, np.nan]]))
    with pytest.raises(ValueError, match='shape'):
        K.resistance_raster(np.ones((2, 2)), shape=(2, 3))


# ------------------------------------------------------------------ the restatement, by hand
def test_a_3_by_3_raster_by_hand():
    R = np.array([[1.0, 1.0, 1.0], [1.0, 4.0, 1.0], [1.0, 1.0, 1.0]])
    d = K.numpy_cost_surfaces(R, (1.0, 1.0), [0])[0]
    side, diag_mid = (0.5 * (1.0 + 1.0)) * 1.0, (0.5 * (1.0 + 4.0)) * R2
    want = np.array([[0.0, side, side + side],
                     [side, side + (0.5 * (1.0 + 4.0)) * 1.0, side + (0.5 * (1.0 + 1.0)) * R2],
                     [side + side, side + (0.5 * (1.0 + 1.0)) * R2,
                      (side + (0.5 * (1.0 + 1.0)) * R2) + side]])
    np.testing.assert_array_equal(d, want)
    assert want[1, 1] == 3.5 < diag_mid                      # round the corner, not across
    assert want[2, 2] < 2 * diag_mid                         # and round the dear centre
    # from the centre every step carries half of its 4
    c = K.numpy_cost_surfaces(R, (1.0, 1.0), [4])[0]
    assert 2.5 + 1.0 < 2.5 * R2                              # a corner: straight, then along
    np.testing.assert_array_equal(c, [[3.5, 2.5, 3.5], [2.5, 0, 2.5], [3.5, 2.5, 3.5]])


def test_a_1_by_5_raster_with_a_wall():
    R = np.array([[1.0, 2.0, 4.0, INF, 1.0]])
    d = K.numpy_cost_surfaces(R, (1.0, 1.0), [0, 4, 3])
    np.testing.assert_array_equal(d[0], [[0.0, 1.5, 4.5, INF, INF]])
    np.testing.assert_array_equal(d[1], [[INF, INF, INF, INF, 0.0]])
    # an impassable source: 0 on itself, inf everywhere else
    np.testing.assert_array_equal(d[2], [[INF, INF, INF, 0.0, INF]])
    np.testing.assert_array_equal(K.numpy_cost_surfaces(R, (3.0, 1.0), [2])[0],
                                  [[13.5, 9.0, 0.0, INF, INF]])


def test_a_single_cell():
    np.testing.assert_array_equal(K.numpy_cost_surfaces(np.array([[5.0]]), (1, 1), [0, 0]),
                                  np.zeros((2, 1, 1)))
    np.testing.assert_array_equal(K.numpy_cost_matrix(np.array([[INF]]), (1, 1), [0]), [[0.0]])


def test_cells_that_are_not_square():
    R = np.array([[1.0, 3.0], [1.0, 1.0]])
    d = K.numpy_cost_surfaces(R, (2.0, 0.5), [0])[0]
    diag = np.sqrt(2.0 * 2.0 + 0.5 * 0.5)
    east, south = (0.5 * (1.0 + 3.0)) * 2.0, (0.5 * (1.0 + 1.0)) * 0.5
    assert d[1, 0] == south == 0.5
    assert d[1, 1] == (0.5 * (1.0 + 1.0)) * diag < south + 2.0
    # (0, 1): straight east 4, south and the diagonal 4.6, or the diagonal and north 3.06
    north = (0.5 * (1.0 + 3.0)) * 0.5
    assert d[0, 1] == d[1, 1] + north < min(east, south + (0.5 * (1.0 + 3.0)) * diag)
    np.testing.assert_array_equal(K.numpy_cost_surfaces(R, (-2.0, 0.5), [0])[0], d)   # |res|


def test_an_impassable_source_and_an_enclosed_cell():
    R = np.ones((3, 4))
    R[0, 0] = INF
    R[:, 2] = INF                                            # column 3 is cut off
    D = K.numpy_cost_matrix(R, (1.0, 1.0), [0, 5, 3, 11, 4])
    assert (D == D.T).all() and (np.diag(D) == 0).all()
    assert np.isinf(D[0, 1:]).all()                          # the impassable source
    assert D[1, 4] == 1.0 and D[2, 3] == 2.0                 # (1, 1)-(1, 0); column 3, rows 0-2
    assert np.isinf(D[1, 2]) and np.isinf(D[4, 3])


def test_the_matrix_is_the_surfaces_of_the_lower_index():
    rng = np.random.RandomState(1)
    R = 1.0 / np.maximum(rng.rand(9, 11), 0.05)
    R[3:6, 4] = INF
    cells = rng.choice(99, 20, replace=False)
    S_ = K.numpy_cost_surfaces(R, (1.0, 1.5), cells).reshape(20, -1)[:, cells]
    D = K.numpy_cost_matrix(R, (1.0, 1.5), cells)
    a, b = np.triu_indices(20, 1)
    np.testing.assert_array_equal(D[a, b], S_[a, b])
    np.testing.assert_array_equal(D[b, a], S_[a, b])
    ok = np.isfinite(S_)
    assert (ok == ok.T).all() and 0 < (~ok).sum() < 60       # a cell of the wall was drawn
    assert np.abs(S_[ok] - S_.T[ok]).max() <= 99 * 2.0 ** -52 * S_[ok].max()   # the other direction
    with pytest.raises(ValueError, match='listed twice'):
        K.numpy_cost_matrix(R, (1, 1), [3, 4, 3])
    for bad in ([-1], [99]):
        with pytest.raises(ValueError, match=r'0\.\.98'):
            K.numpy_cost_matrix(R, (1, 1), bad)
        with pytest.raises(ValueError, match=r'0\.\.98'):
            K.numpy_cost_surfaces(R, (1, 1), bad)
    for bad_R in (np.zeros((2, 2)), -np.ones((2, 2)), np.full((2, 2), np.nan), np.ones(4)):
        with pytest.raises(ValueError, match='R'):
            K.numpy_cost_surfaces(bad_R, (1, 1), [0])
    with pytest.raises(ValueError, match='res'):
        K.numpy_cost_surfaces(np.ones((2, 2)), (0.0, 1.0), [0])
    np.testing.assert_array_equal(K.expand(np.array([[0.0, 2.0], [2.0, 0.0]]), [1, 0, 1]),
                                  [[0, 2, 0], [2, 0, 2], [0, 2, 0]])


# ------------------------------------------------------------------ the public calls
W_, H_ = 12, 9


def _land(seed=2, wall=True):
    """two layers over 12 x 9 cells of size (1, 1.5): all ones, and a conductance in (0.05, 1]
    with a wall of zeros in column 6 that leaves two gaps"""
    rng = np.random.RandomState(seed)
    cond = np.maximum(rng.rand(H_, W_), 0.05)
    if wall:
        cond[1:8, 6] = 0.0
    lyrs = {0: Layer(np.ones((H_, W_)), 'defined', 'flat', (W_, H_), res=(1, 1.5)),
            1: Layer(cond, 'defined', 'cond', (W_, H_), res=(1, 1.5))}
    return Landscape(lyrs, res=(1, 1.5))


class _Dev:
    """the device's calls in numpy, on columns kept in slot order"""

    def __init__(self, D, x, y, e, z):
        self.D, self.x, self.y, self.e, self.z = D, x, y, e, z
        self.L = D.shape[1]
        self.W64 = (self.L + 1023) // 1024 * 16
        self.cfg = types.SimpleNamespace(n_layers=e.shape[1], W=W_, H=H_)
        self.calls = []

    def _matrices(self, predictors, slots):
        src = {F_X: lambda i: self.x, F_Y: lambda i: self.y, F_E: lambda i: self.e[:, i],
               F_Z: lambda i: self.z[:, i]}
        return [M.euclid(np.column_stack([src[f](i)[slots] for f, i in cols]))
                for cols in predictors]

    def _sums(self, Xs, perm, slots):
        Y = M.genetic_distances(self.D[slots])
        sums = np.array([[M.unfold_tril(Y) @ M.unfold_tril(X[q][:, q]) for X in Xs]
                         for q in perm])
        return sums, M.numpy_moments(Y, Xs)

    def dist_perm_sums(self, predictors, perm, slots=None, locus_mask=None):
        self.calls.append(('cols', predictors, perm.copy(), slots))
        return self._sums(self._matrices(predictors, slots), perm, slots)

    def dist_perm_sums_mat(self, predictors, mats, perm, slots=None, locus_mask=None):
        self.calls.append(('mat', predictors, np.array(mats), perm.copy(), slots))
        return self._sums(self._matrices(predictors, slots) + list(mats), perm, slots)

    def cost_matrix(self, R, res, cells):
        self.calls.append(('cost_matrix', R.copy(), tuple(res), np.array(cells)))
        return K.numpy_cost_matrix(R, res, cells)

    def cost_surfaces(self, R, res, src):
        self.calls.append(('cost_surfaces', R.copy(), tuple(res), np.array(src)))
        return K.numpy_cost_surfaces(R, res, src)


class _Species(SpeciesAnalyses):
    """a Species stand-in: the real methods over the numpy device"""

    def __init__(self, D, x, y, e, z, ids, land, move_surf=1):
        self._dev = _Dev(D, x, y, e, z)
        self.ids = np.asarray(ids)
        trt = types.SimpleNamespace(lyr_num=1, loci=np.array([2, 5]), name='trait_0')
        self.gen_arch = types.SimpleNamespace(traits={0: trt})
        self._genomes_assigned = True
        self._rng = np.random.RandomState(77)
        self.name = 'spp_0'
        self._land_ref = land
        self._land_dim = tuple(land.dim)
        self._land_res = land.res
        self._move_surf = None if move_surf is None else True
        mv = {} if move_surf is None else {'move_surf': {'layer': move_surf}}
        self._spp_params = types.SimpleNamespace(movement=types.SimpleNamespace(**mv))

    def _geno_sample(self, individs):
        order = np.argsort(self.ids)
        if individs is None:
            return self.ids[order], order
        ids = np.sort(np.asarray(individs))
        return ids, order[np.searchsorted(self.ids[order], ids)]

    def _get_cells(self, individs=None):
        _, slots = self._geno_sample(individs)
        return np.int32(np.floor(np.column_stack([self._dev.x, self._dev.y])[slots]))

    def __iter__(self):
        return iter(np.sort(self.ids).tolist())

    def _get_individs(self, ids):
        return {int(i): None for i in ids}


def _model(spp):
    from geonomics_amd.sim.model import Model
    mod = types.SimpleNamespace(comm={0: spp}, _rng=np.random.RandomState(9))
    for name in ('_get_spp_num', '_test_sample', 'run_mmrr', 'run_mantel', 'calc_cost_distances',
                 'calc_cost_surface'):
        setattr(mod, name, types.MethodType(getattr(Model, name), mod))
    return mod


def _pop(n=60, L=30, seed=8, land=None, move_surf=1):
    D, x, y, e, z = small_sample(n, L, seed)
    rng = np.random.RandomState(seed + 100)
    x, y = rng.uniform(0, W_, n), rng.uniform(0, H_, n)
    # nobody stands on the wall (a cell of the wall is at inf from everything)
    x[np.floor(x) == 6] += 1.0
    x[:2], y[:2] = [3.2, 3.9], [4.5, 4.1]                     # two individuals on one cell
    ids = rng.permutation(n) * 3 + 1                          # slot order is not id order
    return _Species(D, x, y, e, z, ids, land or _land(), move_surf), D, x, y, e, z, ids


def test_calc_cost_distances_solves_the_distinct_cells_and_expands():
    spp, D, x, y, e, z, ids = _pop()
    mod = _model(spp)
    res = mod.calc_cost_distances()
    o = np.argsort(ids)
    cells = np.int32(np.floor(np.column_stack([x, y])))[o]
    np.testing.assert_array_equal(res['ids'], ids[o])
    np.testing.assert_array_equal(res['cells'], cells)
    R = K.resistance_raster(spp._land_ref[1].rast)            # the move_surf's layer, inverted
    lin = cells[:, 1] * W_ + cells[:, 0]
    what, R_got, res_got, cells_got = spp._dev.calls[-1]
    assert what == 'cost_matrix' and res_got == (1.0, 1.5)
    np.testing.assert_array_equal(R_got, R)
    np.testing.assert_array_equal(cells_got, np.unique(lin))  # distinct, each once
    assert np.unique(lin).size < lin.size
    surf = K.numpy_cost_surfaces(R, (1.0, 1.5), lin).reshape(lin.size, -1)
    want = surf[:, lin]
    assert res['dist'].shape == (60, 60) and res['dist'].dtype == np.float64
    assert (res['dist'] == res['dist'].T).all() and np.isfinite(res['dist']).all()
    assert np.abs(res['dist'] - want).max() <= H_ * W_ * 2.0 ** -52 * want.max()
    a, b = np.flatnonzero(np.isin(ids[o], ids[:2]))           # the two on one cell
    assert res['dist'][a, b] == 0 and lin[a] == lin[b]
    # the other sources of R, the selections and the sample of n
    flat = mod.calc_cost_distances(lyr='flat', kind='resistance', individs=ids[:7])
    assert flat['dist'].shape == (7, 7)
    np.testing.assert_array_equal(spp._dev.calls[-1][1], np.ones((H_, W_)))
    shut = mod.calc_cost_distances(lyr=1, barrier=0.5, n=12)
    assert shut['ids'].size == 12
    assert np.isinf(spp._dev.calls[-1][1]).sum() == (spp._land_ref[1].rast <= 0.5).sum()
    c = np.full((H_, W_), 2.0)
    c[0, 0] = np.nan
    mod.calc_cost_distances(cost=c, lyr=5)                    # cost overrides lyr
    assert spp._dev.calls[-1][1][0, 0] == INF and spp._dev.calls[-1][1][1, 1] == 2.0
    for kw, match in ((dict(cost=np.ones((H_, W_ + 1))), 'shape'), (dict(lyr=2), 'lyr'),
                      (dict(lyr='sea'), 'lyr'), (dict(kind='friction'), 'kind'),
                      (dict(individs=ids[:5], n=3), 'not both')):
        with pytest.raises(ValueError, match=match):
            mod.calc_cost_distances(**kw)


def test_the_move_surf_is_the_default_layer_and_its_absence_an_error():
    spp = _pop(move_surf='cond')[0]
    _model(spp).calc_cost_distances(individs=spp.ids[:4])
    np.testing.assert_array_equal(spp._dev.calls[-1][1], K.resistance_raster(spp._land_ref[1].rast))
    none = _pop(move_surf=None)[0]
    mod = _model(none)
    for call in (lambda: mod.calc_cost_distances(), lambda: mod.calc_cost_surface(1.0, 1.0),
                 lambda: mod.run_mmrr(predictors=('geo', 'cost'), nperm=5),
                 lambda: mod.run_mantel('cost', nperm=5)):
        with pytest.raises(ValueError, match=r'no move_surf.*lyr=.*cost='):
            call()
    mod.calc_cost_distances(lyr=1)                            # said, it is fine
    mod.run_mantel(('cost', dict(cost=np.ones((H_, W_)))), nperm=5, seed=1)


def test_calc_cost_surface_floors_the_points_to_cells():
    spp = _pop()[0]
    mod = _model(spp)
    one = mod.calc_cost_surface(3.7, 2.2)
    what, R, res, src = spp._dev.calls[-1]
    assert what == 'cost_surfaces' and res == (1.0, 1.5) and src.tolist() == [2 * W_ + 3]
    assert one.shape == (1, H_, W_) and one[0, 2, 3] == 0 and one.dtype == np.float64
    some = mod.calc_cost_surface([0.0, 11.99], np.array([8.99, 0.0]), lyr=0, kind='resistance')
    assert spp._dev.calls[-1][3].tolist() == [8 * W_, 11] and some.shape == (2, H_, W_)
    np.testing.assert_array_equal(some, K.numpy_cost_surfaces(np.ones((H_, W_)), (1, 1.5),
                                                              [8 * W_, 11]))
    for px, py in ((-0.1, 1), (12.0, 1), (1, 9.0), (1, -1e-9), (np.nan, 1), ([1, 2], [1])):
        with pytest.raises(ValueError, match='outside the landscape|not finite|as many'):
            mod.calc_cost_surface(px, py)


def _host_matrices(spp, D, x, y, e, ids):
    o = np.argsort(ids)
    cells = np.int32(np.floor(np.column_stack([x, y])))[o]
    lin = cells[:, 1] * W_ + cells[:, 0]
    cost = K.numpy_cost_surfaces(K.resistance_raster(spp._land_ref[1].rast), (1, 1.5), lin) \
        .reshape(lin.size, -1)[:, lin]
    cost = np.triu(cost) + np.triu(cost, 1).T
    flat = K.numpy_cost_surfaces(np.ones((H_, W_)), (1, 1.5), lin).reshape(lin.size, -1)[:, lin]
    flat = np.triu(flat) + np.triu(flat, 1).T
    return dict(Y=M.genetic_distances(D[o]), geo=M.euclid(np.column_stack([x, y])[o]),
                env=M.euclid(e[o, 1]), cost=cost, flat=flat)


def test_cost_predictors_are_parsed_and_put_back_in_the_callers_order():
    spp, D, x, y, e, z, ids = _pop()
    mod = _model(spp)
    m = _host_matrices(spp, D, x, y, e, ids)
    rows = M.draw_row_shuffles(60, 49, seed=3)
    order = ['cost', 'geo', 'flat', 'env']
    res = mod.run_mmrr(predictors=('cost', 'geo', ('cost', dict(lyr=0, kind='resistance',
                                                                 name='flat')), 'env'),
                       nperm=49, seed=3)
    Xs = [m[k] for k in order]
    sums, mom = M.numpy_perm_sums(m['Y'], Xs, rows), M.numpy_moments(m['Y'], Xs)
    ref = M.mmrr(sums, mom, order)
    assert list(res) == list(ref)
    assert [k for k in res if k.endswith('(p)')][1:] == [k + '(p)' for k in order]
    for k in ref:
        assert abs(res[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), k
    what, cols, mats, perm, slots = spp._dev.calls[-1]
    assert what == 'mat' and cols == [[(F_X, 0), (F_Y, 0)], [(F_E, 1)]]     # columns first,
    assert mats.shape == (2, 60, 60)                                        # then the matrices
    assert np.abs(mats[0] - m['cost']).max() <= 108 * 2.0 ** -52 * m['cost'].max()
    assert np.abs(mats[1] - m['flat']).max() <= 108 * 2.0 ** -52 * m['flat'].max()
    np.testing.assert_array_equal(perm, M.invert_rows(rows))
    np.testing.assert_array_equal(slots, np.argsort(ids))
    # without a cost predictor the old entry is called, as ever
    mod.run_mmrr(nperm=5, seed=1)
    assert spp._dev.calls[-1][0] == 'cols'
    # one predictor, given as a name or as a tuple; Mantel's x and given take the same forms
    only = mod.run_mmrr(predictors='cost', nperm=9, seed=1)
    assert list(only)[2] == 'cost' and spp._dev.calls[-1][1] == []
    named = mod.run_mmrr(predictors=('cost', dict(name='ibr')), nperm=9, seed=1)
    assert list(named)[2] == 'ibr' and named['ibr'] == only['cost']
    for x_, given, a, b in (('cost', None, 'cost', None), ('cost', 'geo', 'cost', 'geo'),
                            ('env', ('cost', dict(lyr=0, kind='resistance')), 'env', 'flat'),
                            (('cost', dict(name='a')), ('cost', dict(lyr='flat', name='b',
                                                                     kind='resistance')),
                             'cost', 'flat')):
        got = mod.run_mantel(x_, given=given, nperm=49, seed=3)
        Xs = [m[a]] + ([] if b is None else [m[b]])
        ref = M.mantel(M.numpy_perm_sums(m['Y'], Xs, rows), M.numpy_moments(m['Y'], Xs), 0,
                       None if b is None else 1)
        assert abs(got['r'] - ref['r']) <= 1e-12 and got['p'] == ref['p']
        assert np.abs(got['perm_r'] - ref['perm_r']).max() <= 1e-12


def test_cost_predictor_rules():
    spp, D, x, y, e, z, ids = _pop()
    mod = _model(spp)
    with pytest.raises(ValueError, match='listed twice'):
        mod.run_mmrr(predictors=('cost', 'geo', 'cost'), nperm=5)
    with pytest.raises(ValueError, match='listed twice'):
        mod.run_mmrr(predictors=(('cost', dict(lyr=0)), ('cost', dict(lyr=1))), nperm=5)
    with pytest.raises(ValueError, match='listed twice'):
        mod.run_mantel('cost', given=('cost', dict(lyr=0)), nperm=5)
    with pytest.raises(ValueError, match='listed twice'):
        mod.run_mmrr(predictors=('geo', ('cost', dict(name='geo'))), nperm=5)
    mod.run_mmrr(predictors=(('cost', dict(lyr=0, kind='resistance', name='a')),
                             ('cost', dict(lyr=1, name='b'))), nperm=5, seed=1)
    with pytest.raises(ValueError, match="unknown predictor 'gen'"):
        mod.run_mmrr(predictors=('cost', 'gen'), nperm=5)
    with pytest.raises(ValueError, match='unknown predictor'):
        mod.run_mantel('cost', given='resistance', nperm=5)
    with pytest.raises(ValueError, match="unknown predictor .*'cost'"):
        mod.run_mantel('elevation', nperm=5)
    with pytest.raises(ValueError, match="'cost' predictor takes .*not layer"):
        mod.run_mmrr(predictors=(('cost', dict(layer=0)),), nperm=5)
    with pytest.raises(ValueError, match='at most 4 predictors'):
        mod.run_mmrr(predictors=('geo', 'env', 'phn', 'cost', ('cost', dict(name='b'))), nperm=5)
    with pytest.raises(ValueError, match='no predictors'):
        mod.run_mmrr(predictors=(), nperm=5)
    with pytest.raises(ValueError, match='kind'):
        mod.run_mmrr(predictors=(('cost', dict(kind='friction')),), nperm=5)
    # degrees of freedom count the cost predictors too
    with pytest.raises(ValueError, match='degrees of freedom'):
        mod.run_mmrr(predictors=('geo', 'cost'), individs=np.sort(ids)[:3], nperm=5)
    big = _Species(np.zeros((8193, 4), np.int64), np.ones(8193), np.ones(8193),
                   np.zeros((8193, 2)), np.zeros((8193, 1)), np.arange(8193), _land())
    for call in (lambda: _model(big).run_mmrr(predictors=('cost',), nperm=5),
                 lambda: _model(big).run_mantel('cost', nperm=5),
                 lambda: _model(big).calc_cost_distances()):
        with pytest.raises(ValueError, match='at most 8192 individuals.*n='):
            call()
    assert not big._dev.calls


def test_a_pair_at_infinite_cost_is_refused_with_its_number():
    land = _land()
    land[1].rast[:, 6] = 0.0                                  # the wall closes: two halves
    spp, D, x, y, e, z, ids = _pop(land=land)
    mod = _model(spp)
    west = int((np.floor(x) < 6).sum())
    assert 0 < west < 60
    res = mod.calc_cost_distances()                           # the matrix itself says inf
    assert np.isinf(res['dist']).sum() == 2 * west * (60 - west)
    for call in (lambda: mod.run_mmrr(predictors=('geo', 'cost'), nperm=5),
                 lambda: mod.run_mantel('geo', given='cost', nperm=5)):
        with pytest.raises(ValueError, match=r"'cost': %d pairs .*infinite cost"
                           % (west * (60 - west))):
            call()
    assert all(c[0] != 'mat' for c in spp._dev.calls)         # nothing reached the test
    mod.run_mmrr(predictors=('geo', ('cost', dict(lyr=0, kind='resistance'))), nperm=5, seed=1)
    mod.run_mmrr(predictors=('geo', 'cost'), individs=ids[np.floor(x) < 6], nperm=5, seed=1)


def test_mmrr_on_a_euclidean_and_a_cost_matrix_is_a_refit_per_permutation():
    """numpy_perm_sums / numpy_moments take matrices of any origin: an MMRR on [euclid, cost]
    from them against a per-permutation lstsq fit on explicitly permuted matrices"""
    spp, D, x, y, e, z, ids = _pop(n=40)
    m = _host_matrices(spp, D, x, y, e, ids)
    Y, Xs = m['Y'], [m['geo'], m['cost']]
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
    res = M.mmrr(S_all[1:], mom, ['geo', 'cost'])
    assert smallest_gap(S_all[1:], mom) > GAP
    t = np.array([f[1] for f in fits])
    tp = (1 + (np.abs(t[1:]) >= np.abs(t[0])).sum(axis=0)) / 61
    for k, name in enumerate(['Intercept', 'geo', 'cost']):
        assert res[name + '(p)'] == tp[k]
        assert abs(res[name] - fits[0][0][k]) <= BAR * np.abs(fits[0][0]).max()


def test_the_new_calls_have_the_documented_signatures():
    from geonomics_amd.sim.model import Model
    sig = inspect.signature(Model.calc_cost_distances)
    assert list(sig.parameters) == ['self', 'spp', 'lyr', 'kind', 'barrier', 'cost', 'individs',
                                    'n']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['spp'], d['kind']) == (0, 'conductance')
    assert all(d[k] is None for k in ('lyr', 'barrier', 'cost', 'individs', 'n'))
    sig = inspect.signature(Model.calc_cost_surface)
    assert list(sig.parameters) == ['self', 'x', 'y', 'spp', 'lyr', 'kind', 'barrier', 'cost']


def test_a_tiled_species_refuses():
    from geonomics_amd.structs.tiled import TiledSpecies
    for name in ('_calc_cost_distances', '_calc_cost_surface', '_run_mmrr', '_run_mantel'):
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            getattr(TiledSpecies, name)(object(), predictors=('geo', 'cost'))


def test_the_binding_exports_the_new_entry_points():
    from geonomics_amd import _native as nat
    for name in ('gnx_cost_surfaces', 'gnx_cost_matrix', 'gnx_cost_budget', 'gnx_cost_info',
                 'gnx_dist_perm_sums_mat'):
        assert name in nat.EXPORTS
    for name in ('cost_surfaces', 'cost_matrix', 'cost_budget', 'cost_info',
                 'dist_perm_sums_mat'):
        assert callable(getattr(nat.Device, name))
