"""Circuit-theory resistance distances and current maps on the CPU (geonomics_amd/sim/circuit.py,
Species._calc_resistance_distances / _calc_current_map, the 'circuit' entries of run_mmrr /
run_mantel), with numpy in place of the device.

The restatement (per component one grounded node and scipy's splu) against circuits worked out
by hand - the series chain, Foster's theorem, the metric properties and Rayleigh's bound by the
least-cost distance, the components, the unit current of a 1-wide corridor - and the public
calls on the stand-in Species of test_cost_host.py whose device is the restatement."""
import inspect
import types

import numpy as np
import pytest

from geonomics_amd.sim import circuit as Q
from geonomics_amd.sim import cost as K
from geonomics_amd.sim import mmrr as M
import test_cost_host as TC
from test_cost_host import F_E, F_X, F_Y, H_, W_

INF = np.inf
EPS = 2.0 ** -52


# ------------------------------------------------------------------ the restatement
def test_a_series_chain_adds_its_resistors():
    for r in (1.0, 0.3, 7.5):
        want = 2.0 * r * np.arange(9)
        got = Q.numpy_resistance_matrix(np.full((1, 9), r), (2.0, 5.0), np.arange(9))
        assert np.abs(got[0] - want).max() <= 8 * EPS * want.max()
        want = 0.7 * r * np.arange(9)
        got = Q.numpy_resistance_matrix(np.full((9, 1), r), (5.0, 0.7), np.arange(9))
        assert np.abs(got[0] - want).max() <= 8 * EPS * want.max()
        np.testing.assert_array_equal(got, got.T)


def _random_raster(H, W, seed, shut=()):
    R = 1.0 / np.maximum(np.random.RandomState(seed).rand(H, W), 0.05)
    for y, x in shut:
        R[y, x] = INF
    return R


def test_fosters_theorem():
    """sum over the edges of g_uv reff(u, v) = (cells of the component) - 1"""
    R = _random_raster(6, 7, 3, shut=((2, 3), (4, 1)))
    for res in ((1.0, 1.0), (2.0, 0.5)):
        D = Q.numpy_resistance_matrix(R, res, np.arange(42))
        L = Q.laplacian(R, res).tocoo()
        up = L.row < L.col
        total = (-L.data[up] * D[L.row[up], L.col[up]]).sum()
        assert abs(total - 39) <= 1e-11, total
        assert (np.asarray(abs(L).sum(axis=1)).ravel()[[2 * 7 + 3, 4 * 7 + 1]] == 0).all()
        assert np.abs(np.asarray(L.sum(axis=1))).max() <= 64 * EPS * L.data.max()


def test_metric_properties_and_the_least_cost_bound():
    R = _random_raster(12, 9, 4)
    R[:, 4] = INF
    R[5, 4] = 1.5                                            # a 1-wide door in a wall ...
    R[0:11, 7] = INF                                         # ... and a 1-wide dead-end corridor
    R[0:11, 6] = INF
    res = (1.0, 1.5)
    cells = np.arange(108)
    D = Q.numpy_resistance_matrix(R, res, cells)
    C = K.numpy_cost_matrix(R, res, cells)
    np.testing.assert_array_equal(D, D.T)
    np.testing.assert_array_equal(np.isinf(D), np.isinf(C))
    ok = np.isfinite(D)
    assert (D[ok] >= 0).all() and (np.diag(D) == 0).all()
    big = np.where(ok, D, 0.0)
    tri = big[:, :, None] + big[None, :, :]                  # d(a, b) + d(b, c) over b
    fin = ok[:, :, None] & ok[None, :, :]
    worst = np.where(fin, tri, INF).min(axis=1)
    assert (big <= worst + 1e-10)[ok].all()
    # every further route lowers the resistance: never above the cheapest path
    assert (D[ok] <= C[ok] * (1 + 1e-12)).all()
    assert (D[ok] < 0.9 * C[ok])[(C > 6)[ok]].any()
    # along the corridor of column 8 (rows 0..10: cells (y, 8)) there is one route only
    col = np.arange(0, 10) * 9 + 8
    for a in col:
        for b in col:
            assert abs(D[a, b] - C[a, b]) <= 1e-12 * max(C[a, b], 1.0)


def test_components():
    R = np.full((6, 8), 2.0)
    R[:, 3] = INF                                            # a wall with no gap
    R[1:4, 5:8] = INF
    R[2, 6] = 1.0                                            # an isolated passable pocket cell
    cells = np.array([0, 8 + 1, 3, 4, 5 * 8 + 7, 2 * 8 + 6, 2 * 8 + 5])
    D = Q.numpy_resistance_matrix(R, (1, 1), cells)
    lab = Q.components(R)
    assert lab[0, 0] == 0 and lab[5, 2] == 0 and lab[0, 4] == 4 and lab[5, 7] == 4
    assert lab[2, 6] == 2 * 8 + 6 and (lab[:, 3] == -1).all() and lab.dtype == np.int64
    assert np.isfinite(D[0, 1]) and np.isfinite(D[3, 4]) and D[0, 1] > 0
    assert np.isinf(D[:2, 3:]).all() and np.isinf(D[3:, :2]).all()          # across the wall
    for k in (2, 5, 6):                                      # on the wall; the pocket; a barrier
        assert D[k, k] == 0 and np.isinf(np.delete(D[k], k)).all()
    x, anchor = Q.numpy_potentials(R, (1, 1), cells)
    assert anchor.tolist() == [0, 0, -1, 3, 3, 5, -1]
    assert (x[[0, 2, 3, 5, 6]] == 0).all()
    L = Q.laplacian(R, (1, 1))
    b = np.zeros(48)
    b[cells[1]], b[cells[0]] = 1.0, -1.0
    assert np.abs(L @ x[1].ravel() - b).max() <= 1e-13
    assert x[1].ravel()[cells[0]] == 0 and abs(x[1].ravel()[cells[1]] - D[0, 1]) <= 1e-13
    with pytest.raises(ValueError, match='listed twice'):
        Q.numpy_resistance_matrix(R, (1, 1), [1, 2, 1])
    with pytest.raises(ValueError, match='cells in 0..47'):
        Q.numpy_current_map(R, (1, 1), [48])
    with pytest.raises(ValueError, match='every entry > 0'):
        Q.numpy_potentials(-R, (1, 1), [1])


def test_the_current_of_a_corridor():
    R = np.full((5, 9), INF)
    R[2, :] = np.linspace(1, 3, 9)                           # a 1-wide corridor along row 2
    R[0, 0] = 1.0                                            # a cell of its own
    cur, used, skipped = Q.numpy_current_map(R, (1, 1), [2 * 9 + 1, 2 * 9 + 6])
    want = np.zeros((5, 9))
    want[2, 1:7] = 1.0
    assert np.abs(cur - want).max() <= 8 * EPS and (used, skipped) == (1, 0)
    assert (cur[~np.isfinite(R)] == 0).all() and cur[0, 0] == 0 and abs(cur[2, 7]) <= 8 * EPS
    # three cells: the pairs (1, 6), (1, 4), (4, 6); one across the wall, one on it
    cur, used, skipped = Q.numpy_current_map(R, (1, 1), [2 * 9 + 1, 2 * 9 + 6, 2 * 9 + 4, 0, 9])
    want = np.zeros((5, 9))
    want[2, 1:7] += 1.0
    want[2, 1:5] += 1.0
    want[2, 4:7] += 1.0
    assert np.abs(cur - want).max() <= 16 * EPS and (used, skipped) == (3, 7)
    # two routes share the ampere
    R = np.full((3, 3), 1.0)
    R[1, 1] = INF
    cur, _, _ = Q.numpy_current_map(R, (1, 1), [3, 5])
    assert abs(cur[1, 0] - 1) <= 4 * EPS and abs(cur[1, 2] - 1) <= 4 * EPS
    assert abs(cur[0, 1] - 0.5) <= 4 * EPS and abs(cur[2, 1] - 0.5) <= 4 * EPS and cur[1, 1] == 0


# ------------------------------------------------------------------ the model layer
class _Dev(TC._Dev):
    """test_cost_host's numpy device with the circuit calls restated"""

    def circuit_matrix(self, R, res, cells, tol=None, max_iter=None):
        self.calls.append(('circuit_matrix', R.copy(), tuple(res), np.array(cells), tol, max_iter))
        return Q.numpy_resistance_matrix(R, res, cells)

    def circuit_current(self, R, res, cells, tol=None, max_iter=None):
        self.calls.append(('circuit_current', R.copy(), tuple(res), np.array(cells), tol,
                           max_iter))
        return Q.numpy_current_map(R, res, cells)

    def circuit_info(self):
        return dict(kernel_ms=0.0, launches=0, iterations=0, restarts=0, worst_residual=0.0)


def _pop(**kw):
    out = TC._pop(**kw)
    spp = out[0]
    old = spp._dev
    spp._dev = _Dev(old.D, old.x, old.y, old.e, old.z)
    return out


def _model(spp):
    from geonomics_amd.sim.model import Model
    mod = TC._model(spp)
    for name in ('calc_resistance_distances', 'calc_current_map'):
        setattr(mod, name, types.MethodType(getattr(Model, name), mod))
    return mod


def test_calc_resistance_distances_solves_the_distinct_cells_and_expands():
    spp, D, x, y, e, z, ids = _pop()
    mod = _model(spp)
    res = mod.calc_resistance_distances(tol=1e-9, max_iter=500)
    o = np.argsort(ids)
    cells = np.int32(np.floor(np.column_stack([x, y])))[o]
    np.testing.assert_array_equal(res['ids'], ids[o])
    np.testing.assert_array_equal(res['cells'], cells)
    assert sorted(res) == ['cells', 'dist', 'ids', 'info']
    assert sorted(res['info']) == ['iterations', 'kernel_ms', 'launches', 'restarts',
                                   'worst_residual']
    R = K.resistance_raster(spp._land_ref[1].rast)
    lin = cells[:, 1] * W_ + cells[:, 0]
    what, R_got, res_got, cells_got, tol, max_iter = spp._dev.calls[-1]
    assert what == 'circuit_matrix' and res_got == (1.0, 1.5) and (tol, max_iter) == (1e-9, 500)
    np.testing.assert_array_equal(R_got, R)
    np.testing.assert_array_equal(cells_got, np.unique(lin))
    uniq, inv = np.unique(lin, return_inverse=True)
    np.testing.assert_array_equal(res['dist'],
                                  Q.numpy_resistance_matrix(R, (1.0, 1.5), uniq)[inv][:, inv])
    a, b = np.flatnonzero(np.isin(ids[o], ids[:2]))           # the two on one cell
    assert res['dist'][a, b] == 0 and lin[a] == lin[b]
    assert (res['dist'] == res['dist'].T).all() and np.isfinite(res['dist']).all()
    mod.calc_resistance_distances(lyr='flat', kind='resistance', n=12)
    assert spp._dev.calls[-1][4:] == (None, None) and spp._dev.calls[-1][3].size <= 12
    np.testing.assert_array_equal(spp._dev.calls[-1][1], np.ones((H_, W_)))
    for kw, match in ((dict(tol=0.0), 'tol'), (dict(tol=np.nan), 'tol'),
                      (dict(max_iter=0), 'max_iter'), (dict(max_iter=2.5), 'max_iter'),
                      (dict(lyr=2), 'lyr'), (dict(kind='friction'), 'kind'),
                      (dict(individs=ids[:5], n=3), 'not both')):
        with pytest.raises(ValueError, match=match):
            mod.calc_resistance_distances(**kw)
    none = _pop(move_surf=None)[0]
    with pytest.raises(ValueError, match=r'no move_surf.*lyr=.*cost='):
        _model(none).calc_resistance_distances()
    with pytest.raises(ValueError, match=r'no move_surf.*lyr=.*cost='):
        _model(none).run_mantel('circuit', nperm=5)


def test_calc_current_map_floors_the_points_and_counts_the_pairs():
    spp, D, x, y, e, z, ids = _pop()
    mod = _model(spp)
    res = mod.calc_current_map([3.7, 9.2, 3.1], [2.2, 7.5, 2.9])
    what, R, rs, cells, tol, max_iter = spp._dev.calls[-1]
    assert what == 'circuit_current' and rs == (1.0, 1.5)
    assert cells.tolist() == [2 * W_ + 3, 7 * W_ + 9]         # distinct, ascending
    assert res['cells'].tolist() == cells.tolist() and res['n_pairs'] == 1
    assert res['n_skipped'] == 0 and res['current'].shape == (H_, W_)
    assert abs(res['current'][2, 3] - 1) <= 1e-12 and abs(res['current'][7, 9] - 1) <= 1e-12
    assert sorted(res) == ['cells', 'current', 'n_pairs', 'n_skipped']
    ind = mod.calc_current_map(individs=ids[:6], lyr=0, kind='resistance', tol=1e-8)
    o = np.argsort(ids[:6])
    c6 = np.int64(np.floor(np.column_stack([x, y])))[:6][o]
    assert ind['cells'].tolist() == np.unique(c6[:, 1] * W_ + c6[:, 0]).tolist()
    assert spp._dev.calls[-1][4] == 1e-8
    m = ind['cells'].size
    assert ind['n_pairs'] == m * (m - 1) // 2
    for args, kw, match in (((-0.1, 1), {}, 'outside the landscape'),
                            ((1, 9.0), {}, 'outside the landscape'),
                            ((np.nan, 1), {}, 'not finite'), (([1, 2], [1]), {}, 'as many'),
                            ((1.0,), {}, 'x and y'), ((1.0, 1.0), dict(individs=ids[:3]),
                                                      'not both'),
                            ((1.0, 1.0), dict(n=3), 'not both'),
                            ((), dict(tol=-1.0), 'tol'), ((), dict(max_iter=0), 'max_iter')):
        with pytest.raises(ValueError, match=match):
            mod.calc_current_map(*args, **kw)
    spp._land_dim = (20, 20)                                  # room for more than 128 cells
    gx, gy = np.meshgrid(np.arange(20) + 0.5, np.arange(7) + 0.25)
    with pytest.raises(ValueError, match='at most 128 distinct cells.*got 140'):
        mod.calc_current_map(gx.ravel(), gy.ravel())
    assert spp._dev.calls[-1][4] == 1e-8                      # nothing reached the device


def _host_matrices(spp, D, x, y, e, ids):
    m = TC._host_matrices(spp, D, x, y, e, ids)
    o = np.argsort(ids)
    cells = np.int32(np.floor(np.column_stack([x, y])))[o]
    lin = cells[:, 1] * W_ + cells[:, 0]
    uniq, inv = np.unique(lin, return_inverse=True)
    R = K.resistance_raster(spp._land_ref[1].rast)
    m['circuit'] = Q.numpy_resistance_matrix(R, (1, 1.5), uniq)[inv][:, inv]
    m['flatc'] = Q.numpy_resistance_matrix(np.ones((H_, W_)), (1, 1.5), uniq)[inv][:, inv]
    return m


def test_circuit_predictors_reach_the_matrix_entry_in_the_callers_order():
    spp, D, x, y, e, z, ids = _pop()
    mod = _model(spp)
    m = _host_matrices(spp, D, x, y, e, ids)
    rows = M.draw_row_shuffles(60, 49, seed=3)
    order = ['circuit', 'geo', 'cost', 'flatc']
    res = mod.run_mmrr(predictors=('circuit', 'geo', 'cost',
                                   ('circuit', dict(lyr=0, kind='resistance', name='flatc',
                                                    tol=1e-9, max_iter=900))),
                       nperm=49, seed=3)
    Xs = [m[k] for k in order]
    ref = M.mmrr(M.numpy_perm_sums(m['Y'], Xs, rows), M.numpy_moments(m['Y'], Xs), order)
    assert list(res) == list(ref)
    assert [k for k in res if k.endswith('(p)')][1:] == [k + '(p)' for k in order]
    for k in ref:
        assert abs(res[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), k
    what, cols, mats, perm, slots = spp._dev.calls[-1]
    assert what == 'mat' and cols == [[(F_X, 0), (F_Y, 0)]]     # the columns first, then the
    assert mats.shape == (3, 60, 60)                            # matrices in the caller's order
    np.testing.assert_array_equal(mats[0], m['circuit'])
    np.testing.assert_array_equal(mats[2], m['flatc'])
    assert np.abs(mats[1] - m['cost']).max() <= 108 * EPS * m['cost'].max()
    solves = [c for c in spp._dev.calls if c[0] in ('circuit_matrix', 'cost_matrix')][-3:]
    assert [c[0] for c in solves] == ['circuit_matrix', 'cost_matrix', 'circuit_matrix']
    assert solves[0][4:] == (None, None) and solves[2][4:] == (1e-9, 900)
    only = mod.run_mmrr(predictors='circuit', nperm=9, seed=1)
    assert list(only)[2] == 'circuit' and spp._dev.calls[-1][1] == []
    named = mod.run_mmrr(predictors=('circuit', dict(name='ibr')), nperm=9, seed=1)
    assert list(named)[2] == 'ibr' and named['ibr'] == only['circuit']
    for x_, given, a, b in (('circuit', None, 'circuit', None), ('circuit', 'geo', 'circuit', 'geo'),
                            ('cost', ('circuit', dict(lyr=0, kind='resistance')), 'cost', 'flatc'),
                            ('env', 'circuit', 'env', 'circuit')):
        got = mod.run_mantel(x_, given=given, nperm=49, seed=3)
        Xs = [m[a]] + ([] if b is None else [m[b]])
        ref = M.mantel(M.numpy_perm_sums(m['Y'], Xs, rows), M.numpy_moments(m['Y'], Xs), 0,
                       None if b is None else 1)
        assert abs(got['r'] - ref['r']) <= 1e-12 and got['p'] == ref['p']
        assert np.abs(got['perm_r'] - ref['perm_r']).max() <= 1e-12


def test_circuit_predictor_rules():
    spp, D, x, y, e, z, ids = _pop()
    mod = _model(spp)
    with pytest.raises(ValueError, match='listed twice'):
        mod.run_mmrr(predictors=('circuit', 'geo', 'circuit'), nperm=5)
    with pytest.raises(ValueError, match='listed twice'):
        mod.run_mmrr(predictors=('cost', ('circuit', dict(name='cost'))), nperm=5)
    mod.run_mmrr(predictors=('cost', 'circuit'), nperm=5, seed=1)      # two kinds, two names
    with pytest.raises(ValueError, match="'circuit' predictor takes .*tol, max_iter.*not layer"):
        mod.run_mmrr(predictors=(('circuit', dict(layer=0)),), nperm=5)
    with pytest.raises(ValueError, match="'cost' predictor takes .*not tol"):
        mod.run_mmrr(predictors=(('cost', dict(tol=1e-9)),), nperm=5)
    with pytest.raises(ValueError, match="unknown predictor .*'cost' or 'circuit'"):
        mod.run_mantel('circuit', given='resistance', nperm=5)
    with pytest.raises(ValueError, match='at most 4 predictors'):
        mod.run_mmrr(predictors=('geo', 'env', 'phn', 'cost', 'circuit'), nperm=5)
    with pytest.raises(ValueError, match='kind'):
        mod.run_mmrr(predictors=(('circuit', dict(kind='friction')),), nperm=5)
    with pytest.raises(ValueError, match='degrees of freedom'):
        mod.run_mmrr(predictors=('geo', 'circuit'), individs=np.sort(ids)[:3], nperm=5)
    big = TC._Species(np.zeros((8193, 4), np.int64), np.ones(8193), np.ones(8193),
                      np.zeros((8193, 2)), np.zeros((8193, 1)), np.arange(8193), TC._land())
    for call in (lambda: _model(big).run_mmrr(predictors=('circuit',), nperm=5),
                 lambda: _model(big).calc_resistance_distances()):
        with pytest.raises(ValueError, match='at most 8192 individuals.*n='):
            call()
    assert not big._dev.calls


def test_a_pair_at_infinite_resistance_is_refused_with_its_number():
    land = TC._land()
    land[1].rast[:, 6] = 0.0                                  # the wall closes: two halves
    spp, D, x, y, e, z, ids = _pop(land=land)
    mod = _model(spp)
    west = int((np.floor(x) < 6).sum())
    res = mod.calc_resistance_distances()
    assert np.isinf(res['dist']).sum() == 2 * west * (60 - west)
    for call in (lambda: mod.run_mmrr(predictors=('geo', 'circuit'), nperm=5),
                 lambda: mod.run_mantel('geo', given='circuit', nperm=5)):
        with pytest.raises(ValueError, match=r"'circuit': %d pairs .*infinite cost"
                           % (west * (60 - west))):
            call()
    assert all(c[0] != 'mat' for c in spp._dev.calls)
    cm = mod.calc_current_map(individs=ids[:8])
    w8 = np.unique(np.int64(np.floor(y[:8])) * W_ + np.int64(np.floor(x[:8])))
    nw = int((w8 % W_ < 6).sum())
    assert cm['n_skipped'] == nw * (w8.size - nw) and cm['n_pairs'] + cm['n_skipped'] == \
        w8.size * (w8.size - 1) // 2


def test_a_request_without_circuit_makes_the_calls_it_made():
    """the same device calls, with the same arguments, as the stand-in of test_cost_host.py
    records for them"""
    reqs = (lambda m: m.run_mmrr(nperm=9, seed=1),
            lambda m: m.run_mmrr(predictors=('cost', 'geo', 'env'), nperm=9, seed=1),
            lambda m: m.run_mantel('geo', given=('cost', dict(lyr=0, kind='resistance')),
                                   nperm=9, seed=1),
            lambda m: m.calc_cost_distances(n=7))
    for req in reqs:
        new, old = _pop()[0], TC._pop()[0]
        a, b = req(_model(new)), req(TC._model(old))
        assert len(new._dev.calls) == len(old._dev.calls) > 0
        for ca, cb in zip(new._dev.calls, old._dev.calls):
            assert ca[0] == cb[0] and len(ca) == len(cb)
            for va, vb in zip(ca[1:], cb[1:]):
                if isinstance(va, np.ndarray):
                    np.testing.assert_array_equal(va, vb)
                else:
                    assert va == vb
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])


def test_the_new_calls_have_the_documented_signatures():
    from geonomics_amd.sim.model import Model
    sig = inspect.signature(Model.calc_resistance_distances)
    assert list(sig.parameters) == ['self', 'spp', 'lyr', 'kind', 'barrier', 'cost', 'individs',
                                    'n', 'tol', 'max_iter']
    sig = inspect.signature(Model.calc_current_map)
    assert list(sig.parameters) == ['self', 'x', 'y', 'spp', 'individs', 'n', 'lyr', 'kind',
                                    'barrier', 'cost', 'tol', 'max_iter']


def test_a_tiled_species_refuses():
    from geonomics_amd.structs.tiled import TiledSpecies
    for name in ('_calc_resistance_distances', '_calc_current_map'):
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            getattr(TiledSpecies, name)(object(), lyr=0)


def test_the_binding_exports_the_new_entry_points():
    from geonomics_amd import _native as nat
    for name in ('gnx_circuit_matrix', 'gnx_circuit_current', 'gnx_circuit_potentials',
                 'gnx_circuit_budget', 'gnx_circuit_info'):
        assert name in nat.EXPORTS
    for name in ('circuit_matrix', 'circuit_current', 'circuit_potentials', 'circuit_budget',
                 'circuit_info'):
        assert callable(getattr(nat.Device, name))
