"""Circuit-theory resistance distances and current maps on the device (csrc/gnx_circuit.hip,
Model.calc_resistance_distances / calc_current_map and the 'circuit' predictor of run_mmrr /
run_mantel).  Needs an MI355X.

The yardstick is the host restatement (sim/circuit.py: every component grounded at one node,
the reduced Laplacian factorised with scipy's splu), never the device code.

The bound on an effective resistance is derived, not chosen.  The device stops a system
L x = b, b = e_i - e_a, at a true residual ||b - L x|| <= tol sqrt(2).  The error of x on the
component (mean removed) is L+ r, at most ||r|| / lambda_2 in norm, lambda_2 the smallest
non-zero eigenvalue of the component's Laplacian; reff reads two differences of two such
solutions, each difference (e_s - e_t)' L+ r being at most sqrt(2) ||r|| / lambda_2, hence

    |reff - ref| <= 4 tol / lambda_2  +  8 e_ref ref,

e_ref the restatement's own relative error, measured as its disagreement with a dense
pseudo-inverse on a raster small enough for both.  lambda_2 comes from scipy's eigsh in
shift-invert mode.  The current of a cell sums, over the P pairs used, conductance-weighted
differences of such potentials, |c - ref| <= 2 P G_u tol / lambda_2 + 16 P 2^-53 |ref| with G_u
the cell's Laplacian diagonal.  The residuals are formed on the host from laplacian() in
extended precision (the fp64 product diag x - G x would itself round at 1e-12 here).

Measured on an MI355X (e_ref = 4.7e-13 there): the serpentine raster (14 focal cells, 11 systems
in one batch, lambda_2 = 3.3e-5) took 704 CG iterations, 1422 launches and 28.4 ms of kernel
time with square cells, 736 iterations, 1486 launches and 28.0 ms with 2 x 0.5 cells, no restart.
The worst |reff - ref| was 1.1e-10, the worst error / bound 9.2e-6 (square) and 4.1e-6; the
current map's worst error 4.1e-10, 1.2e-6 of its bound.  The worst true residual was 1.396e-10
(square) and 1.407e-10 against the threshold 1.414e-10; the host's and gnx_circuit_info's
worst residuals agreed to 6e-5 relative.  The flat 64 x 64 and 65 x 129 rasters were at 1.4e-4
and 7.2e-5 of the bound, the chains at 3.6e-7; the 40 x 40 model (139 individuals on 133 cells,
192 iterations, 4.5 ms) at 2.0e-3, its statistics within 1.1e-12 of the largest entry of their
group, the smallest relative gap of a permuted statistic from the observed one 1.2e-3."""
import numpy as np
import pytest

from test_gpu_parity import native
from test_mmrr_host import BAR, GAP, smallest_gap
from geonomics_amd.sim import circuit as Q
from geonomics_amd.sim import cost as K
from geonomics_amd.sim import mmrr as M

pytestmark = pytest.mark.gpu

INF = np.inf
TOL = 1e-10
GEO = [(0, 0), (1, 0)]                  # (GNX_F_X, 0), (GNX_F_Y, 0)
RES = [(1.0, 1.0), (2.0, 0.5)]


def _device(nat, H, W):
    dev = nat.Device(W, H, 1)
    dev.upload_rasters(np.ones((1, H, W), np.float32))
    return dev


def serpentine(H=66, W=70, step=10, seed=5):
    """66 x 70 (2 x 2 ragged tiles of 64): R = 1 / max(U(0, 1), 0.05); impassable columns at
    x = 8, 18, ... with a gap of 3 cells at alternating ends, so that the current crosses the
    tile borders back and forth; a block of barrier cells with a passable 2 x 2 pocket inside.
    14 focal cells: the corners, the tile-corner cells on both sides of x = 63 / 64 and
    y = 63 / 64, four more along the tile borders, one in the pocket, one on a barrier"""
    R = 1.0 / np.maximum(np.random.RandomState(seed).rand(H, W), 0.05)
    for k, x in enumerate(range(8, W, step)):
        R[:, x] = INF
        if k % 2 == 0:
            R[:3, x] = 1.0 + k
        else:
            R[-3:, x] = 1.0 + k
    R[30:34, 40:44] = INF
    R[31:33, 41:43] = 2.0
    cells = [0, W - 1, (H - 1) * W, H * W - 1,               # the corners
             63 * W + 63, 63 * W + 64, 64 * W + 63, 64 * W + 64,     # the tiles' corners
             31 * W + 41,                                    # inside the pocket
             20 * W + 18,                                    # on a barrier cell
             5 * W + 63, 40 * W + 64, 63 * W + 5, 64 * W + 30]       # along the tile borders
    return R, np.array(cells, np.int32)


def lambda_2(R, res, label=None):
    """the smallest non-zero Laplacian eigenvalue of the component `label` (default: the
    largest one)"""
    from scipy.sparse import identity
    from scipy.sparse.linalg import eigsh
    lab = Q.components(R).ravel()
    if label is None:
        vals, counts = np.unique(lab[lab >= 0], return_counts=True)
        label = vals[np.argmax(counts)]
    nodes = np.flatnonzero(lab == label)
    L = Q.laplacian(R, res).tocsr()[nodes][:, nodes].tocsc()
    if nodes.size <= 400:
        w = np.linalg.eigvalsh(L.toarray())
    else:
        shift = 1e-9 * L.diagonal().max()
        w = np.sort(eigsh(L + shift * identity(nodes.size, format='csc'), k=3, sigma=0.0,
                          which='LM', return_eigenvectors=False)) - shift
    assert abs(w[0]) <= 1e-6 * w[1]                          # the constant vector, then lambda_2
    return float(w[1])


_REF = {}


def restatement_error():
    """the relative disagreement of the grounded splu solve with a dense pseudo-inverse, on a
    22 x 24 raster of the same build (every passable cell of the large component a focal cell
    would be 400 systems: a spread of 40)"""
    if 'e_ref' not in _REF:
        worst = 0.0
        for res in RES:
            R, _ = serpentine(22, 24, 6, seed=6)
            lab = Q.components(R).ravel()
            big = np.flatnonzero(lab == np.bincount(lab[lab >= 0]).argmax())[::9]
            got = Q.numpy_resistance_matrix(R, res, big)
            Lp = np.linalg.pinv(Q.laplacian(R, res).toarray(), hermitian=True)
            d = np.diag(Lp)[big]
            want = d[:, None] + d[None, :] - 2 * Lp[np.ix_(big, big)]
            off = ~np.eye(big.size, dtype=bool)
            worst = max(worst, float((np.abs(got - want)[off] / want[off]).max()))
        _REF['e_ref'] = worst
        print('restatement: splu against pinv, worst relative disagreement %.3g' % worst)
    return _REF['e_ref']


def _ref(what, res):
    """the restatement of the serpentine case, computed once"""
    key = (what, res)
    if key not in _REF:
        R, cells = serpentine()
        if what == 'matrix':
            _REF[key] = Q.numpy_resistance_matrix(R, res, cells)
        elif what == 'current':
            _REF[key] = Q.numpy_current_map(R, res, cells)
        elif what == 'lambda_2':
            _REF[key] = lambda_2(R, res)
        elif what == 'laplacian':
            _REF[key] = Q.laplacian(R, res).tocoo()
    return _REF[key]


@pytest.fixture(scope='module')
def snake():
    nat = native()
    R, cells = serpentine()
    dev = _device(nat, *R.shape)
    yield nat, dev, R, cells
    dev.close()


def _check_matrix(got, ref, lam2, label):
    assert got.shape == ref.shape and got.dtype == np.float64
    np.testing.assert_array_equal(np.isinf(got), np.isinf(ref))
    assert not np.isnan(got).any()
    assert (np.diag(got) == 0).all()
    np.testing.assert_array_equal(got, got.T)
    ok = np.isfinite(ref)
    bound = 4 * TOL / lam2 + 8 * restatement_error() * ref[ok]
    err = np.abs(got[ok] - ref[ok])
    worst = float((err / bound).max())
    print('%s: %d finite, %d inf, lambda_2 %.3g, worst |reff - ref| %.3g, worst error / bound '
          '%.3g' % (label, ok.sum(), (~ok).sum(), lam2, err.max(), worst))
    assert (err <= bound).all(), (label, worst)
    return worst


@pytest.mark.parametrize('res', RES, ids=['square', 'res_2_0.5'])
def test_the_matrix_on_the_serpentine_raster(snake, res):
    nat, dev, R, cells = snake
    got = dev.circuit_matrix(R, res, cells, TOL)
    info = dev.circuit_info()
    print('info %s: %s' % (res, info))
    ref = _ref('matrix', res)
    _check_matrix(got, ref, _ref('lambda_2', res), 'serpentine %s' % (res,))
    # the pocket and the barrier cell are at inf from everything, the other 12 from nothing else
    assert np.isinf(got[8]).sum() == 13 and np.isinf(got[9]).sum() == 13
    assert np.isinf(got).sum() == 2 * (13 + 12)
    assert info['iterations'] > 64 and info['launches'] >= 2 * info['iterations']
    assert info['kernel_ms'] > 0 and info['worst_residual'] <= TOL * np.sqrt(2)
    # a second call, and one system per batch, are the same bits
    again = dev.circuit_matrix(R, res, cells, TOL)
    np.testing.assert_array_equal(again, got)
    dev.circuit_budget(5 * R.size * 8)
    try:
        single = dev.circuit_matrix(R, res, cells, TOL)
        one = dev.circuit_info()
    finally:
        dev.circuit_budget(0)
    np.testing.assert_array_equal(single, got)
    assert one['iterations'] > info['iterations']            # summed over 11 batches of one


@pytest.mark.parametrize('res', RES, ids=['square', 'res_2_0.5'])
def test_the_residuals_of_the_potentials(snake, res):
    nat, dev, R, cells = snake
    x, anchor = dev.circuit_potentials(R, res, cells, TOL)
    info = dev.circuit_info()
    ref_anchor = np.array([0, 0, 0, 0, 0, 0, 0, 0, 8, -1, 0, 0, 0, 0])
    np.testing.assert_array_equal(anchor, ref_anchor)
    L = _ref('laplacian', res)
    data = L.data.astype(np.longdouble)
    worst = 0.0
    for i, a in enumerate(anchor):
        xi = x[i].ravel()
        if a < 0 or a == i:
            assert (xi == 0).all()
            continue
        r = np.zeros(R.size, np.longdouble)
        r[cells[i]] += 1
        r[cells[a]] -= 1
        np.subtract.at(r, L.row, data * xi[L.col].astype(np.longdouble))
        norm = float(np.sqrt((r * r).sum()))
        worst = max(worst, norm)
        assert norm <= TOL * np.sqrt(2), (i, norm)
        assert (xi[~np.isfinite(R.ravel())] == 0).all()
    print('residuals %s: worst on the host %.6g, gnx_circuit_info %.6g, threshold %.6g'
          % (res, worst, info['worst_residual'], TOL * np.sqrt(2)))
    assert abs(info['worst_residual'] - worst) <= 1e-3 * worst


@pytest.mark.parametrize('res', RES, ids=['square', 'res_2_0.5'])
def test_the_current_map(snake, res):
    nat, dev, R, cells = snake
    got, used, skipped = dev.circuit_current(R, res, cells, TOL)
    ref, ref_used, ref_skipped = _ref('current', res)
    assert (used, skipped) == (ref_used, ref_skipped) == (66, 25)
    assert got.shape == R.shape and (got[~np.isfinite(R)] == 0).all()
    assert (got[31:33, 41:43] == 0).all()                    # the pocket: one focal cell, no pair
    G = np.asarray(_ref('laplacian', res).tocsr().diagonal()).reshape(R.shape)
    bound = 2 * used * G * TOL / _ref('lambda_2', res) + 16 * used * 2.0 ** -53 * np.abs(ref)
    err = np.abs(got - ref)
    ok = bound > 0
    worst = float((err[ok] / bound[ok]).max())
    print('current %s: max %.6g, worst error %.3g, worst error / bound %.3g'
          % (res, ref.max(), err.max(), worst))
    assert (err <= bound).all(), worst
    again, _, _ = dev.circuit_current(R, res, cells, TOL)
    np.testing.assert_array_equal(again, got)


def test_refusals_leave_the_handle_usable(snake):
    nat, dev, R, cells = snake
    res = (1.0, 1.0)
    before = dev.circuit_matrix(R, res, cells[:6], TOL)
    bad_R = [R.copy() for _ in range(3)]
    bad_R[0][3, 3], bad_R[1][0, 0], bad_R[2][65, 69] = 0.0, np.nan, -1.0
    calls = [(lambda: dev.circuit_matrix(R, res, [0, -1], TOL), 'not a cell'),
             (lambda: dev.circuit_matrix(R, res, [0, R.size], TOL), 'not a cell'),
             (lambda: dev.circuit_matrix(R, res, [5, 9, 5], TOL), 'listed twice'),
             (lambda: dev.circuit_current(R, res, [5, 9, 5], TOL), 'listed twice'),
             (lambda: dev.circuit_potentials(R, res, [R.size], TOL), 'not a cell'),
             (lambda: dev.circuit_matrix(R, (0.0, 1.0), cells, TOL), 'res_x and res_y'),
             (lambda: dev.circuit_matrix(R, (1.0, INF), cells, TOL), 'res_x and res_y'),
             (lambda: dev.circuit_matrix(R, res, cells, 0.0), 'tol'),
             (lambda: dev.circuit_matrix(R, res, cells, TOL, -1), 'max_iter'),
             (lambda: dev.circuit_matrix(R, res, [], TOL), 'cells'),
             (lambda: dev.circuit_current(R, res, np.arange(129), TOL), '1..128 cells'),
             (lambda: dev.circuit_budget(5 * R.size * 8 - 1), "below one system's rasters"),
             (lambda: dev.circuit_budget(-1), 'bytes >= 0'),
             (lambda: dev.circuit_matrix(R, res, cells, TOL, 1),
              r'did not converge after 1 iterations.*residual of [0-9.e+-]+')]
    calls += [(lambda B=B: dev.circuit_matrix(B, res, cells, TOL), 'every entry must be > 0')
              for B in bad_R]
    for call, match in calls:
        with pytest.raises(nat.GnxError, match=match):
            call()
        np.testing.assert_array_equal(dev.circuit_matrix(R, res, cells[:6], TOL), before)
    with pytest.raises(ValueError, match='R:'):
        dev.circuit_matrix(R[:, :-1], res, cells, TOL)
    # the current map wants every potential resident: 11 systems + one system's work
    dev.circuit_budget(5 * R.size * 8)
    try:
        with pytest.raises(nat.GnxError, match='resident: %d bytes are needed'
                           % ((11 + 4) * R.size * 8)):
            dev.circuit_current(R, res, cells, TOL)
    finally:
        dev.circuit_budget(0)
    np.testing.assert_array_equal(dev.circuit_matrix(R, res, cells[:6], TOL), before)


@pytest.mark.parametrize('H,W', [(1, 9), (9, 1), (64, 64), (65, 129), (1, 1)],
                         ids=lambda v: str(v))
def test_at_every_tile_edge(H, W):
    """the series chain (reff(0, k) = len k r), and flat rasters whose sides are one tile, one
    cell more than one and two tiles, and a single cell"""
    nat = native()
    dev = _device(nat, H, W)
    try:
        R = np.full((H, W), 3.0)
        if H * W == 1:
            assert dev.circuit_matrix(R, (1, 1), [0], TOL).tolist() == [[0.0]]
            cur, used, skipped = dev.circuit_current(R, (1, 1), [0], TOL)
            assert cur.tolist() == [[0.0]] and (used, skipped) == (0, 0)
            return
        if min(H, W) == 1:
            res = (2.0, 0.7)
            cells = np.arange(H * W, dtype=np.int32)
            got = dev.circuit_matrix(R, res, cells, TOL)
            step = 3.0 * (res[0] if H == 1 else res[1])
            want = step * np.abs(cells[:, None] - cells[None, :]).astype(np.float64)
            _check_matrix(got, want, lambda_2(R, res), 'chain %d x %d' % (H, W))
            return
        cells = np.array([0, W - 1, (H - 1) * W, H * W - 1, (H // 2) * W + W // 2], np.int32)
        got = dev.circuit_matrix(R, (1, 1), cells, TOL)
        ref = Q.numpy_resistance_matrix(R, (1, 1), cells)
        _check_matrix(got, ref, lambda_2(R, (1, 1)), '%d x %d' % (H, W))
    finally:
        dev.close()


# ------------------------------------------------------------------ the public calls
def _circuit_model(seed):
    """a 40 x 40 two-layer landscape (all ones; a west-east conductance gradient from 0.1 to
    1), the Species moving along layer 1 as its move_surf"""
    import geonomics_amd as gnx
    from geonomics_amd.sim import params as P
    d = P.default_params_dict(layers=[{'type': 'defined'}, {'type': 'defined'}],
                              species=[{'genomes': True, 'n_traits': 1,
                                        'movement_surface': True}])
    d['landscape']['main']['dim'] = (40, 40)
    d['landscape']['layers']['lyr_0']['init']['defined']['rast'] = np.ones((40, 40))
    d['landscape']['layers']['lyr_1']['init']['defined']['rast'] = \
        np.tile(np.linspace(0.1, 1, 40), (40, 1))
    s = d['comm']['species']['spp_0']
    s['init'].update({'N': 250, 'K_factor': 0.2})
    s['mating'].update({'mating_radius': 4})
    s['movement']['move_surf'].update({'layer': 'lyr_1'})
    s['gen_arch'].update({'L': 64, 'n_recomb_sims': 200, 'use_tskit': False})
    s['gen_arch']['traits']['trait_0'].update({'layer': 'lyr_1', 'n_loci': 4})
    d['model'].update({'T': 12, 'burn_T': 30, 'seed': {'num': seed}})
    mod = gnx.make_model(gnx.make_params_dict(d, 'circuit_test'))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(5, 'main', verbose=False)
    return mod


def test_model_calls_match_the_host_composition():
    mod = _circuit_model(5)
    spp = mod.comm[0]
    ids = np.array([*spp])
    cells = mod.get_cells()
    R = K.resistance_raster(np.tile(np.linspace(0.1, 1, 40), (40, 1)))
    lin = cells[:, 1] * 40 + cells[:, 0]
    uniq, inv = np.unique(lin, return_inverse=True)
    want = Q.expand(Q.numpy_resistance_matrix(R, (1, 1), uniq), inv)
    res = mod.calc_resistance_distances()
    print('calc_resistance_distances: n = %d on %d cells, info %s'
          % (ids.size, uniq.size, res['info']))
    np.testing.assert_array_equal(res['ids'], ids)
    np.testing.assert_array_equal(res['cells'], cells)
    off = ~np.eye(ids.size, dtype=bool)
    same = (lin[:, None] == lin[None, :])
    assert (res['dist'][same] == 0).all()
    _check_matrix(res['dist'], want, lambda_2(R, (1, 1)), 'calc_resistance_distances')
    assert np.isfinite(want[off]).all()
    cm = mod.calc_current_map(individs=ids[:40])
    u40 = np.unique(lin[:40])
    ref_cur, ref_used, ref_skipped = Q.numpy_current_map(R, (1, 1), u40)
    assert (cm['n_pairs'], cm['n_skipped']) == (ref_used, ref_skipped)
    np.testing.assert_array_equal(cm['cells'], u40)
    G = np.asarray(Q.laplacian(R, (1, 1)).diagonal()).reshape(R.shape)
    bound = 2 * ref_used * G * TOL / lambda_2(R, (1, 1)) + 16 * ref_used * 2.0 ** -53 * ref_cur
    assert (np.abs(cm['current'] - ref_cur) <= bound).all()
    # the tests on a sample, against sim/mmrr on the host with the restated matrix
    some = ids[:150]
    sel = np.isin(ids, some)
    n = some.size
    assert n >= 30                                           # 435 pairs for 3 coefficients
    got = mod.run_mmrr(predictors=('geo', 'circuit'), individs=some, nperm=199, seed=3)
    par = mod.run_mantel('circuit', given='geo', individs=some, nperm=199, seed=3)
    D = np.rint(mod.get_genotypes() * 2).astype(np.int64)[sel]
    xy = np.column_stack([mod.get_x(), mod.get_y()])[sel]
    Y = M.genetic_distances(D)
    Xs = [M.euclid(xy), want[np.ix_(sel, sel)]]
    rows = M.draw_row_shuffles(n, 199, seed=3)
    sums, mom = M.numpy_perm_sums(Y, Xs, rows), M.numpy_moments(Y, Xs)
    ref = M.mmrr(sums, mom, ['geo', 'circuit'])
    assert list(got) == list(ref)
    gap = smallest_gap(sums, mom)
    print('model: smallest relative gap %.3g' % gap)
    assert gap > GAP
    for keys in (['Intercept', 'geo', 'circuit'], ['Intercept(t)', 'geo(t)', 'circuit(t)'],
                 ['F-statistic'], ['R^2']):
        r = np.array([ref[k] for k in keys])
        err = np.abs(np.array([got[k] for k in keys]) - r).max() / np.abs(r).max()
        print('%s: %.3g of the largest entry' % (keys[-1], err))
        assert err <= BAR, (keys, err)
    for k in ('Intercept(p)', 'geo(p)', 'circuit(p)', 'F p-value'):
        assert got[k] == ref[k], k
    sums2 = sums[:, ::-1]
    mom2 = dict(mom, sx=mom['sx'][::-1], sxy=mom['sxy'][::-1], sxx=mom['sxx'][::-1, ::-1])
    pref = M.mantel(sums2, mom2, 0, 1)
    assert np.abs(pref['perm_r'] - pref['r']).min() > GAP * abs(pref['r'])
    assert abs(par['r'] - pref['r']) <= BAR and par['nperm'] == 199
    assert np.abs(par['perm_r'] - pref['perm_r']).max() <= BAR
    assert par['p'] == pref['p']
    # ('geo', 'cost') still is what it was before there was a 'circuit': the least-cost matrix
    # of the distinct cells, expanded, behind the 'geo' columns in gnx_dist_perm_sums_mat
    a = mod.run_mmrr(predictors=('geo', 'cost'), individs=some, nperm=49, seed=2)
    _, slots = spp._geno_sample(some)
    us, inv_s = np.unique(lin[sel], return_inverse=True)
    Dc = K.expand(spp._dev.cost_matrix(R, (1.0, 1.0), us), inv_s)
    sums_old, mom_old = spp._dev.dist_perm_sums_mat(
        [GEO], Dc[None], M.invert_rows(M.draw_row_shuffles(n, 49, seed=2)), slots)
    b = M.mmrr(sums_old, mom_old, ['geo', 'cost'])
    assert list(a) == list(b) and all(a[k] == b[k] for k in b)
