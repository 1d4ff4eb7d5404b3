"""Isolation by resistance: least-cost distances over the landscape's cells (an extension: the
reference moves and disperses its individuals along conductance surfaces, but has no analysis
of the cost of travelling through them).

The graph.  Nodes: the H x W cells.  Every cell is joined to its 8 neighbours.  R is an fp64
raster of resistances, every entry > 0 or impassable (inf).  The edge between passable cells
u, v costs
    w = (0.5 * (R[u] + R[v])) * len
evaluated in that order in fp64, len = res_x, res_y or sqrt(res_x^2 + res_y^2) of the step;
an edge exists iff both ends are passable (a diagonal step does not look at the two cells it
passes between).  d(s, t) = the cost of the cheapest path between the cell centres, d(s, s) = 0
(also on an impassable cell), d = inf where there is no path; an impassable source is at inf
from every other cell.  A path's cost is the fp64 sum of its edges from the source on; the
addition is monotone, so the distances are the unique fixed point of d[v] = min_u (d[u] + w_uv)
below d[source] = 0, whatever the order of relaxation: scipy's Dijkstra here, a tiled iterative
solver on the device (csrc/gnx_cost.hip).

resistance_raster builds R from a layer's values; numpy_cost_surfaces / numpy_cost_matrix are
the host restatement of gnx_cost_surfaces / gnx_cost_matrix.  Pure functions, fp64.
"""
import numpy as np

KINDS = ('conductance', 'resistance')


def resistance_raster(values=None, kind='conductance', barrier=None, cost=None, shape=None):
    """R float64 [H][W], inf where impassable.
    kind='conductance': R = 1 / v of the values v; cells with v <= barrier (default 0) are
    impassable.  kind='resistance': R = v; cells with v >= barrier are impassable when barrier
    is given; a passable v <= 0 raises.  cost: an explicit [H][W] array of R (inf / nan:
    impassable; a passable entry <= 0 raises); it overrides values / kind.  shape: the (H, W)
    the result must have"""
    if cost is not None:
        R = np.array(cost, dtype=np.float64)
        want = shape if shape is not None else (None if values is None else np.shape(values))
        if R.ndim != 2 or (want is not None and R.shape != tuple(want)):
            raise ValueError('cost: an [H][W] array%s, not %s'
                             % ('' if want is None else ' of shape %s' % (tuple(want),), R.shape))
        R[np.isnan(R)] = np.inf
        if (R <= 0).any():
            raise ValueError('cost: every passable entry must be > 0 (inf or nan: impassable)')
        return R
    if kind not in KINDS:
        raise ValueError("kind: 'conductance' or 'resistance' (got %r)" % (kind,))
    if values is None:
        raise ValueError('no layer values and no cost raster')
    v = np.array(values, dtype=np.float64)
    if v.ndim != 2 or (shape is not None and v.shape != tuple(shape)):
        raise ValueError('the layer is not an [H][W] raster%s: %s'
                         % ('' if shape is None else ' of shape %s' % (tuple(shape),), v.shape))
    if np.isnan(v).any():
        raise ValueError('the layer holds nan')
    if kind == 'conductance':
        shut = v <= (0.0 if barrier is None else float(barrier))
        shut |= v <= 0                                       # a negative barrier opens nothing
        R = np.full(v.shape, np.inf)
        R[~shut] = 1.0 / v[~shut]
        return R
    shut = np.isinf(v)
    if barrier is not None:
        shut |= v >= float(barrier)
    if (v[~shut] <= 0).any():
        raise ValueError("kind='resistance': every passable value must be > 0 (give barrier=... "
                         "to close cells, or kind='conductance')")
    R = v.copy()
    R[shut] = np.inf
    return R


def _check(R, res):
    R = np.asarray(R, np.float64)
    if R.ndim != 2 or R.size == 0:
        raise ValueError('R: an [H][W] raster')
    if np.isnan(R).any() or (R <= 0).any():
        raise ValueError('R: every entry > 0, or inf where impassable')
    rx, ry = abs(float(res[0])), abs(float(res[1]))
    if not (np.isfinite(rx) and np.isfinite(ry) and rx > 0 and ry > 0):
        raise ValueError('res: two positive cell sizes (got %r)' % (res,))
    return R, rx, ry


def edge_graph(R, res=(1.0, 1.0)):
    """the pinned graph as a scipy CSR matrix [H W][H W] (both directions of every edge)"""
    from scipy.sparse import csr_matrix
    R, rx, ry = _check(R, res)
    H, W = R.shape
    idx = np.arange(H * W).reshape(H, W)
    diag = np.sqrt(rx * rx + ry * ry)
    us, vs, ws = [], [], []
    # E, S, SE, SW
    for (ua, va, ln) in ((np.s_[:, :-1], np.s_[:, 1:], rx), (np.s_[:-1, :], np.s_[1:, :], ry),
                         (np.s_[:-1, :-1], np.s_[1:, 1:], diag),
                         (np.s_[:-1, 1:], np.s_[1:, :-1], diag)):
        w = (0.5 * (R[ua] + R[va])) * ln
        ok = np.isfinite(w)
        us.append(idx[ua][ok])
        vs.append(idx[va][ok])
        ws.append(w[ok])
    u, v, w = np.concatenate(us), np.concatenate(vs), np.concatenate(ws)
    return csr_matrix((np.concatenate([w, w]), (np.concatenate([u, v]), np.concatenate([v, u]))),
                      shape=(H * W, H * W))


def _sources(src, n_cells, what):
    src = np.asarray(src, np.int64).ravel()
    if src.size and (src.min() < 0 or src.max() >= n_cells):
        raise ValueError('%s: cells in 0..%d (cell = y * W + x)' % (what, n_cells - 1))
    return src


def numpy_cost_surfaces(R, res, src):
    """the accumulated-cost raster of every source cell (y * W + x) -> float64 [n_src][H][W]
    (gnx_cost_surfaces restated with scipy's Dijkstra)"""
    from scipy.sparse.csgraph import dijkstra
    R, _, _ = _check(R, res)
    H, W = R.shape
    src = _sources(src, H * W, 'src')
    if src.size == 0:
        return np.zeros((0, H, W))
    d = dijkstra(edge_graph(R, res), directed=True, indices=src)
    return np.asarray(d, np.float64).reshape(src.size, H, W)


def numpy_cost_matrix(R, res, cells):
    """pairwise least-cost distances float64 [n][n] of distinct cells (gnx_cost_matrix
    restated): exactly symmetric, the entry a > b being the one computed from source b"""
    R, _, _ = _check(R, res)
    cells = _sources(cells, R.size, 'cells')
    if np.unique(cells).size != cells.size:
        raise ValueError('cells: a cell is listed twice')
    S = numpy_cost_surfaces(R, res, cells).reshape(cells.size, -1)[:, cells]
    up = np.triu(S)
    return up + np.triu(S, 1).T


def expand(D, inverse):
    """the matrix of individuals from the matrix of their distinct cells: individual i stands
    on distinct cell inverse[i] (two individuals on one cell are at cost 0)"""
    inverse = np.asarray(inverse, np.int64).ravel()
    return np.ascontiguousarray(np.asarray(D, np.float64)[inverse][:, inverse])
