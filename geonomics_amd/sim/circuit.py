"""Isolation by resistance in McRae's circuit-theory sense: effective resistances and cumulative
current maps over the landscape's cells (an extension: the reference has no such analysis;
sim/cost.py gives the least-cost distances over the same graph).

The graph is the one sim/cost.py pins.  Nodes: the H x W cells, 8 neighbours each; an edge
exists iff both ends are passable (R finite) and is a resistor of
    w = (0.5 * (R[u] + R[v])) * len        len = res_x, res_y or sqrt(res_x^2 + res_y^2)
ohms, evaluated in that order in fp64.  Its conductance is g = 1.0 / w, and the Laplacian is
L = diag(sum g) - G, taken component by component.

    reff(s, t) = (e_s - e_t)' L+ (e_s - e_t)      two passable cells of one component
    reff(s, s) = 0                                also on an impassable cell
    reff       = inf                              between components, from or to an impassable cell

The matrix is exactly symmetric: the entry a > b is computed once and mirrored.  The current
of a pair (s, t): with the potentials v = L+ (e_s - e_t), the current through cell u is
    c(u) = 0.5 * (sum_k g_uk |v_u - v_k| + |b_u|)        b = +1 at s, -1 at t, 0 elsewhere
(Circuitscape's node current: the source and the sink carry 1, a cell of a 1-wide corridor
between them carries 1).  The current map of a set of cells is the sum of c over all unordered
pairs that share a component; impassable cells hold 0.

The device solves L x_i = e_i - e_a per focal cell i against the first listed focal cell a of
its component (the anchor) by conjugate gradients (csrc/gnx_circuit.hip); here every component
is grounded at one node and the reduced Laplacian factorised with scipy's splu.  Pure
functions, fp64.
"""
import numpy as np

from . import cost as _cost
from .cost import expand                                    # noqa: F401  (reused as it is)


def laplacian(R, res=(1.0, 1.0)):
    """L = diag(sum g) - G as a scipy CSR matrix [H W][H W], g = 1.0 / w of the pinned edges;
    the rows and columns of impassable cells are empty"""
    from scipy.sparse import csr_matrix, diags
    Wg = _cost.edge_graph(R, res).tocoo()
    G = csr_matrix((1.0 / Wg.data, (Wg.row, Wg.col)), shape=Wg.shape)
    return (diags(np.asarray(G.sum(axis=1)).ravel()) - G).tocsr()


def components(R):
    """int64 [H][W]: the label of every passable cell's connected component = the lowest cell
    index (y * W + x) in it; -1 on impassable cells"""
    from scipy.sparse.csgraph import connected_components
    R = np.asarray(R, np.float64)
    R, _, _ = _cost._check(R, (1.0, 1.0))
    ok = np.isfinite(R).ravel()
    _, lab = connected_components(_cost.edge_graph(R), directed=False)
    first = np.full(lab.max() + 1, R.size, np.int64)
    np.minimum.at(first, lab, np.arange(R.size))
    out = first[lab]
    out[~ok] = -1
    return out.reshape(R.shape)


def _cells(R, cells):
    cells = _cost._sources(cells, R.size, 'cells')
    if np.unique(cells).size != cells.size:
        raise ValueError('cells: a cell is listed twice')
    return cells


def _solvers(R, res):
    """(labels [H W], {label: (nodes of the component without its ground, splu of the reduced
    Laplacian or None for a single cell, position of every cell among those nodes)})"""
    from scipy.sparse.linalg import splu
    L = laplacian(R, res).tocsc()
    lab = components(R).ravel()
    out = {}
    for c in np.unique(lab[lab >= 0]):
        nodes = np.flatnonzero(lab == c)[1:]               # the lowest cell is the ground
        pos = np.full(lab.size, -1, np.int64)
        pos[nodes] = np.arange(nodes.size)
        lu = splu(L[nodes][:, nodes].tocsc()) if nodes.size else None
        out[int(c)] = (nodes, lu, pos)
    return lab, out


def _grounded(solver, n_all, s, t):
    """v [n_all] with L v = e_s - e_t on the component of `solver`, 0 at its ground and
    outside the component"""
    nodes, lu, pos = solver
    v = np.zeros(n_all)
    if lu is None or s == t:
        return v
    b = np.zeros(nodes.size)
    if pos[s] >= 0:
        b[pos[s]] += 1.0
    if pos[t] >= 0:
        b[pos[t]] -= 1.0
    v[nodes] = lu.solve(b)
    return v


def numpy_potentials(R, res, cells):
    """(x float64 [n][H][W], anchor int64 [n]) of distinct cells (gnx_circuit_potentials
    restated): anchor[i] = the index in `cells` of the first listed cell of cell i's component
    (-1 on an impassable cell); x[i] solves L x = e_i - e_anchor on that component with
    x = 0 at the anchor's cell, and is 0 everywhere for an anchor or an impassable cell.  The
    device's x[i] differs from this one by a constant on the component"""
    R, _, _ = _cost._check(R, res)
    cells = _cells(R, cells)
    lab, solvers = _solvers(R, res)
    x = np.zeros((cells.size, R.size))
    anchor = np.full(cells.size, -1, np.int64)
    first = {}
    for i, c in enumerate(cells):
        if lab[c] < 0:
            continue
        a = first.setdefault(int(lab[c]), i)
        anchor[i] = a
        if a != i:
            v = _grounded(solvers[int(lab[c])], R.size, int(c), int(cells[a]))
            on = lab == lab[c]
            v[on] -= v[cells[a]]
            x[i] = v
    return x.reshape((cells.size,) + R.shape), anchor


def numpy_resistance_matrix(R, res, cells):
    """pairwise effective resistances float64 [n][n] of distinct cells (gnx_circuit_matrix
    restated): per component one node is grounded and the reduced Laplacian factorised; exactly
    symmetric, the entry a > b being the mirror of b < a"""
    R, _, _ = _cost._check(R, res)
    cells = _cells(R, cells)
    n = cells.size
    lab, solvers = _solvers(R, res)
    D = np.full((n, n), np.inf)
    np.fill_diagonal(D, 0.0)
    for c, (nodes, lu, pos) in solvers.items():
        idx = np.flatnonzero(lab[cells] == c)
        if idx.size < 2:
            continue
        # column i of Z: the grounded solution of L z = e_i, read at the focal cells
        Z = np.zeros((idx.size, idx.size))
        for k, i in enumerate(idx):
            if pos[cells[i]] < 0:
                continue                                   # the ground itself: z = 0
            b = np.zeros(nodes.size)
            b[pos[cells[i]]] = 1.0
            z = lu.solve(b)
            at = pos[cells[idx]]
            Z[:, k] = np.where(at >= 0, z[np.maximum(at, 0)], 0.0)
        for a in range(idx.size):
            for b_ in range(a + 1, idx.size):
                r = (Z[a, a] - Z[b_, a]) - (Z[a, b_] - Z[b_, b_])
                D[idx[a], idx[b_]] = D[idx[b_], idx[a]] = r
    return D


def numpy_current_map(R, res, cells):
    """(current float64 [H][W], pairs used, pairs skipped) of distinct cells
    (gnx_circuit_current restated): the sum of the node currents c(u) over all unordered pairs
    of cells that share a component; a pair with an impassable cell or across components is
    skipped; impassable cells hold 0"""
    R, _, _ = _cost._check(R, res)
    cells = _cells(R, cells)
    n = cells.size
    lab, solvers = _solvers(R, res)
    G = (-laplacian(R, res)).tocoo()
    off = G.row != G.col
    gu, gv, gg = G.row[off], G.col[off], G.data[off]
    cur = np.zeros(R.size)
    used = 0
    for a in range(n):
        for b_ in range(a + 1, n):
            s, t = int(cells[a]), int(cells[b_])
            if lab[s] < 0 or lab[s] != lab[t]:
                continue
            used += 1
            v = _grounded(solvers[int(lab[s])], R.size, s, t)
            c = np.bincount(gu, weights=gg * np.abs(v[gu] - v[gv]), minlength=R.size)
            c[s] += 1.0
            c[t] += 1.0
            cur += 0.5 * c
    return cur.reshape(R.shape), used, n * (n - 1) // 2 - used
