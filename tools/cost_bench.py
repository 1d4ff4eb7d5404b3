"""Least-cost distances and matrix predictors on the device (csrc/gnx_cost.hip,
gnx_dist_perm_sums_mat): one JSON line per measurement.

    python tools/cost_bench.py                      # 1024 x 1024, 1024 sources
    python tools/cost_bench.py --host-sources 64    # profiles/r24_cost.txt: scipy on 64 of them

Two rasters of 1024 x 1024 cells: bench.py's seeded smooth conductance field (the move_surf of
C4, 0.5 .. 1), and the same with long barriers (a wall every 128 columns, open for 16 cells at
alternating ends, so that the cheapest path to the far side winds through the whole raster).
gnx_cost_matrix of n random passable cells: host clock around the call, the kernels' HIP-event
time, rounds and batches (gnx_cost_info), and settled cell distances (H W per source) per second
of kernel time.  The yardstick is scipy's Dijkstra on the same graph (sim/cost.py), the sources
split over 16 host processes; it is run before the device is opened, on --host-sources of the
sources (its time per source does not depend on their number), and compared value by value.

Then gnx_dist_perm_sums_mat with one column predictor and one matrix beside gnx_dist_perm_sums
with two column predictors: a sample of n individuals of bench.py's 'small' population.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geonomics_amd.sim import cost as K  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def rasters(W, H):
    """name -> R float64 [H][W]"""
    from scipy.ndimage import zoom
    rng = np.random.RandomState(1)                    # bench.smooth_field(W, H, 1)
    k = 16
    f = zoom(rng.rand(H // k + 3, W // k + 3), k, order=3)[:H, :W]
    f = ((f - f.min()) / (f.max() - f.min())).astype(np.float32)
    cond = f.astype(np.float64) * 0.5 + 0.5
    smooth = K.resistance_raster(cond)
    walls = smooth.copy()
    for i, x in enumerate(range(128, W, 128)):
        walls[:, x] = np.inf
        if i % 2 == 0:
            walls[:16, x] = smooth[:16, x]
        else:
            walls[-16:, x] = smooth[-16:, x]
    return {'smooth': smooth, 'barriers': walls}


_G = {}


def _host_init(R, res):
    _G['graph'] = K.edge_graph(R, res)


def _host_solve(src):
    from scipy.sparse.csgraph import dijkstra
    return dijkstra(_G['graph'], directed=True, indices=src)


def host_dijkstra(R, res, src, procs):
    """scipy's Dijkstra, the sources split over `procs` processes -> seconds, distances"""
    parts = [p for p in np.array_split(src, procs) if p.size]
    ctx = mp.get_context('spawn')
    with ctx.Pool(len(parts), initializer=_host_init, initargs=(R, res)) as pool:
        pool.map(_host_solve, [p[:1] for p in parts])        # the graphs are built
        t0 = time.perf_counter()
        out = pool.map(_host_solve, parts)
        dt = time.perf_counter() - t0
    return dt, np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--sources', type=int, default=1024)
    ap.add_argument('--host-sources', type=int, default=128)
    ap.add_argument('--procs', type=int, default=16)
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--nperm', type=int, default=999)
    ap.add_argument('--reps', type=int, default=2)
    a = ap.parse_args()
    W = H = a.size
    res = (1.0, 1.0)
    Rs = rasters(W, H)
    rng = np.random.RandomState(3)
    cells = {k: np.sort(rng.choice(np.flatnonzero(np.isfinite(R.ravel())), a.sources,
                                   replace=False)).astype(np.int32) for k, R in Rs.items()}
    host = {}
    if a.host_sources > 0:
        for k, R in Rs.items():
            sub = cells[k][:: max(1, a.sources // a.host_sources)][:a.host_sources]
            dt, d = host_dijkstra(R, res, sub, a.procs)
            host[k] = (sub, d, dt)
            emit(what='scipy_dijkstra', raster=k, cells=W * H, sources=int(sub.size),
                 processes=a.procs, s=round(dt, 3), s_per_source_per_process=round(
                     dt / np.ceil(sub.size / a.procs), 4),
                 s_for_all_sources=round(dt * a.sources / sub.size, 2),
                 note='the last figure scales the measured time to --sources')
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    import bench
    from geonomics_amd import _native as nat
    from geonomics_amd.sim import mmrr as M
    dev = nat.Device(W, H, 1)
    dev.upload_rasters(np.ones((1, H, W), np.float32))
    for k, R in Rs.items():
        for rep in range(a.reps):
            t0 = time.perf_counter()
            D = dev.cost_matrix(R, res, cells[k])
            dt = time.perf_counter() - t0
            info = dev.cost_info()
            emit(what='cost_matrix', raster=k, cells=W * H, sources=a.sources, rep=rep,
                 wall_s=round(dt, 3), kernel_ms=round(info['kernel_ms'], 2),
                 rounds=info['rounds'], batches=info['batches'], launches=info['launches'],
                 settled_cells_per_s=W * H * a.sources / (info['kernel_ms'] * 1e-3),
                 max_finite=float(D[np.isfinite(D)].max()), n_inf=int(np.isinf(D).sum()))
        if k in host:
            sub, d, dt = host[k]
            got = dev.cost_surfaces(R, res, sub[:8]).reshape(8, -1)
            ref = d[:8]
            ok = np.isfinite(ref)
            emit(what='device_vs_scipy', raster=k, sources=8,
                 inf_pattern_equal=bool((np.isfinite(got) == ok).all()),
                 max_rel_err=float((np.abs(got[ok] - ref[ok]) / np.maximum(ref[ok], 1e-300)).max()),
                 bit_equal=bool((got[ok] == ref[ok]).all()))
    dev.close()
    # ---- the matrix path of the permutation test
    cfg = bench.WORKLOADS['small']
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(5, False, True)
    n = min(a.n, dev.N)
    slots = np.sort(np.random.RandomState(1).choice(dev.N, n, replace=False)).astype(np.int64)
    perm = M.invert_rows(M.draw_row_shuffles(n, a.nperm, seed=1))
    x, y = (dev.download(f).astype(np.float64)[slots] for f in (nat.F_X, nat.F_Y))
    geo = M.euclid(np.column_stack([x, y]))[None]
    GEO, ENV = [(nat.F_X, 0), (nat.F_Y, 0)], [(nat.F_E, 1)]
    t_old, t_mat = [], []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        old = dev.dist_perm_sums([ENV, GEO], perm, slots)
        t1 = time.perf_counter()
        new = dev.dist_perm_sums_mat([ENV], geo, perm, slots)
        t2 = time.perf_counter()
        if rep:
            t_old.append(t1 - t0)
            t_mat.append(t2 - t1)
    emit(what='dist_perm_sums_mat', n=n, nperm=a.nperm,
         two_columns_ms=[round(t * 1e3, 1) for t in t_old],
         column_and_matrix_ms=[round(t * 1e3, 1) for t in t_mat],
         ratio=min(t_mat) / min(t_old),
         max_rel_diff=float((np.abs(new[0] - old[0]) / np.abs(old[0])).max()),
         note='host clock around the synchronous calls; the matrix call uploads n x n doubles')
    dev.close()


if __name__ == '__main__':
    main()
