"""Model.run_mmrr / run_mantel on the device (csrc/gnx_mantel.hip, sim/mmrr.py): one JSON line
per measurement.

    python tools/mmrr_bench.py                        # c4_metric, n = 8192, 999 permutations
    tools/kstat_cmd.sh r20_mmrr tools/mmrr_bench.py   # the same under rocprofv3: kernel times

bench.py's metric population (10^6 individuals, L = 10^5) walked 20 steps; a random sample of n
living individuals over all loci, predictors geo = (x, y) and env = layer 1.
gnx_dist_perm_sums is synchronous and ends with its downloads (host clock around it): the call
with one permutation is the Gram part (gather, the n x n Gram matrix into scratch, the moments,
one pass of the tiles), the call with nperm permutations less that one the permutation part,
reported in ms and in pair evaluations (one Y[a][b] x one predictor distance) per second; the
kernels' own times come from the rocprofv3 run.  Then the statistics (sim/mmrr.py) from the
sums, and for scale the host restatement: numpy on the downloaded genomes and columns, a few
permutations of a smaller sample (no existing kernel does this work: the parent commit offers
nothing else to compare against).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from geonomics_amd import _native as nat  # noqa: E402
from geonomics_amd.sim import mmrr as M  # noqa: E402

PREDICTORS = [[(nat.F_X, 0), (nat.F_Y, 0)], [(nat.F_E, 1)]]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return t


def host_restatement(dev, slots, nperm, seed):
    """numpy on the downloaded sample -> (seconds: download + distances, permutations), sums"""
    t0 = time.perf_counter()
    packed = dev.download_genomes(slots)
    by = np.ascontiguousarray(packed).view(np.uint8).reshape(packed.shape[0], 2, -1)
    bits = np.unpackbits(by, axis=2, bitorder='little')[:, :, :dev.L]
    D = (bits[:, 0] + bits[:, 1]).astype(np.float32)
    G = np.rint(D @ D.T).astype(np.int64)             # entries below 2^24: exact
    g = np.diag(G)
    Y = 0.5 * np.sqrt((g[:, None] + g[None, :] - 2 * G).astype(np.float64))
    x, y, e = (dev.download(f).astype(np.float64) for f in (nat.F_X, nat.F_Y, nat.F_E))
    Xs = [M.euclid(np.column_stack([x[slots], y[slots]])), M.euclid(e[1][slots])]
    t1 = time.perf_counter()
    rows = M.draw_row_shuffles(slots.size, nperm, seed=seed)
    sums = M.numpy_perm_sums(Y, Xs, rows)
    t2 = time.perf_counter()
    return (t1 - t0, t2 - t1), sums, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c4_metric', choices=sorted(bench.WORKLOADS))
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--nperm', type=int, default=999)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--host-n', type=int, default=2048)
    ap.add_argument('--host-nperm', type=int, default=3)
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    cfg = bench.WORKLOADS[a.workload]
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(20, False, True)
    N, L = dev.N, cfg['L']
    rng = np.random.RandomState(1)
    n = min(a.n, N)
    slots = np.sort(rng.choice(N, n, replace=False)).astype(np.int64)
    perm = M.invert_rows(M.draw_row_shuffles(n, a.nperm, seed=1))
    m = n * (n - 1) // 2
    K = len(PREDICTORS)
    t1 = timed(lambda: dev.dist_perm_sums(PREDICTORS, perm[:1], slots), a.reps)
    out = {}

    def full():
        out['r'] = dev.dist_perm_sums(PREDICTORS, perm, slots)
    tp = timed(full, a.reps)
    perm_s = max(min(tp) - min(t1), 1e-9)
    tiles = (n + 63) // 64
    emit(workload=a.workload, what='gram_part', N=N, L=L, n=n, predictors=K,
         ms=[round(x * 1e3, 2) for x in t1],
         note='gather, Gram into scratch, moments, one permutation; host clock')
    emit(workload=a.workload, what='permutation_part', N=N, L=L, n=n, predictors=K,
         nperm=a.nperm, call_ms=[round(x * 1e3, 2) for x in tp], ms=round(perm_s * 1e3, 2),
         pair_evaluations=m * K * (a.nperm - 1),
         pair_evaluations_per_s=m * K * (a.nperm - 1) / perm_s,
         tile_evaluations=tiles * (tiles + 1) // 2 * 4096 * K * (a.nperm - 1),
         bytes_to_host=(a.nperm * K + 3 + 2 * K + K * (K + 1) // 2) * 8,
         bytes_from_host=perm.nbytes)
    sums, mom = out['r']
    t0 = time.perf_counter()
    res = M.mmrr(sums, mom, ['geo', 'env'])
    par = M.mantel(sums[:, ::-1], dict(mom, sx=mom['sx'][::-1], sxy=mom['sxy'][::-1],
                                       sxx=mom['sxx'][::-1, ::-1]), 0, 1)
    emit(workload=a.workload, what='host_algebra', ms=round((time.perf_counter() - t0) * 1e3, 3),
         mmrr={k: float(v) for k, v in res.items()},
         mantel_env_given_geo=dict(r=par['r'], p=par['p']))
    if a.host_n > 0:
        hs = slots[:min(a.host_n, n)]
        (td, tperm), ref, rows = host_restatement(dev, hs, a.host_nperm, 2)
        got, _ = dev.dist_perm_sums(PREDICTORS, M.invert_rows(rows), hs)
        emit(workload=a.workload, what='host_restatement', n=int(hs.size), nperm=a.host_nperm,
             download_and_distances_s=round(td, 3), permutations_s=round(tperm, 3),
             s_per_permutation=round(tperm / a.host_nperm, 4),
             device_vs_host_rel_err=float((np.abs(got - ref) / ref).max()))
    dev.close()


if __name__ == '__main__':
    main()
