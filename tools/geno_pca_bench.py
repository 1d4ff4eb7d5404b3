"""Genetic PCA on the device (csrc/gnx_geno.hip, sim/pca.py): one JSON line per measurement.

    python tools/geno_pca_bench.py --part metric   # c4_metric: passes, Gram, full PCA
    python tools/geno_pca_bench.py --part c2       # C2: device PCA vs the host route

metric: bench.py's c4_metric population (10^6 individuals, L = 10^5) walked 20 steps (blocks
shared with parents), then: live physical blocks (gnx_debug_halves, after a collection), the
time of one gnx_geno_matmul and one gnx_geno_rmatmul pass with k = 16 (after warm-up; the
calls are synchronous, timed by the host clock around them), FLOPs and bytes per pass from
the shapes, gnx_geno_gram at n = 8192 over all loci, and a whole randomized
calc_genetic_PCA(n_pcs=3) (n_iter 8, oversample 10).
c2: the C2 workload (10^5 x 10^4) the same way, three repeats each of the device route and of
the parent's only route: gnx_download_genomes of every slot (what Model.get_genotypes does),
unpacking, and numpy randomized PCA in fp64 with the same n_iter.
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
from geonomics_amd.sim import pca as P  # noqa: E402

FP32_PEAK = 157.3e12         # MI355X_MICROARCH: FP32 vector
HBM_PEAK = 8.0e12


def emit(**kw):
    print(json.dumps(kw), flush=True)


def setup(name, seed=1, steps=20):
    cfg = bench.WORKLOADS[name]
    dev, _, _ = bench.build_device(cfg, seed, 0)
    bench.setup_genomes(dev, cfg, seed)
    dev.walk(steps, False, True)
    return dev, cfg


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return t


def passes(dev, cfg, name, k=16, reps=5):
    import torch
    N, L = dev.N, cfg['L']
    rows, broken, gcs, used, free, total = (int(v) for v in dev.debug_halves())
    info = dev.genome_info()
    logical = 2 * N * info['NB']
    emit(workload=name, what='blocks', N=N, L=L, NB=info['NB'], BW_words=info['BW'],
         logical_blocks=logical, live_physical_blocks=used, shared_fraction=1 - used / logical)
    M = torch.randn((L, k), dtype=torch.float32, device='cuda')
    Y = torch.randn((N, k), dtype=torch.float32, device='cuda')
    flops = 2.0 * N * L * k
    geno_bytes = N * 2 * dev.W64 * 8.0             # every row's words, as the kernels read them
    distinct = used * info['BW'] * 8.0             # ... of which distinct (shared blocks)
    for what, fn, io in (('matmul', lambda: dev.geno_matmul(M), (L * k + N * k) * 4.0),
                         ('rmatmul', lambda: dev.geno_rmatmul(Y), (L * k + N * k) * 4.0)):
        t = timed(fn, reps)
        best = min(t)
        emit(workload=name, what=what, k=k, ms=[round(x * 1e3, 3) for x in t],
             ms_best=round(best * 1e3, 3), flop=flops, bytes_read=geno_bytes + io,
             bytes_distinct=distinct + io, tflops=flops / best / 1e12,
             share_fp32_peak=flops / FP32_PEAK / best,
             share_hbm_peak=(geno_bytes + io) / HBM_PEAK / best,
             bound='compute' if flops / FP32_PEAK > (geno_bytes + io) / HBM_PEAK else 'hbm')


def part_metric():
    dev, cfg = setup('c4_metric')
    passes(dev, cfg, 'c4_metric')
    slots = np.random.RandomState(0).choice(dev.N, 8192, replace=False).astype(np.int64)
    t = timed(lambda: dev.geno_gram(slots), 2, warm=1)
    emit(workload='c4_metric', what='gram', n=8192, L=cfg['L'], ms=[round(x * 1e3, 1) for x in t])
    t = timed(lambda: P.device_randomized_pca(dev, 3), 2, warm=1)
    emit(workload='c4_metric', what='calc_genetic_PCA_randomized', n_pcs=3, n_iter=8,
         oversample=10, s=[round(x, 3) for x in t])
    dev.close()


def host_route(dev, cfg, n_iter=8):
    """the parent commit's only route: download every genome, unpack, numpy PCA in fp64"""
    L = cfg['L']
    t0 = time.perf_counter()
    packed = dev.download_genomes(np.arange(dev.N))
    t1 = time.perf_counter()
    by = np.ascontiguousarray(packed).view(np.uint8).reshape(packed.shape[0], 2, -1)
    bits = np.unpackbits(by, axis=2, bitorder='little')[:, :, :L]
    D = (bits[:, 0] + bits[:, 1]).astype(np.float64)
    del bits, by
    t2 = time.perf_counter()
    scores, ratio = P.randomized_pca(lambda M: D @ M, lambda Y: D.T @ Y, D.mean(axis=0),
                                     D.shape[0], L, 3, n_iter=n_iter,
                                     sumsq=(D * D).sum(axis=0))
    t3 = time.perf_counter()
    return (t1 - t0, t2 - t1, t3 - t2, t3 - t0), scores, ratio


def part_c2():
    dev, cfg = setup('c2')
    passes(dev, cfg, 'c2')
    dev_t, host_t = [], []
    for r in range(3):
        t0 = time.perf_counter()
        s_dev, r_dev = P.device_randomized_pca(dev, 3)
        dev_t.append(time.perf_counter() - t0)
        t, s_host, r_host = host_route(dev, cfg)
        host_t.append(t)
        emit(workload='c2', what='repeat', r=r, device_s=round(dev_t[-1], 3),
             host_download_s=round(t[0], 3), host_unpack_s=round(t[1], 3),
             host_pca_s=round(t[2], 3), host_total_s=round(t[3], 3),
             ratio_device=r_dev.tolist(), ratio_host=r_host.tolist(),
             score_cos=[float(abs((s_dev[:, j] * s_host[:, j]).sum())
                              / np.linalg.norm(s_dev[:, j]) / np.linalg.norm(s_host[:, j]))
                        for j in range(3)])
    d, h = np.array(dev_t), np.array([t[3] for t in host_t])
    emit(workload='c2', what='device_vs_host', device_s_median=float(np.median(d)),
         device_s_spread=[float(d.min()), float(d.max())], host_s_median=float(np.median(h)),
         host_s_spread=[float(h.min()), float(h.max())], ratio_host_over_device=float(
             np.median(h) / np.median(d)))
    dev.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['metric', 'c2'], required=True)
    a = ap.parse_args()
    import torch
    torch.cuda.init()           # torch's HIP runtime first, the library's handles behind it (bench.py)
    part_metric() if a.part == 'metric' else part_c2()
