"""Weighted relationship matrices on the device (csrc/gnx_grm.hip, sim/quantgen.py): one JSON
line per measurement.

    python tools/grm_bench.py --part metric   # c4_metric: gnx_grm at n = 8192, L = 10^5
    python tools/grm_bench.py --part c2       # C2: the device route vs download + numpy fp64

metric: bench.py's c4_metric population (10^6 individuals, L = 10^5) walked 20 steps, a random
sample of 8192: the allele counts (gnx_stats_group_counts), the GCTA table (grm_values),
gnx_grm (kernel_ms by HIP events around its kernels, best and all repeats after a warm-up; the
whole call by the host clock, which adds the download of the 512 MiB matrix), the achieved
TFLOP/s - 2 n^2 L for the full matrix that comes back, and n (n + 128) L for the tiles of the
upper triangle that are computed - against the 157 TF f32 matrix peak and the 122 TF of an
untuned LDS-tiled f32 MFMA GEMM, the kernel with its expansion alone and its MFMAs alone
(gnx_grm_probe), gnx_geno_gram on the same sample, and the host parts of a heritability
estimate on that matrix (eigh, REML, Haseman-Elston) for a synthetic response.
c2: the C2 workload (10^5 x 10^4), a sample of --n (default 8192), three repeats each of the
device route (counts + table + gnx_grm) and of the parent's only route to the same matrix:
gnx_download_genomes of the sample, unpacking, the standardised Z in fp64 and Z Z^T in numpy.
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
from geonomics_amd.sim import quantgen as Q  # noqa: E402

F32_MATRIX_PEAK = 157.3e12   # MI355X: f32 MFMA = the f32 vector rate
F32_GEMM_UNTUNED = 122e12    # an untuned LDS-tiled kernel on mfma_f32_32x32x2f32 at 4096^3


def emit(**kw):
    print(json.dumps(kw), flush=True)


def setup(name, seed=1, steps=20):
    cfg = bench.WORKLOADS[name]
    dev, _, _ = bench.build_device(cfg, seed, 0)
    bench.setup_genomes(dev, cfg, seed)
    dev.walk(steps, False, True)
    return dev, cfg


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def device_route(dev, slots, mask_words):
    n = slots.size
    t_counts, c = clock(lambda: dev.stats_group_counts(slots, np.array([0, n], np.int64))[0][0])
    t_table, (val, used) = clock(lambda: Q.grm_values(c, n))
    mask = mask_words(np.flatnonzero(used))
    t_grm, G = clock(lambda: dev.grm(val, slots, mask))
    return dict(counts_s=t_counts, table_s=t_table, grm_s=t_grm,
                kernel_ms=dev.grm_info()['kernel_ms'], n_loci=int(used.sum())), G, val, used


def mask_words_of(dev):
    def f(loci):
        m = np.zeros(dev.W64, np.uint64)
        np.bitwise_or.at(m, loci >> 6, np.uint64(1) << (loci & 63).astype(np.uint64))
        return m
    return f


def rates(n, L_used, ms):
    full, tri = 2.0 * n * n * L_used, 1.0 * n * (n + 128) * L_used
    s = ms * 1e-3
    return dict(tflops_full_matrix=full / s / 1e12, tflops_computed_tiles=tri / s / 1e12,
                share_f32_matrix_peak=tri / s / F32_MATRIX_PEAK,
                share_untuned_f32_gemm=tri / s / F32_GEMM_UNTUNED)


def part_metric(n, reps):
    dev, cfg = setup('c4_metric')
    L = cfg['L']
    slots = np.random.RandomState(0).choice(dev.N, n, replace=False).astype(np.int64)
    mw = mask_words_of(dev)
    first, G, val, used = device_route(dev, slots, mw)        # the warm-up
    emit(workload='c4_metric', what='first_call', n=n, L=L, **first)
    mask = mw(np.flatnonzero(used))
    ms, wall = [], []
    for _ in range(reps):
        t, G2 = clock(lambda: dev.grm(val, slots, mask))
        wall.append(t)
        ms.append(dev.grm_info()['kernel_ms'])
    assert (G2 == G).all() and (G == G.T).all()
    emit(workload='c4_metric', what='gnx_grm', n=n, L=L, n_loci=int(used.sum()),
         kernel_ms=[round(x, 3) for x in ms], kernel_ms_best=min(ms),
         call_s=[round(x, 3) for x in wall], diag_mean=float(np.diag(G).mean()),
         **rates(n, int(used.sum()), min(ms)))
    for mode, what in ((1, 'expansion_alone'), (2, 'mfma_alone')):
        dev.grm_probe(mode)
        pm = []
        for _ in range(2):
            dev.grm(val, slots, mask)
            pm.append(dev.grm_info()['kernel_ms'])
        dev.grm_probe(0)
        emit(workload='c4_metric', what=what, kernel_ms=[round(x, 3) for x in pm],
             share_of_kernel=min(pm) / min(ms))
    t = [clock(lambda: dev.geno_gram(slots))[0] for _ in range(3)]
    emit(workload='c4_metric', what='gnx_geno_gram', n=n, L=L, call_s=[round(x, 3) for x in t[1:]])
    # the host side of calc_heritability on this matrix, for a synthetic response
    rng = np.random.RandomState(1)
    t_eigh, (evals, U) = clock(lambda: Q.eig_grm(G))
    y = U @ (rng.standard_normal(n) * np.sqrt(0.5 * np.maximum(evals, 0) + 0.5))
    t_reml, fit = clock(lambda: Q.reml(evals, U, y))
    t_he, he = clock(lambda: Q.he_regression(G, y))
    emit(workload='c4_metric', what='heritability_parts', n=n, grm_s=first['counts_s']
         + first['table_s'] + min(wall), eigh_s=t_eigh, reml_s=t_reml, he_s=t_he,
         h2=fit['h2'], se_h2=fit['se_h2'], he_h2=he)
    dev.close()


def host_route(dev, cfg, slots):
    """the parent commit's only route: download the sample's genomes, unpack, numpy in fp64"""
    L = cfg['L']
    t0 = time.perf_counter()
    packed = dev.download_genomes(slots)
    t1 = time.perf_counter()
    by = np.ascontiguousarray(packed).view(np.uint8).reshape(packed.shape[0], 2, -1)
    bits = np.unpackbits(by, axis=2, bitorder='little')[:, :, :L]
    D = (bits[:, 0] + bits[:, 1]).astype(np.float64)
    del bits, by
    t2 = time.perf_counter()
    n = D.shape[0]
    p = D.sum(0) / (2.0 * n)
    used = (p > 0) & (p < 1) & (np.minimum(p, 1 - p) >= 0.01)
    Z = (D[:, used] - 2 * p[used]) / np.sqrt(2 * p[used] * (1 - p[used]) * used.sum())
    G = Z @ Z.T
    t3 = time.perf_counter()
    return (t1 - t0, t2 - t1, t3 - t2, t3 - t0), G


def part_c2(n):
    dev, cfg = setup('c2')
    slots = np.random.RandomState(0).choice(dev.N, n, replace=False).astype(np.int64)
    mw = mask_words_of(dev)
    device_route(dev, slots, mw)                               # warm-up
    d_t, h_t = [], []
    for r in range(3):
        t0 = time.perf_counter()
        parts, G, _, used = device_route(dev, slots, mw)
        d_t.append(time.perf_counter() - t0)
        t, Gh = host_route(dev, cfg, slots)
        h_t.append(t[3])
        emit(workload='c2', what='repeat', r=r, n=n, L=cfg['L'], device_s=round(d_t[-1], 4),
             host_download_s=round(t[0], 3), host_unpack_s=round(t[1], 3),
             host_grm_s=round(t[2], 3), host_total_s=round(t[3], 3),
             max_abs_diff=float(np.abs(G - Gh).max()), **parts,
             **rates(n, parts['n_loci'], parts['kernel_ms']))
    d, h = np.array(d_t), np.array(h_t)
    emit(workload='c2', what='device_vs_host', n=n, device_s_median=float(np.median(d)),
         device_s_spread=[float(d.min()), float(d.max())], host_s_median=float(np.median(h)),
         host_s_spread=[float(h.min()), float(h.max())],
         ratio_host_over_device=float(np.median(h) / np.median(d)))
    dev.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['metric', 'c2'], required=True)
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    import torch
    torch.cuda.init()           # torch's HIP runtime first, the library's handles behind it (bench.py)
    part_metric(a.n, a.reps) if a.part == 'metric' else part_c2(a.n)
