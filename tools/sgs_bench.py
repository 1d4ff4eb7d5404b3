"""Model.calc_spatial_structure on the device (csrc/gnx_sgs.hip, sim/sgs.py): one JSON line per
measurement.

    python tools/sgs_bench.py                        # c3: 10^5 individuals, L = 10^5
    tools/kstat_cmd.sh r22_sgs tools/sgs_bench.py    # the same under rocprofv3: kernel times

bench.py's population walked a few steps (blocks shared with parents), all loci.
gnx_sgs_sums is synchronous and ends with its downloads (host clock around it).  Per max_dist
(ten classes equal in ln r from 1 to max_dist, every living individual): the call that only
asks for the work (cell sort, the cells' row ranges to the host, the count), the whole call,
and the candidate pair-words per second of the difference - gather, k_sgs_self, the task list
and k_sgs_pairs together, a lower bound of the pair kernel's rate; the kernel's own time comes
from the rocprofv3 run.  `tile_pair_words` is what the 64 x 64 tiles of the task list work off
(rows past a cell's end are padding): its ratio to the candidate pair-words is the share of the
tiles that holds pairs.  Then a random sample of 8192 individuals with one class covering every
pair (one cell: every tile of the triangle is full) beside gnx_geno_gram on the same sample,
the one existing kernel that does the same pair work (its call ends with the download of the
n x n int64 matrix, 512 MiB: compare the kernels' times of the rocprofv3 run).
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
from geonomics_amd.sim import sgs as G  # noqa: E402

BIG = 1 << 60


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


def tile_pair_words(x, y, side, W, H, nw):
    """what the task list of gnx_sgs_sums works off, recomputed on the host from the
    coordinates: 64 x 64 tiles of (cell, cell) and (cell, forward neighbour), times the words
    rounded up to the stage of 16"""
    ncx, ncy = max(1, int(np.ceil(W / side))), max(1, int(np.ceil(H / side)))
    cx = np.clip(np.floor(x.astype(np.float64) / side), 0, ncx - 1).astype(np.int64)
    cy = np.clip(np.floor(y.astype(np.float64) / side), 0, ncy - 1).astype(np.int64)
    cnt = np.bincount(cy * ncx + cx, minlength=ncx * ncy).reshape(ncy, ncx)
    t = (cnt + 63) // 64
    tiles = (t * (t + 1) // 2).sum()
    pad = np.pad(t, ((0, 1), (1, 1)))
    for dx, dy in ((1, 0), (-1, 1), (0, 1), (1, 1)):
        tiles += (t * pad[dy:dy + ncy, 1 + dx:1 + dx + ncx]).sum()
    return int(tiles) * 4096 * ((nw + 15) // 16 * 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c3', choices=sorted(bench.WORKLOADS))
    ap.add_argument('--max-dist', type=float, nargs='+', default=[8.0, 32.0, 64.0])
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--reps', type=int, default=2)
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    cfg = bench.WORKLOADS[a.workload]
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(a.steps, False, True)
    N, L = dev.N, cfg['L']
    nw = (L + 63) // 64
    cnt1, _ = dev.stats_group_counts(np.arange(N), np.array([0, N]))
    pbar = G.locus_terms(cnt1[0], N)[0]
    x, y = dev.download(nat.F_X), dev.download(nat.F_Y)
    for md in a.max_dist:
        edges = G.default_edges(1.0, md, 10)
        t_work = timed(lambda: dev.sgs_sums(edges), a.reps)
        got = dev.sgs_sums(edges, None, None, pbar, None, BIG)
        t_all = timed(lambda: dev.sgs_sums(edges, None, None, pbar, None, BIG), a.reps, warm=0)
        rest = min(t_all) - min(t_work)
        tpw = tile_pair_words(x, y, md * (1.0 + 1e-6), cfg['W'], cfg['H'], nw)
        emit(workload=a.workload, what='sgs_sums', N=N, L=L, max_dist=md, words=nw,
             work_pair_words=got['work'], candidate_pairs=got['work'] // nw,
             pairs_in_classes=int(got['isums'][:, 0].sum()), n_zero=got['n_zero'],
             tile_pair_words=tpw, tile_fill=got['work'] / tpw,
             work_only_ms=[round(v * 1e3, 2) for v in t_work],
             call_ms=[round(v * 1e3, 2) for v in t_all],
             pair_words_per_s_at_least=got['work'] / rest,
             tile_pair_words_per_s_at_least=tpw / rest)
    # one class covering every pair of a sample of 8192, beside the Gram kernel
    n = 8192
    slots = np.sort(np.random.RandomState(1).choice(N, n, replace=False)).astype(np.int64)
    one = np.array([0.0, 4.0 * max(cfg['W'], cfg['H'])])
    got = dev.sgs_sums(one, slots, None, pbar, None, BIG)
    t_sgs = timed(lambda: dev.sgs_sums(one, slots, None, pbar, None, BIG), a.reps, warm=0)
    Gm = dev.geno_gram(slots)
    t_gram = timed(lambda: dev.geno_gram(slots), a.reps, warm=0)
    g = np.diag(Gm)
    iu = np.triu_indices(n, 1)
    same = (x[slots][iu[0]] == x[slots][iu[1]]) & (y[slots][iu[0]] == y[slots][iu[1]])
    want = int((g[iu[0]] + g[iu[1]] - 2 * Gm[iu])[~same].sum())
    emit(workload=a.workload, what='sgs_vs_gram', n=n, L=L, words=nw,
         work_pair_words=got['work'], pairs=int(got['isums'][0, 0]), n_zero=got['n_zero'],
         sgs_call_ms=[round(v * 1e3, 2) for v in t_sgs],
         gram_call_ms=[round(v * 1e3, 2) for v in t_gram],
         gram_bytes_to_host=n * n * 8, sgs_bytes_to_host=(33 * 3 + 32 * 7) * 8,
         pair_words_per_s_call=got['work'] / min(t_sgs),
         integer_sums_equal_gram=bool(int(got['isums'][0, 2] - 2 * got['isums'][0, 1]) == want))
    dev.close()


if __name__ == '__main__':
    main()
