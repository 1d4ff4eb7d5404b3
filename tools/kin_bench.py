"""Model.calc_relatedness / find_kin on the device (csrc/gnx_kin.hip, sim/kin.py): one JSON line
per measurement, to stdout and to profiles/kin_bench.txt (--out).

    python tools/kin_bench.py                          # c4_metric: 10^6 individuals, L = 10^5
    tools/kstat_cmd.sh kin tools/kin_bench.py          # the same under rocprofv3: kernel times

bench.py's population walked a few steps (blocks shared with parents), all loci.

(a) gnx_kin_matrix beside gnx_geno_gram on one random sample of 8192 individuals: the same
64 x 64 LDS-staged popcount tile over the same n (n + 64) / 2 pairs x words, three popcounts per
pair-word against four, two int accumulators per pair against one.  Both calls are synchronous
and end with a download of 512 MiB (two int32 matrices; one int64 matrix), so the host clock
around them compares like with like; the calls alternate.  gnx_kin_info gives the HIP-event time
of the matrix call's kernels (gather, nhet, tiles).  `tile_pair_words` is what the kernels work
off: the 64 x 64 tiles of the upper triangle, diagonal included, times the words rounded up to
the stage of 16.

(b) gnx_kin_pairs over every living individual at one max_dist and KING's second-degree
threshold: the call that only asks for the work (cell sort, the cells' ranges to the host, the
count), the whole call, gnx_kin_info's event time, and candidate pair-words per second of the
event time less the cell sort.
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
from geonomics_amd.sim import kin as K  # noqa: E402

BIG = 1 << 60


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c4_metric', choices=sorted(bench.WORKLOADS))
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--max-dist', type=float, default=16.0)
    ap.add_argument('--min-kinship', type=float, default=2 ** -3.5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kin_bench.txt'))
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    cfg = bench.WORKLOADS[a.workload]
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(a.steps, False, True)
    N, L = dev.N, cfg['L']
    nw = (L + 63) // 64
    lines = ['# tools/kin_bench.py --workload %s: N = %d, L = %d, walked %d steps; host clock '
             'around the synchronous calls and HIP events around their kernels (gnx_kin_info), '
             '%d repetitions after one warm-up' % (a.workload, N, L, a.steps, a.reps)]

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def clock(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    # (a) the matrix beside the Gram matrix, alternating
    n = min(a.n, N)
    slots = np.sort(np.random.RandomState(1).choice(N, n, replace=False)).astype(np.int64)
    M = dev.kin_matrix(slots)
    Gm = dev.geno_gram(slots)
    t_kin, t_gram, k_ms = [], [], []
    for _ in range(a.reps):
        t_kin.append(clock(lambda: dev.kin_matrix(slots))[0])
        k_ms.append(dev.kin_info()['kernel_ms'])
        t_gram.append(clock(lambda: dev.geno_gram(slots))[0])
    tiles = (n + 63) // 64
    tiles = tiles * (tiles + 1) // 2
    tpw = tiles * 4096 * ((nw + 15) // 16 * 16)
    # the two matrices agree where they overlap: the dosage product of two heterozygous loci is
    # 1, so G_ab >= hh_ab, and G_aa = nhet_a + 4 (homozygous-1 loci of a)
    kin = K.king(M['hh'], M['ibs0'], M['nhet'][:, None], M['nhet'][None, :])
    iu = np.triu_indices(n, 1)
    emit(workload=a.workload, what='(a) gnx_kin_matrix beside gnx_geno_gram', n=n, L=L, words=nw,
         tiles=tiles, tile_pair_words=tpw, pair_words=n * (n - 1) // 2 * nw,
         kin_call_ms=[round(v, 2) for v in t_kin], gram_call_ms=[round(v, 2) for v in t_gram],
         kin_kernel_ms=[round(v, 2) for v in k_ms], bytes_to_host_each=n * n * 8,
         call_ratio_kin_over_gram=round(min(t_kin) / min(t_gram), 3),
         kin_tile_pair_words_per_s=tpw / (min(k_ms) * 1e-3),
         gram_kernel_ms_estimate=round(min(t_gram) - (min(t_kin) - min(k_ms)), 2),
         hh_le_gram=bool((M['hh'] <= Gm).all()),
         diag_consistent=bool(((np.diag(Gm) - M['nhet']) % 4 == 0).all()),
         kinship_off_diagonal=[float(np.nanmin(kin[iu])), float(np.nanmedian(kin[iu])),
                               float(np.nanmax(kin[iu]))])
    del M, Gm, kin

    # (b) the pair list over everybody
    T = K.threshold(a.min_kinship)
    md = a.max_dist
    t_work = [clock(lambda: dev.kin_pairs(T, md))[0] for _ in range(a.reps + 1)][1:]
    sort_ms = dev.kin_info()['kernel_ms']
    got = dev.kin_pairs(T, md, None, None, 1 << 24, BIG)
    t_all, k_ms = [], []
    for _ in range(a.reps):
        t_all.append(clock(lambda: dev.kin_pairs(T, md, None, None, 1 << 24, BIG))[0])
        k_ms.append(dev.kin_info()['kernel_ms'])
    info = dev.kin_info()
    tpw = info['tasks'] * 4096 * ((nw + 15) // 16 * 16)
    rel = K.relationship(K.king(got['hh'], got['ibs0'], got['nhet'][got['pa']],
                                got['nhet'][got['pb']]), got['ibs0'])
    names, counts = np.unique(rel, return_counts=True)
    rest = (min(k_ms) - sort_ms) * 1e-3
    emit(workload=a.workload, what='(b) gnx_kin_pairs over everybody', N=N, L=L, words=nw,
         max_dist=md, min_kinship=a.min_kinship, T=T, work_pair_words=got['work'],
         cell_pairs=got['work'] // nw, n_candidates=got['n_candidates'], n_found=got['n_found'],
         relationships=dict(zip(names.tolist(), counts.tolist())), info=info,
         tile_pair_words=tpw, tile_fill=got['work'] / tpw,
         work_only_ms=[round(v, 2) for v in t_work], cell_sort_kernel_ms=round(sort_ms, 3),
         call_ms=[round(v, 2) for v in t_all], kernel_ms=[round(v, 2) for v in k_ms],
         pair_words_per_s=got['work'] / rest, tile_pair_words_per_s=tpw / rest)
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
