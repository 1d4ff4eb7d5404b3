"""Model.calc_ld_decay on the device (csrc/gnx_ld.hip, sim/ld.py): one JSON line per
measurement, printed and written to profiles/r16_ld.txt (--out).

    python tools/ld_bench.py                         # c2: 10^5 individuals, L = 10^4

bench.py's population walked a few steps (blocks shared with parents), every living individual,
the map of a constant rate 1 / L between neighbours.  gnx_ld_bins is synchronous and ends with
its downloads: `call_ms` is the host clock around it, `kernel_ms` the HIP-event time of its
kernels (gnx_ld_info).
  transpose   a request whose bins no pair falls in lists no tile: the call is pass 1 alone
              (memset, k_ld_bits, k_ld_rowsum).  Its bytes - the genome lines read once, the bit
              rows written twice (memset, then the words) and read once - over its kernel time,
              beside gnx_measure_copy.
  full        every pair of loci, 20 bins of c.  popcount words per second = listed tiles x
              4096 x chromosome words over (kernel time - the transpose's).
  band        the same up to c = 0.05.
  vs_stats_ld 8192 loci, one bin, beside gnx_stats_ld (the reference's _calc_ld pair by pair,
              whose call ends with the download of the 8192 x 8192 fp64 matrix).
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
from geonomics_amd.sim import ld as LD  # noqa: E402

BIG = 1 << 60
LINES = []


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def timed(dev, fn, reps, warm=1):
    """-> (host seconds, kernel ms of gnx_ld_info) of `reps` calls after `warm` warm-ups"""
    for _ in range(warm):
        fn()
    t, k = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
        k.append(dev.ld_info()['kernel_ms'])
    return t, k


def ms(v):
    return [round(x * 1e3, 2) for x in v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c2', choices=sorted(bench.WORKLOADS))
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_ld.txt'))
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    cfg = bench.WORKLOADS[a.workload]
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(a.steps, False, True)
    N, L = dev.N, cfg['L']
    n_chrom = 2 * N
    nq = (n_chrom + 63) // 64
    loci = np.arange(L)
    pos = LD.map_positions(np.r_[0.0, np.full(L - 1, 1.0 / L)])
    mm = LD.min_minor(0.05, n_chrom)
    copy = nat.measure_copy(2 << 30, 5)
    emit(what='copy', gb_per_s=round(copy, 1))

    # pass 1 alone
    none = np.array([1e9, 2e9])
    t, k = timed(dev, lambda: dev.ld_bins(loci, pos, none, None, mm, True, BIG), a.reps)
    lines = np.unique(loci >> 10).size
    t_bytes = L * ((nq + 15) // 16 * 16) * 8
    moved = n_chrom * lines * 128 + 3 * t_bytes
    k1 = min(k)
    emit(workload=a.workload, what='transpose', N=N, L=L, chromosome_words=nq,
         genome_bytes_read=n_chrom * lines * 128, bit_row_bytes=t_bytes, call_ms=ms(t),
         kernel_ms=[round(v, 3) for v in k], info=dev.ld_info(),
         gb_per_s=round(moved / (k1 * 1e-3) / 1e9, 1), copy_gb_per_s=round(copy, 1))

    for what, edges in (('full', LD.default_edges('c', 20)),
                        ('band', LD.default_edges('c', 20, 0.05))):
        e = LD.c_to_morgans(edges)
        got = dev.ld_bins(loci, pos, e, None, mm, True, BIG)
        t, k = timed(dev, lambda: dev.ld_bins(loci, pos, e, None, mm, True, BIG), a.reps,
                     warm=0)
        words = got['work'] * 4096
        emit(workload=a.workload, what=what, N=N, L=L, chromosome_words=nq,
             kept=int((np.minimum(got['c1'], n_chrom - got['c1']) >= mm).sum()),
             work_tile_words=got['work'], tiles=got['work'] // nq, pairs=int(got['pairs'].sum()),
             call_ms=ms(t), kernel_ms=[round(v, 3) for v in k], info=dev.ld_info(),
             popcount_words=words,
             popcount_words_per_s=words / max((min(k) - k1) * 1e-3, 1e-9),
             mean_r2=[float('%.6g' % v) for v in got['sum_r2'] / np.maximum(got['pairs'], 1)])

    # 8192 loci, one bin, beside the older path
    n = min(8192, L)
    sub = np.sort(np.random.RandomState(1).choice(L, n, replace=False))
    one = np.array([0.0, np.inf])
    got = dev.ld_bins(sub, pos[sub], one, None, 1, True, BIG)
    t_new, k_new = timed(dev, lambda: dev.ld_bins(sub, pos[sub], one, None, 1, True, BIG),
                         a.reps, warm=0)
    old = dev.stats_ld(sub)
    t_old = []
    for _ in range(max(1, a.reps - 1)):
        t0 = time.perf_counter()
        dev.stats_ld(sub)
        t_old.append(time.perf_counter() - t0)
    v = old[np.triu_indices(n, 1)]
    ok = np.isfinite(v)
    mean_new = got['sum_r2'][0] / got['pairs'][0]
    emit(workload=a.workload, what='vs_stats_ld', n_loci=n, N=N, chromosome_words=nq,
         pairs=int(got['pairs'][0]), old_finite_pairs=int(ok.sum()),
         new_call_ms=ms(t_new), new_kernel_ms=[round(x, 3) for x in k_new],
         old_call_ms=ms(t_old), old_bytes_to_host=n * n * 8,
         old_over_new=round(min(t_old) / min(t_new), 2),
         mean_r2_new=mean_new, mean_r2_old=float(v[ok].mean()),
         rel_diff=abs(mean_new - v[ok].mean()) / v[ok].mean())
    dev.close()
    with open(a.out, 'w') as f:
        f.write('# python tools/ld_bench.py on one MI355X (%s: N = %d, L = %d, walked %d steps); '
                'host clock around the\n# synchronous calls and HIP-event kernel time '
                '(gnx_ld_info), %d repetitions\n' % (a.workload, N, L, a.steps, a.reps))
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
