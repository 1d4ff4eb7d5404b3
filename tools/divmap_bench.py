"""gnx_divmap_sums (csrc/gnx_divmap.hip) on the metric population: one JSON line per measurement.

    python tools/divmap_bench.py                      # c4_metric: (a) 8 x 8 win 1, (b) 64 x 64 win 5
    python tools/divmap_bench.py --out profiles/divmap_bench.txt
    tools/kstat_cmd.sh divmap_b tools/divmap_bench.py --case b --no-copy
                                                  # under rocprofv3: the kernels' own times

bench.py's metric population (10^6 individuals, L = 10^5) after bench.py's warm-up of 10 steps.
Map cells are the rectangles of an nx x ny grid over the landscape (what Species._group_by_grid
gives), everybody in a cell.  Every call here is synchronous and ends with its downloads, so the
host clock around the call is the call: 2 warm-ups, then `reps` calls; min, median and the
spread (max - min) / median are reported.
  (a) an 8 x 8 map, win = 1: the new call + sim/divmap.window_stats against the route the parent
      commit has for the same numbers, gnx_stats_group_counts on the same grouping +
      sim/fst.diversity (G L = 6.4 10^6 counts per table, within its limits).  The integers of
      both routes are compared.
  (b) a 64 x 64 map, win = 5: the call the parent commit cannot make (4096 groups).
Each rate is the genome bytes stage A must read, 2 n W64 8, over the time, and that as a
fraction of the library's copy rate (gnx_measure_copy, read + write bytes).
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
from geonomics_amd.sim import divmap as DM  # noqa: E402
from geonomics_amd.sim import fst as F  # noqa: E402

LINES = []


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return np.array(t)


def summary(t, nbytes, copy_gbps):
    med = float(np.median(t))
    out = dict(min_ms=round(float(t.min()) * 1e3, 3), median_ms=round(med * 1e3, 3),
               spread=round(float(t.max() - t.min()) / med, 3), reps=int(t.size),
               gbytes_per_s=round(nbytes / float(t.min()) / 1e9, 1))
    if copy_gbps:
        out['fraction_of_copy_rate'] = round(out['gbytes_per_s'] / copy_gbps, 3)
    return out


def grouped(x, y, cfg, nx, ny):
    lab = np.clip((y * (ny / cfg['H'])).astype(np.int64), 0, ny - 1) * nx + \
        np.clip((x * (nx / cfg['W'])).astype(np.int64), 0, nx - 1)
    order = np.argsort(lab, kind='stable')
    return order, np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=nx * ny))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c4_metric', choices=sorted(bench.WORKLOADS))
    ap.add_argument('--warmup-steps', type=int, default=10)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--no-copy', action='store_true', help='skip the copy-rate measurement')
    ap.add_argument('--case', default='ab', choices=['a', 'b', 'ab'], help='which measurements')
    ap.add_argument('--out', default=None, help='also write the lines to this text file')
    a = ap.parse_args()
    cfg = bench.WORKLOADS[a.workload]
    copy_gbps = None if a.no_copy else bench.measured_copy_bandwidth()
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(a.warmup_steps, False, True)
    N, L, W64 = dev.N, cfg['L'], dev.W64
    nbytes = 2 * N * W64 * 8
    emit(workload=a.workload, what='population', N=N, L=L, W64=W64, genome_bytes=nbytes,
         copy_gbytes_per_s=copy_gbps, blocks=dev.genome_info()['NB'])
    x, y = dev.download(nat.F_X).astype(np.float64), dev.download(nat.F_Y).astype(np.float64)

    if 'a' in a.case:
        case_a(dev, a, cfg, x, y, nbytes, copy_gbps)
    if 'b' in a.case:
        case_b(dev, a, cfg, x, y, nbytes, copy_gbps)
    dev.close()
    if a.out:
        head = ('# tools/divmap_bench.py --workload %s: N = %d, L = %d; host clock around the '
                'synchronous calls, %d repetitions after 2 warm-ups\n' % (a.workload, N, L, a.reps))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(head + '\n'.join(LINES) + '\n')


def case_a(dev, a, cfg, x, y, nbytes, copy_gbps):
    """8 x 8, win = 1: both routes to the same numbers"""
    L = cfg['L']
    order, cs = grouped(x, y, cfg, 8, 8)
    new, old = {}, {}

    def new_route():
        new['sums'] = dev.divmap_sums(order, cs, 8, 8, 0)
        s = new['sums']
        new['stats'] = DM.window_stats(s['n'], s['S'], s['sum_het'], s['sum_cc'], L)

    def old_route():
        old['c'] = dev.stats_group_counts(order, cs)
        old['stats'] = F.diversity(old['c'][0], old['c'][1], np.diff(cs))
    t_new = timed(new_route, a.reps)
    t_old = timed(old_route, a.reps)
    c1, ch = (c.astype(np.int64) for c in old['c'])
    m = 2 * np.diff(cs)[:, None]
    same = bool((new['sums']['S'].ravel() == ((c1 > 0) & (c1 < m)).sum(axis=1)).all()
                and (new['sums']['sum_het'].ravel() == ch.sum(axis=1)).all()
                and (new['sums']['sum_cc'].ravel() == (c1 * (m - c1)).sum(axis=1)).all())
    rel = float(np.nanmax(np.abs(new['stats']['pi'].ravel() - old['stats']['pi'])
                          / old['stats']['pi']))
    emit(workload=a.workload, what='(a) gnx_divmap_sums + window_stats', grid=[8, 8], win=1,
         info=dev.divmap_info(), bytes_to_host=24 * 64, **summary(t_new, nbytes, copy_gbps))
    emit(workload=a.workload, what='(a) gnx_stats_group_counts + fst.diversity', G=64,
         bytes_to_host=8 * 64 * L, **summary(t_old, nbytes, copy_gbps))
    emit(workload=a.workload, what='(a) new over old', integers_equal=same,
         pi_max_rel_diff=rel, median_ratio=round(float(np.median(t_new) / np.median(t_old)), 3),
         min_ratio=round(float(t_new.min() / t_old.min()), 3))


def case_b(dev, a, cfg, x, y, nbytes, copy_gbps):
    """64 x 64, win = 5"""
    N = dev.N
    order, cs = grouped(x, y, cfg, 64, 64)
    got = {}

    def big():
        got['sums'] = dev.divmap_sums(order, cs, 64, 64, 2)
    t = timed(big, a.reps)
    s = got['sums']
    ok = bool((s['n'] == DM.box_sum(np.diff(cs).reshape(64, 64), 2)).all())
    emit(workload=a.workload, what='(b) gnx_divmap_sums', grid=[64, 64], win=5,
         info=dev.divmap_info(), cell_sizes=[int(np.diff(cs).min()), int(np.diff(cs).max())],
         window_sizes=[int(s['n'].min()), int(s['n'].max())], n_equals_box_sum=ok,
         S_range=[int(s['S'].min()), int(s['S'].max())], bytes_to_host=24 * 4096,
         bytes_from_host=4 * N, **summary(t, nbytes, copy_gbps))


if __name__ == '__main__':
    main()
