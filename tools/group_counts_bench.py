"""gnx_stats_group_counts (csrc/gnx_group_counts.hip) on the metric population: one JSON line per
measurement.

    python tools/group_counts_bench.py                            # c4_metric, G = 1, 4, 64
    tools/kstat_cmd.sh r08_gc tools/group_counts_bench.py --groups 1 --no-copy
                                                  # under rocprofv3: the kernels' own times

bench.py's metric population (10^6 individuals, L = 10^5) after bench.py's warm-up of 10 steps.
Groups are the rectangles of an nx x ny grid over the landscape (what Species._group_by_grid
gives), G = nx * ny, everybody in a group.  gnx_stats_group_counts and gnx_stats_locus_counts -
the parent commit's only route to such counts, and only for everybody at once - are both
synchronous and end with their downloads, so the host clock around the call is the call:
2 warm-ups, then `reps` calls; min, median and the spread (max - min) / median are reported.
The call includes the host's check of the slots, their upload (4 n bytes) and the download of
the two tables (8 G L bytes); the kernel alone is in the rocprofv3 run.  Each rate is the
genome bytes the kernel must read, 2 n W64 8, over the time, and that as a fraction of the
library's copy rate (gnx_measure_copy, read + write bytes).
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
from geonomics_amd.sim import fst as F  # noqa: E402

GRIDS = {1: (1, 1), 4: (2, 2), 64: (8, 8), 1024: (32, 32)}


def emit(**kw):
    print(json.dumps(kw), flush=True)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c4_metric', choices=sorted(bench.WORKLOADS))
    ap.add_argument('--groups', default='1,4,64')
    ap.add_argument('--warmup-steps', type=int, default=10)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--no-copy', action='store_true', help='skip the copy-rate measurement')
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
    ref = {}

    def locus():
        ref['c'] = dev.stats_locus_counts()
    t = timed(locus, a.reps)
    emit(workload=a.workload, what='gnx_stats_locus_counts', **summary(t, nbytes, copy_gbps))
    x, y = dev.download(nat.F_X).astype(np.float64), dev.download(nat.F_Y).astype(np.float64)
    for G in (int(g) for g in a.groups.split(',')):
        nx, ny = GRIDS[G]
        lab = np.clip((y * (ny / cfg['H'])).astype(np.int64), 0, ny - 1) * nx + \
            np.clip((x * (nx / cfg['W'])).astype(np.int64), 0, nx - 1)
        _, order, gs = F.make_groups(np.arange(N), lab)       # slots stand in for the ids
        got = {}

        def group():
            got['c'] = dev.stats_group_counts(order, gs)
        t = timed(group, a.reps)
        ok = bool((got['c'][0].sum(axis=0) == ref['c'][0]).all()
                  and (got['c'][1].sum(axis=0) == ref['c'][1]).all())
        emit(workload=a.workload, what='gnx_stats_group_counts', G=G,
             group_sizes=[int(np.diff(gs).min()), int(np.diff(gs).max())],
             sums_equal_locus_counts=ok, bytes_to_host=8 * G * L, bytes_from_host=4 * N,
             **summary(t, nbytes, copy_gbps))
    dev.close()


if __name__ == '__main__':
    main()
