"""The device call behind Model.calc_ihs (csrc/gnx_sweeps.hip, sim/sweeps.py): one JSON line per
measurement, printed and written to profiles/r20_sweeps.txt (--out).

    python tools/sweeps_bench.py --workload c4_metric --steps 20 --n 1000

bench.py's population walked a few steps, a sample of n individuals, all loci, the map of a
constant rate 1 / L between neighbours in units of 2^-24 Morgans, min_maf 0.05, cutoff 0.05.
`kernel_ms` is the HIP-event time of the call's kernels (gnx_sweeps_info), `call_ms` the host
clock around the synchronous call.
  probe   max_work = 0: the bit transpose and c1 alone
  scan    the whole call; its kernel time less the probe's is the scan kernel's
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import bench  # noqa: E402
from geonomics_amd.sim import ld as LD  # noqa: E402
from geonomics_amd.sim import sweeps as SW  # noqa: E402

LINES = []


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def timed(dev, fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t, k = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(round((time.perf_counter() - t0) * 1e3, 3))
        k.append(round(dev.sweeps_info()['kernel_ms'], 3))
    return t, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c4_metric', choices=sorted(bench.WORKLOADS))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--n', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r20_sweeps.txt'))
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    cfg = bench.WORKLOADS[a.workload]
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(a.steps, False, True)
    N, L = dev.N, cfg['L']
    slots = np.sort(np.random.RandomState(1).choice(N, a.n, replace=False)).astype(np.int64)
    pos, brk, scale = SW.sweep_map(np.r_[0.0, np.full(L - 1, 1.0 / L)], 'morgans')
    loci = np.arange(L)
    num, den = SW.cutoff_fraction(0.05)
    mm = max(2, LD.min_minor(0.05, 2 * a.n))
    kw = dict(slots=slots, min_minor=mm, cut_num=num, cut_den=den)
    t, k = timed(dev, lambda: dev.sweeps_scan(loci, pos, brk, max_work=0, **kw), a.reps)
    emit(workload=a.workload, what='probe', N=N, L=L, n=a.n, steps=a.steps, call_ms=t,
         kernel_ms=k, kernel_ms_median=float(np.median(k)))
    probe = float(np.median(k))
    got = dev.sweeps_scan(loci, pos, brk, max_work=1 << 60, **kw)
    t, k = timed(dev, lambda: dev.sweeps_scan(loci, pos, brk, max_work=1 << 60, **kw), a.reps)
    info = dev.sweeps_info()
    kept = SW.kept_loci(got['c1'], 2 * a.n, mm)
    st = got['status'][kept]
    med = float(np.median(k))
    emit(workload=a.workload, what='scan', N=N, L=L, n=a.n, min_minor=mm, kept=int(kept.sum()),
         work=got['work'], steps_total=info['steps_total'], launches=info['launches'],
         mean_steps=round(float(got['steps'][kept].mean()), 2),
         share_cutoff=round(float((st == 0).mean()), 4), call_ms=t, kernel_ms=k,
         kernel_ms_median=med, kernel_ms_spread=[min(k), max(k)],
         scan_kernel_ms=round(med - probe, 3), transpose_ms=round(probe, 3),
         scan_share=round((med - probe) / med, 4),
         steps_per_s=round(info['steps_total'] / ((med - probe) * 1e-3)))
    dev.close()
    head = ('# python tools/sweeps_bench.py on one MI355X (%s: N = %d, L = %d, walked %d steps, '
            'sample n = %d);\n# HIP-event kernel time (gnx_sweeps_info) and host clock, %d '
            'repetitions after 2 warm-ups\n' % (a.workload, N, L, a.steps, a.n, a.reps))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(head + '\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
