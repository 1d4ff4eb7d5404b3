"""Model.calc_roh / calc_ibs_sharing on the device (csrc/gnx_tracts.hip, sim/tracts.py): one JSON
line per measurement, printed and written to profiles/r08_tracts.txt (--out).

    python tools/tracts_bench.py --workload c4_metric --steps 20 --no-pairs --no-parent
    python tools/tracts_bench.py --workload c2 --append

bench.py's population walked a few steps (blocks shared with parents), the map of a constant rate
1 / L between neighbours in units of 2^-32 Morgans.  The calls are synchronous and end with their
downloads: `call_ms` is the host clock around them, `kernel_ms` the HIP-event time of their
kernels (gnx_tracts_info).
  self    every living individual, min_loci 50 and 100 (the walked and the O(1) path of a word
          with differences).  bytes_read = the genome words the scan loaded (blocks that both
          homologues share are skipped) beside the bound 2 N L / 8, over the kernel time, beside
          gnx_measure_copy.
  pairs   n = 1024 and 4096 sampled individuals, min_loci 50 and 100: word steps (haplotype pairs
          x genome words) per second of kernel time.
  parent  the route without this call: download the genotypes of --parent-n individuals in chunks,
          unpack them and run the numpy restatement (brute_self); scaled to N for the ratio.
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
from geonomics_amd import _native as nat  # noqa: E402
from geonomics_amd.sim import tracts as TR  # noqa: E402

BIG = 1 << 60
LINES = []


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def timed(dev, fn, reps, warm=1):
    """-> (host seconds, kernel ms of gnx_tracts_info) of `reps` calls after `warm` warm-ups"""
    for _ in range(warm):
        fn()
    t, k = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
        k.append(dev.tracts_info()['kernel_ms'])
    return t, k


def ms(v):
    return [round(x * 1e3, 2) for x in v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c2', choices=sorted(bench.WORKLOADS))
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-pairs', action='store_true')
    ap.add_argument('--no-parent', action='store_true')
    ap.add_argument('--parent-n', type=int, default=20000)
    ap.add_argument('--append', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r08_tracts.txt'))
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    cfg = bench.WORKLOADS[a.workload]
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(a.steps, False, True)
    N, L = dev.N, cfg['L']
    pos, _, _ = TR.tract_map(np.r_[0.0, np.full(L - 1, 1.0 / L)], 'morgans')
    min_len = TR.to_units(0.0005, 'morgans')
    copy = nat.measure_copy(2 << 30, 5)
    emit(what='copy', gb_per_s=round(copy, 1))
    bound = 2 * N * ((L + 63) // 64) * 8

    for ml in (50, 100):
        got = dev.tracts_self(pos, None, ml, min_len)
        t, k = timed(dev, lambda: dev.tracts_self(pos, None, ml, min_len), a.reps, warm=0)
        info = dev.tracts_info()
        emit(workload=a.workload, what='self', N=N, L=L, steps=a.steps, min_loci=ml,
             min_len_morgans=0.0005, tracts=int(got['per'][:, 0].sum()),
             mean_f_roh=float(got['per'][:, 2].mean() / (pos[-1] - pos[0])), call_ms=ms(t),
             kernel_ms=[round(v, 3) for v in k], bytes_read=info['bytes_read'],
             bytes_bound=bound, read_share=round(info['bytes_read'] / bound, 4),
             gb_per_s=round(info['bytes_read'] / (min(k) * 1e-3) / 1e9, 1),
             gb_per_s_on_bound=round(bound / (min(k) * 1e-3) / 1e9, 1),
             copy_gb_per_s=round(copy, 1))
    t, k = timed(dev, lambda: dev.tracts_self(pos, None, 100, min_len,
                                              np.array([0, min_len, 4 * min_len, 2 ** 62]),
                                              None, True), a.reps, warm=0)
    emit(workload=a.workload, what='self, hist and cover', N=N, L=L, min_loci=100,
         call_ms=ms(t), kernel_ms=[round(v, 3) for v in k])

    if not a.no_pairs:
        rng = np.random.RandomState(1)
        for n in (1024, 4096):
            slots = np.sort(rng.choice(N, n, replace=False)).astype(np.int64)
            for ml in (50, 100):
                got = dev.tracts_pairs(pos, None, ml, min_len, None, slots, False, BIG)
                t, k = timed(dev, lambda: dev.tracts_pairs(pos, None, ml, min_len, None, slots,
                                                           False, BIG), a.reps, warm=0)
                emit(workload=a.workload, what='pairs', n=n, L=L, min_loci=ml,
                     work_word_steps=got['work'],
                     tracts=int(np.triu(got['cnt'], 1).sum()), call_ms=ms(t),
                     kernel_ms=[round(v, 3) for v in k],
                     word_steps_per_s=got['work'] / (min(k) * 1e-3))

    if not a.no_parent:
        import gnx_oracle as O
        m = min(a.parent_n, N)
        want = dev.tracts_self(pos, None, 100, min_len, None, np.arange(m, dtype=np.int64))
        t0 = time.perf_counter()
        per = []
        for lo in range(0, m, 2000):
            idx = np.arange(lo, min(m, lo + 2000), dtype=np.int64)
            g = O.unpack_genomes(dev.download_genomes(idx), L)          # [n][L][2]
            per.append(TR.brute_self(np.transpose(g, (0, 2, 1)), pos, None, 100,
                                     min_len)['per'])
        dt = time.perf_counter() - t0
        same = bool((np.concatenate(per) == want['per']).all())
        t, k = timed(dev, lambda: dev.tracts_self(pos, None, 100, min_len), a.reps, warm=0)
        emit(workload=a.workload, what='parent', individuals=m, N=N, L=L, equal=same,
             download_and_numpy_s=round(dt, 2), scaled_to_N_s=round(dt * N / m, 1),
             device_call_ms=ms(t), ratio=round(dt * N / m / min(t), 1))
    dev.close()
    head = ('# python tools/tracts_bench.py on one MI355X (%s: N = %d, L = %d, walked %d steps); '
            'host clock around the\n# synchronous calls and HIP-event kernel time '
            '(gnx_tracts_info), %d repetitions\n' % (a.workload, N, L, a.steps, a.reps))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a' if a.append else 'w') as f:
        f.write(head + '\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
