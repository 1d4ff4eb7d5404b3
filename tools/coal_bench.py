"""Pairwise coalescence through the recorded pedigree (csrc/gnx_coal.hip, sim/coal.py): one JSON
line per measurement.

    python tools/coal_bench.py                      # the model of tools/lineage_bench.py

The 'use_tskit': True model of tools/lineage_bench.py (~9 x 10^4 individuals, L = 1000, 200 main
steps, the pedigree never simplified) is burned in and walked.  Then, for a request of `--nodes`
sample nodes (512: both homologues of 256 living individuals) x all loci, once for individuals
drawn at random over the landscape and once for the individuals nearest to its centre (whose
lineages meet far more often):

  times      gnx_coal_times for the pair and locus sums and the histogram of T: the kernels' own
             time (HIP events around every launch, gnx_lineage_info), the call's host clock, the
             (pair, locus) cells per second of kernel time; without an age limit and with
             `--max-ago`; every call is made `--reps` times after one warm-up call (the very
             first call of the run also uploads the node table), median (min-max) of the
             kernel time
  segments   gnx_coal_segments on the architecture's map (sim/tracts.tract_map), with cover and a
             histogram, same limits
  host       sim/coal.coal_times_np (the numpy restatement) on `--host-nodes` of the nodes x
             `--host-loci` loci, its time scaled by cells to the full request, and whether the
             device equals it
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    from lineage_bench import params
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=420, help='landscape side (K = 0.5 per cell)')
    ap.add_argument('--N', type=int, default=85000)
    ap.add_argument('--L', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--r', type=float, default=2e-3)
    ap.add_argument('--nodes', type=int, default=512)
    ap.add_argument('--max-ago', type=int, default=50)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-nodes', type=int, default=24)
    ap.add_argument('--host-loci', type=int, default=20)
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    import geonomics_amd as gnx
    from geonomics_amd.sim import coal as CO
    from geonomics_amd.sim import tracts as TR
    warnings.simplefilter('ignore')
    mod = gnx.make_model(params(a.side, a.N, a.L, a.steps, a.r, 19))
    spp = mod.comm[0]
    mod.walk(10000, 'burn', verbose=False)
    if spp._tt is None:
        raise SystemExit('no pedigree was recorded; lower --side')
    mod.walk(a.steps, 'main', verbose=False)
    tt, dev = spp._tt, spp._dev
    tab, bt = tt.node_table()
    ids = np.array([*spp])
    xy = spp._get_coords()
    loci = np.arange(a.L)
    rec = spp.gen_arch.recombinations
    rates = np.zeros(a.L)
    rates[rec._positions] = rec._rates
    pos, brk, _ = TR.tract_map(rates, 'morgans')
    n_ind = a.nodes // 2
    emit(what='model', living=int(ids.size), pedigree_rows=int(bt.size), loci=a.L,
         main_steps=a.steps, sample_nodes=2 * n_ind, pairs=CO.n_pairs(2 * n_ind),
         cells=CO.n_pairs(2 * n_ind) * a.L)
    rng = np.random.RandomState(0)
    centre = np.argsort(((xy - a.side / 2.0) ** 2).sum(axis=1), kind='stable')[:n_ind]
    samples = (('random', np.sort(rng.choice(ids.size, n_ind, replace=False))),
               ('centre', np.sort(centre)))
    tedges = np.unique(np.rint(np.linspace(0, a.steps + 2, 41)).astype(np.int64))
    big = 1 << 60

    def timed(call):
        """-> (the last result, host seconds of the last call, kernel ms median / min / max)"""
        call()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = call()
            t = time.perf_counter() - t0
            ms.append(dev.lineage_info()['kernel_ms'])
        return got, t, dict(kernel_ms=round(float(np.median(ms)), 3),
                            kernel_ms_min=round(min(ms), 3), kernel_ms_max=round(max(ms), 3))

    for name, pick in samples:
        rows = np.searchsorted(tt.ids, ids[pick])
        nodes = np.stack([2 * rows, 2 * rows + 1], 1).ravel()
        for max_ago in (None, a.max_ago):
            got, t, ms = timed(lambda: dev.coal_times(tab, bt, nodes, loci, spp.t, max_ago,
                                                      tedges, max_work=big))
            hit = int(got['locus_cnt'].sum())
            emit(what='times', sample=name, max_ago=max_ago, call_s=round(t, 4),
                 launches=dev.lineage_info()['launches'], share_coalesced=hit / got['work'],
                 mean_T=(float(got['locus_sum'].sum()) / hit if hit else None),
                 cells_per_s_kernel=got['work'] / (ms['kernel_ms'] * 1e-3), **ms)
            sg, t, ms = timed(lambda: dev.coal_segments(
                tab, bt, nodes, loci, pos, spp.t, brk, max_ago, 1, 0,
                [0, 1 << 28, 1 << 30, 1 << 32, TR.INT64_MAX], True, big))
            emit(what='segments', sample=name, max_ago=max_ago, call_s=round(t, 4),
                 launches=dev.lineage_info()['launches'],
                 segments=int(np.triu(sg['cnt'], 1).sum()),
                 longest_morgans=float(sg['longest'].max()) / TR.POS_PER_MORGAN,
                 cells_per_s_kernel=sg['work'] / (ms['kernel_ms'] * 1e-3), **ms)
        hn = nodes[np.sort(rng.choice(nodes.size, min(a.host_nodes, nodes.size), replace=False))]
        hl = np.sort(rng.choice(a.L, min(a.host_loci, a.L), replace=False))
        t0 = time.perf_counter()
        ref = CO.coal_times_np(tab, bt, tt, hn, hl, spp.t, a.max_ago, tedges)
        t = time.perf_counter() - t0
        got = dev.coal_times(tab, bt, hn, hl, spp.t, a.max_ago, tedges,
                             CO_OUT, max_work=big)
        same = all(np.array_equal(ref[k], got[k]) for k in CO_OUT + ('thist',))
        emit(what='host', sample=name, subsample_nodes=int(hn.size), subsample_loci=int(hl.size),
             cells=ref['work'], s=round(t, 3),
             scaled_to_full_request_s=round(t * CO.n_pairs(nodes.size) * a.L / ref['work'], 1),
             equals_device=bool(same))


CO_OUT = ('pair_sum', 'pair_cnt', 'locus_sum', 'locus_cnt', 'locus_max', 'mrca')

if __name__ == '__main__':
    main()
