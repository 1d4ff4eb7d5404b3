"""Lineages through the recorded pedigree (csrc/gnx_lineage.hip, structs/pedigree.py): one
JSON line per measurement.

    python tools/lineage_bench.py                   # ~9 x 10^4 individuals, L = 1000, 200 steps

(recombination rate 0.002 between neighbouring loci, two Morgans: see --r)

A 'use_tskit': True model at the largest size Species._PEDIGREE_MAX_BITS admits (2 x 10^8
genotype bits: 10^5 individuals x 10^3 loci) is burned in and walked `--steps` main steps, the
pedigree recorded from the device's births.  Then, for both nodes of every living individual
and all loci:

  trace      gnx_lineage_trace for first / last / n_kept: the kernels' own time (HIP events
             around every launch, gnx_lineage_info) and the call's host clock (upload of the
             node table, launches, downloads)
  range      the per-locus min / max alone (what _check_coalescence asks for)
  stats      Species._calc_lineage_stats(as_arrays=True), end to end: the trace plus the fp64
             formulas on the host
  host       TreeTables.trace (the vectorised numpy walk) on a subsample of `--host-nodes`
             sample nodes x `--host-loci` loci, its time scaled by queries to the full request
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


def emit(**kw):
    print(json.dumps(kw), flush=True)


def params(side, N, L, T, r, seed):
    import geonomics_amd as gnx
    from geonomics_amd.sim import params as P
    d = P.default_params_dict(layers=[{'type': 'defined'}], species=[{'genomes': True}])
    d['landscape']['main']['dim'] = (side, side)
    d['landscape']['layers']['lyr_0']['init']['defined']['rast'] = np.ones((side, side))
    s = d['comm']['species']['spp_0']
    s['init'].update({'N': N, 'K_factor': 0.5})
    s['mating'].update({'mating_radius': 4})
    s['gen_arch'].update({'L': L, 'n_recomb_sims': 2000, 'use_tskit': True, 'r_distr_alpha': r})
    d['model'].update({'T': T, 'burn_T': 30, 'seed': {'num': seed}})
    return gnx.make_params_dict(d, 'lineage_bench')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=460, help='landscape side (K = 0.5 per cell)')
    ap.add_argument('--N', type=int, default=90000)
    ap.add_argument('--L', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--r', type=float, default=2e-3,
                    help='recombination rate between neighbouring loci (the default of 0.5 makes '
                         '~L / 2 edge rows per gamete: the HOST tables of 10^5 individuals over '
                         'hundreds of steps would not fit)')
    ap.add_argument('--host-nodes', type=int, default=2000)
    ap.add_argument('--host-loci', type=int, default=50)
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    import geonomics_amd as gnx
    warnings.simplefilter('ignore')
    mod = gnx.make_model(params(a.side, a.N, a.L, a.steps, a.r, 19))
    spp = mod.comm[0]
    t0 = time.perf_counter()
    mod.walk(10000, 'burn', verbose=False)
    t1 = time.perf_counter()
    if spp._tt is None:
        raise SystemExit('%d individuals x %d loci at genome assignment: past '
                         '_PEDIGREE_MAX_BITS, no pedigree; lower --side' % (len(spp), a.L))
    mod.walk(a.steps, 'main', verbose=False)
    t2 = time.perf_counter()
    tt = spp._tt
    tab, bt = tt.node_table()
    ids = np.array([*spp])
    rows = np.searchsorted(tt.ids, ids)
    nodes = np.stack([2 * rows, 2 * rows + 1], 1).ravel()
    loci = np.arange(a.L)
    size = dict(living=int(ids.size), sample_nodes=int(nodes.size), loci=a.L,
                pedigree_rows=int(bt.size), main_steps=a.steps,
                genotype_bits_at_assignment=int(tt.n_founders * a.L * 2),
                queries=int(nodes.size) * a.L)
    emit(what='model', burn_s=round(t1 - t0, 2), main_s=round(t2 - t1, 2),
         node_table_bytes=int(tab.nbytes + bt.nbytes), **size)
    dev = spp._dev
    for rep in range(2):        # the first call uploads the node table, the second finds it
        t0 = time.perf_counter()
        tr = dev.lineage_trace(tab, bt, nodes, loci, spp.t, want=('first', 'last', 'n_kept'),
                               locus_range=False)
        t = time.perf_counter() - t0
        info = dev.lineage_info()
        hops = int(tr['n_kept'].sum(dtype=np.int64))
        emit(what='trace', rep=rep, call_s=round(t, 3), kernel_ms=round(info['kernel_ms'], 3),
             launches=info['launches'], table_uploaded=info['uploaded'],
             kept_nodes=hops, mean_kept=round(hops / tr['n_kept'].size, 2),
             queries_per_s_kernel=size['queries'] / (info['kernel_ms'] * 1e-3),
             bytes_to_host=int(3 * tr['n_kept'].nbytes))
    del tr
    t0 = time.perf_counter()
    rg = dev.lineage_trace(tab, bt, nodes, loci, spp.t, want=())
    t = time.perf_counter() - t0
    info = dev.lineage_info()
    emit(what='range', call_s=round(t, 3), kernel_ms=round(info['kernel_ms'], 3),
         launches=info['launches'], bytes_to_host=int(2 * rg['locus_lo'].nbytes),
         loci_coalesced=int(((rg['locus_lo'] == rg['locus_hi']) & (rg['locus_lo'] >= 0)).sum()))
    t0 = time.perf_counter()
    st = spp._calc_lineage_stats(as_arrays=True)
    t = time.perf_counter() - t0
    emit(what='stats', end_to_end_s=round(t, 2), kernel_ms=round(dev.lineage_info()['kernel_ms'], 3),
         share_with_two_or_more=float(np.mean(~np.isnan(st['time']))),
         mean_time=float(np.nanmean(st['time'])), mean_dist=float(np.nanmean(st['dist'])))
    del st
    rng = np.random.RandomState(0)
    hn = nodes[np.sort(rng.choice(nodes.size, min(a.host_nodes, nodes.size), replace=False))]
    hl = np.sort(rng.choice(a.L, min(a.host_loci, a.L), replace=False))
    t0 = time.perf_counter()
    host = tt.trace(hn, hl, spp.t)
    t = time.perf_counter() - t0
    got = dev.lineage_trace(tab, bt, hn, hl, spp.t, locus_range=False)
    same = all(np.array_equal(host[k], got[k]) for k in ('root', 'first', 'last', 'n_kept'))
    q = hn.size * hl.size
    emit(what='host', subsample_nodes=int(hn.size), subsample_loci=int(hl.size), queries=q,
         s=round(t, 3), scaled_to_full_request_s=round(t * size['queries'] / q, 1),
         equals_device=bool(same))


if __name__ == '__main__':
    main()
