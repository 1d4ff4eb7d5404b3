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

The model never simplifies its pedigree while it runs ('tskit_simp_interval': None): the
measurements above are of the table that holds every individual that ever lived.

    python tools/lineage_bench.py --simplify        # the same run, simplified once at its end

  trace      before: gnx_lineage_trace for the full request on the unsimplified table
  reach      gnx_pedigree_reach for the living (csrc/gnx_simplify.hip): kernel time, launches,
             the bytes the pass must move (every mask written once, the children's non-empty
             masks and their paths' words read once) and their rate beside gnx_measure_copy;
             then once more with the byte budget raised so that all words go in one block
  simplify   TreeTables.simplify on the host: seconds, rows and edges before / after
  trace      after: the same request on the simplified table, equal to the one before
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
    s['gen_arch'].update({'L': L, 'n_recomb_sims': 2000, 'use_tskit': True, 'r_distr_alpha': r,
                          'tskit_simp_interval': None})
    d['model'].update({'T': T, 'burn_T': 30, 'seed': {'num': seed}})
    return gnx.make_params_dict(d, 'lineage_bench')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=420, help='landscape side (K = 0.5 per cell)')
    ap.add_argument('--N', type=int, default=85000)
    ap.add_argument('--L', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--r', type=float, default=2e-3,
                    help='recombination rate between neighbouring loci (the default of 0.5 makes '
                         '~L / 2 edge rows per gamete: the HOST tables of 10^5 individuals over '
                         'hundreds of steps would not fit)')
    ap.add_argument('--simplify', action='store_true',
                    help='simplify the pedigree once at the end and measure that instead')
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
    if a.simplify:
        return simplify(a, spp, tt, ids, size)
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


def simplify(a, spp, tt, ids, size):
    """--simplify: the full trace, one simplification for the living, the full trace again"""
    from geonomics_amd import _native as nat
    dev = spp._dev
    loci = np.arange(a.L)
    want = ('first', 'last', 'n_kept')

    def trace(when):
        tab, bt = tt.node_table()
        rows = np.searchsorted(tt.ids, ids)
        nodes = np.stack([2 * rows, 2 * rows + 1], 1).ravel()
        t0 = time.perf_counter()
        tr = dev.lineage_trace(tab, bt, nodes, loci, spp.t, want=want, locus_range=False)
        t = time.perf_counter() - t0
        info = dev.lineage_info()
        emit(what='trace', when=when, rows=int(bt.size), call_s=round(t, 3),
             kernel_ms=round(info['kernel_ms'], 3), launches=info['launches'],
             table_uploaded=info['uploaded'])
        # node ids are renumbered by the simplification: compare the individuals behind them
        # (every 8th locus: the ids are int64)
        sub = {k: tr[k][::8] for k in want}
        return {k: np.where(v >= 0, tt.ids[np.maximum(v, 0) >> 1] * 2 + (v & 1), -1)
                if k != 'n_kept' else v.copy() for k, v in sub.items()}

    before = trace('before')
    tab, bt = tt.node_table()
    rows = np.searchsorted(tt.ids, ids)
    n_rows, n_edges = int(bt.size), tt._edges_count()
    t0 = time.perf_counter()
    node_loci = dev.pedigree_reach(tab, bt, rows)
    t = time.perf_counter() - t0
    info = dev.lineage_info()
    # every mask written once (16 W64 bytes per row); per child with a non-empty mask its mask
    # and the words of its path read once
    anc = node_loci > 0
    has_parent = tab[:, 0] >= 0
    moved = 8 * dev.W64 * (2 * n_rows + 2 * int((anc & has_parent).sum()))
    copy = nat.measure_copy(1 << 30, 3)
    rate = moved / (info['kernel_ms'] * 1e-3) / 1e9
    emit(what='reach', call_s=round(t, 3), kernel_ms=round(info['kernel_ms'], 3),
         launches=info['launches'], cohorts=int(np.unique(bt).size),
         nodes_ancestral=int(anc.sum()), nodes=int(anc.size),
         rows_with_an_ancestral_node=int((anc[0::2] | anc[1::2]).sum()),
         bytes_moved=int(moved), gb_per_s=round(rate, 1), measure_copy_gb_per_s=round(copy, 1),
         fraction_of_copy=round(rate / copy, 4))
    # the same pass with all words in one column block: a launch per cohort and no more
    dev.lineage_budget(2 * n_rows * dev.W64 * 8)
    same = np.array_equal(dev.pedigree_reach(tab, bt, rows), node_loci)
    info = dev.lineage_info()
    dev.lineage_budget(0)
    emit(what='reach_one_block', kernel_ms=round(info['kernel_ms'], 3), launches=info['launches'],
         mask_bytes=int(2 * n_rows * dev.W64 * 8), equals_default_budget=bool(same),
         fraction_of_copy=round(moved / (info['kernel_ms'] * 1e-3) / 1e9 / copy, 4))
    t0 = time.perf_counter()
    tt.simplify(rows, node_loci)
    t = time.perf_counter() - t0
    dev.lineage_forget()
    emit(what='simplify', host_s=round(t, 3), rows_before=n_rows, rows_after=int(tt.ids.size),
         edges_before=n_edges, edges_after=tt._edges_count(),
         kept_fraction=round(tt.ids.size / n_rows, 4), living=int(ids.size))
    after = trace('after')
    emit(what='equal', loci_compared=int(before['n_kept'].shape[0]), **{k: bool(np.array_equal(before[k], after[k])) for k in want})


if __name__ == '__main__':
    main()
