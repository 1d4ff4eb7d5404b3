"""Model.run_gea on the device (csrc/gnx_gea.hip, sim/gea.py): one JSON line per measurement.

    python tools/gea_bench.py                       # C2, 1024 / 4096 / 8192 loci
    tools/kstat_cmd.sh r10_gea tools/gea_bench.py   # the same under rocprofv3: kernel times

bench.py's C2 population (10^5 individuals, L = 10^4) walked 20 steps (blocks shared with
parents).  For n_loci evenly spaced loci: gnx_geno_locus_gram and gnx_geno_locus_cross (the
calls are synchronous and end with their downloads: host clock around them), the whole
Species._run_cca (the real method, on a stand-in Species around the handle: cross-products,
the host recurrence, the scores' gnx_geno_matmul), and the parent commit's only route:
download_genomes of every slot (what Model.get_genotypes does), unpacking the same loci, then
sklearn's CCA where it imports, otherwise the host recurrence with numpy products.  Bytes that
cross to the host are counted from the shapes of what each route downloads.  The host clock
includes the n_loci^2 int64 download of C; the kernels' own times come from the rocprofv3
run, and the AND + popcount rate in the `gram` line uses the call's time as a lower bound.
"""
import argparse
import json
import os
import sys
import time
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from geonomics_amd.sim import gea as G  # noqa: E402
from geonomics_amd.structs.analyses import SpeciesAnalyses  # noqa: E402
from geonomics_amd.structs.species import Species  # noqa: E402

# 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz 32-bit VALU operations per second; one AND + popcount
# of a 64-bit word is 2 v_and_b32 + 2 v_bcnt_u32_b32
INT32_RATE = 256 * 4 * 16 * 2.4e9
OPS_PER_WORD = 4


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


class _StandIn(SpeciesAnalyses):
    _field = Species._field


def stand_in_species(dev, lyr_num):
    """the real Species methods of the analysis around a bare handle"""
    trt = types.SimpleNamespace(lyr_num=lyr_num, loci=np.zeros(0, np.int64))
    spp = _StandIn()
    spp._dev, spp.gen_arch = dev, types.SimpleNamespace(traits={0: trt})
    spp._genomes_assigned = True
    return spp


def host_route(dev, loci, lyr_num):
    """the parent commit's only route -> (seconds: download, unpack, fit), results, how"""
    from geonomics_amd import _native as nat
    t0 = time.perf_counter()
    order = np.argsort(dev.download(nat.F_ID), kind='stable')       # rows in ascending-id order
    packed = dev.download_genomes(order)
    Z = np.column_stack([dev.download(nat.F_E)[lyr_num], dev.download(nat.F_X),
                         dev.download(nat.F_Y)]).astype(np.float64)[order]
    t1 = time.perf_counter()
    by = np.ascontiguousarray(packed).view(np.uint8).reshape(packed.shape[0], 2, -1)
    bits = np.unpackbits(by, axis=2, bitorder='little')[:, :, loci]
    D = (bits[:, 0] + bits[:, 1]).astype(np.int64)
    del bits, by
    t2 = time.perf_counter()
    try:
        from sklearn.cross_decomposition import CCA
        X = D / 2.0
        cca = CCA(n_components=3).fit(X, Z)
        res = dict(ind_df=cca.transform(X), loci_df=cca.x_loadings_, var_df=cca.y_loadings_)
        how = 'sklearn CCA'
    except ImportError:
        Df = D.astype(np.float64)
        res = G.cca_from_cross_products(*G.numpy_cross_products(D, Z), D.shape[0],
                                        lambda M: Df @ M)
        how = 'host recurrence, numpy products'
    t3 = time.perf_counter()
    return (t1 - t0, t2 - t1, t3 - t2), res, how, packed.nbytes + Z.shape[0] * 3 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c2', choices=sorted(bench.WORKLOADS))
    ap.add_argument('--loci', type=int, nargs='+', default=[1024, 4096, 8192])
    ap.add_argument('--host-route-up-to', type=int, default=1024,
                    help='largest n_loci the host route is run at (its fit is O(N n_loci^2) '
                         'per pseudo-inverse on one core)')
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    cfg = bench.WORKLOADS[a.workload]
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(20, False, True)
    N, L = dev.N, cfg['L']
    spp = stand_in_species(dev, 1)
    warnings.simplefilter('ignore', G.GEAConvergenceWarning)
    for n_loci in a.loci:
        loci = np.unique(np.linspace(0, L - 1, n_loci).astype(np.int64))
        n_loci = loci.size
        words = (N + 63) // 64
        t = timed(lambda: dev.geno_locus_gram(loci), 3)
        pairs = n_loci * (n_loci + 1) / 2.0                 # what is needed ...
        tiles = (n_loci + 63) // 64
        done = tiles * (tiles + 1) / 2.0 * 64 * 64          # ... and what the tile kernel does
        best = min(t)
        emit(workload=a.workload, what='gram', N=N, n_loci=n_loci,
             ms=[round(x * 1e3, 2) for x in t], bytes_to_host=n_loci * n_loci * 8 + n_loci * 8,
             and_popcounts=done * 4 * words, and_popcounts_needed=pairs * 4 * words,
             and_popcounts_per_s_at_least=done * 4 * words / best,
             int32_issue_rate=INT32_RATE,
             share_of_issue_rate_at_least=done * 4 * words * OPS_PER_WORD / best / INT32_RATE)
        t = timed(lambda: dev.geno_locus_cross(loci, 1), 3)
        emit(workload=a.workload, what='cross', N=N, n_loci=n_loci,
             ms=[round(x * 1e3, 2) for x in t], bytes_to_host=(n_loci * 3 + 12 + 256 * 9) * 8)
        t0 = time.perf_counter()          # once: three eigh of n_loci x n_loci on the host
        res = spp._run_cca(loci=loci)
        t = [time.perf_counter() - t0]
        to_host = n_loci * n_loci * 8 + n_loci * 8 + (n_loci * 3 + 12 + 256 * 9) * 8 \
            + N * 8 + N * 3 * 4                              # C, s, D^T Z ..., ids, scores
        emit(workload=a.workload, what='run_gea_device', N=N, n_loci=n_loci,
             s=[round(x, 3) for x in t], bytes_to_host=to_host,
             n_by_l_bytes_fp64=N * n_loci * 8)
        if n_loci <= a.host_route_up_to:
            (td, tu, tf), ref, how, nbytes = host_route(dev, loci, 1)
            err = {k: float(np.abs(res[k] - ref[k]).max() / np.abs(ref[k]).max())
                   for k in ('ind_df', 'loci_df', 'var_df')}
            emit(workload=a.workload, what='run_gea_host_route', how=how, N=N, n_loci=n_loci,
                 download_s=round(td, 3), unpack_s=round(tu, 3), fit_s=round(tf, 3),
                 total_s=round(td + tu + tf, 3), bytes_to_host=nbytes,
                 device_vs_host_rel_err=err)
    dev.close()


if __name__ == '__main__':
    main()
