"""The mixed-model association scan on the device (csrc/gnx_quad.hip, sim/assoc.py lmm_*): one
JSON line per measurement.

    python tools/lmm_bench.py --part metric   # c4_metric: n = 8192, L = 10^5
    python tools/lmm_bench.py --part c2       # C2: n = 8192, L = 10^4, and the host route

Both parts: bench.py's population walked 20 steps, a random sample of --n individuals (default
8192) and a response (the x coordinate plus noise, standardised: spatial structure is what the
mixed model is there for).  The real Species methods run around the bare handle: _calc_grm, then
_run_lmm with that matrix - its `seconds` (eigh, reml, cross, quad) are the whole call's split -
and then gnx_assoc_quad alone on the call's own rotation and table: kernel_ms by HIP events
around its kernels, best and all repeats after a warm-up, the whole call by the host clock (it
adds the finite checks, the transposition of M and its 256 MiB upload), and 2 n^2 L_used FLOP
over the kernel time against the 157 TF f32 matrix peak and gnx_grm's 78 TF.
c2 adds the parent commit's only route to the same numbers: gnx_download_genomes of the sample,
unpacking, the centred Z in fp64 and M Z in numpy on the host's threads, squared and summed.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from geonomics_amd import _native as nat  # noqa: E402
from geonomics_amd.sim import assoc as A  # noqa: E402
from geonomics_amd.structs.analyses import SpeciesAnalyses  # noqa: E402
from geonomics_amd.structs.species import Species  # noqa: E402

F32_MATRIX_PEAK = 157.3e12   # MI355X: f32 MFMA = the f32 vector rate
GRM_RATE = 78.5e12           # gnx_grm on its computed tiles (profiles/grm_bench.txt)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


class _StandIn(SpeciesAnalyses):
    _field = Species._field


def stand_in_species(dev):
    """the real Species methods of the analysis around a bare handle"""
    spp = _StandIn()
    spp._dev, spp.gen_arch = dev, types.SimpleNamespace(traits={})
    spp._genomes_assigned = True
    return spp


def mask_words(dev, loci):
    m = np.zeros(dev.W64, np.uint64)
    np.bitwise_or.at(m, loci >> 6, np.uint64(1) << (loci & 63).astype(np.uint64))
    return m


def host_route(dev, L, slots, M, centre, use):
    """the parent commit's only route -> (seconds: download, unpack, M Z and squares; q)"""
    t0 = time.perf_counter()
    packed = dev.download_genomes(slots)
    t1 = time.perf_counter()
    by = np.ascontiguousarray(packed).view(np.uint8).reshape(packed.shape[0], 2, -1)
    bits = np.unpackbits(by, axis=2, bitorder='little')[:, :, :L]
    Z = (bits[:, 0] + bits[:, 1]).astype(np.float64)
    del bits, by
    t2 = time.perf_counter()
    Z -= centre[None, :]
    Z[:, ~use] = 0.0
    q = np.zeros(L)
    for a in range(0, L, 2048):                  # M Z in column blocks: 128 MiB at a time
        Cm = M @ Z[:, a:a + 2048]
        q[a:a + 2048] = (Cm * Cm).sum(axis=0)
    t3 = time.perf_counter()
    return (t1 - t0, t2 - t1, t3 - t2, t3 - t0), q


def run(name, n, reps, with_host):
    cfg = bench.WORKLOADS[name]
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(20, False, True)
    L = cfg['L']
    spp = stand_in_species(dev)
    dev.geno_gram(np.arange(2, dtype=np.int64))      # gathers the walked population into [0, N)
    rng = np.random.RandomState(0)
    all_ids = np.sort(dev.download(nat.F_ID))
    ids = np.sort(rng.choice(all_ids, n, replace=False))
    _, slots = spp._geno_sample(ids)
    x = dev.download(nat.F_X)[slots].astype(np.float64)
    y = (x - x.mean()) / x.std() + rng.standard_normal(n)
    t_grm, grm = clock(lambda: spp._calc_grm(individs=ids))
    t_all, res = clock(lambda: spp._run_lmm(y=y, individs=ids, grm=grm))
    sec = dict(res['seconds'], grm=t_grm)
    emit(workload=name, what='run_lmm', n=n, L=L, n_loci_grm=res['n_loci_grm'],
         tested=int(res['tested'].sum()), delta=res['delta'], h2=res['h2'], gif=float(res['gif'][0]),
         seconds={k: round(v, 4) for k, v in sec.items()}, call_s=round(t_all + t_grm, 3),
         eigh_share=sec['eigh'] / (t_all + t_grm), kernel_ms=res['kernel_ms'])
    t_ols, ols = clock(lambda: spp._run_gwas(y=y, individs=ids))
    emit(workload=name, what='run_gwas', call_s=round(t_ols, 4), gif=float(ols['gif'][0]))
    # gnx_assoc_quad alone, on the call's own rotation and table
    M = A.lmm_rotation(grm['eig'][0], grm['eig'][1], res['delta']).astype(np.float32)
    got = dev.assoc_cross(np.ones(n), slots)
    use, _ = A.lmm_testable(got['s1'], got['s2'], n)
    val = A.lmm_table(got['s1'], n, use)
    mask = mask_words(dev, np.flatnonzero(use))
    first = dev.assoc_quad(val, M, slots, mask)                       # the warm-up
    ms, wall = [], []
    for _ in range(reps):
        t, again = clock(lambda: dev.assoc_quad(val, M, slots, mask))
        wall.append(t)
        ms.append(again['kernel_ms'])
    assert again['q'].tobytes() == first['q'].tobytes()
    flop = 2.0 * n * n * int(use.sum())
    rate = flop / (min(ms) * 1e-3)
    emit(workload=name, what='gnx_assoc_quad', n=n, m=n, L=L, n_loci=int(use.sum()),
         kernel_ms=[round(v, 3) for v in ms], kernel_ms_best=min(ms),
         call_s=[round(v, 3) for v in wall], tflops=rate / 1e12,
         share_f32_matrix_peak=rate / F32_MATRIX_PEAK, share_of_gnx_grm_rate=rate / GRM_RATE)
    if with_host:
        M64 = M.astype(np.float64)
        centre = A.lmm_centre(got['s1'], n)
        h_t = []
        for r in range(reps):
            t, qh = host_route(dev, L, slots, M64, centre, use)
            h_t.append(t[3])
            rel = float((np.abs(again['q'] - qh)[use] / qh[use]).max())
            emit(workload=name, what='host_route', r=r, download_s=round(t[0], 3),
                 unpack_s=round(t[1], 3), product_s=round(t[2], 3), total_s=round(t[3], 3),
                 max_rel_diff=rel)
        emit(workload=name, what='device_vs_host', device_call_s_median=float(np.median(wall)),
             host_s_median=float(np.median(h_t)),
             ratio_host_over_device=float(np.median(h_t) / np.median(wall)))
    dev.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['metric', 'c2'], required=True)
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    import torch
    torch.cuda.init()           # torch's HIP runtime first, the library's handles behind it (bench.py)
    run('c4_metric' if a.part == 'metric' else 'c2', a.n, a.reps, a.part == 'c2')
