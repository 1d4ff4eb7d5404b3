"""The logistic sweep on the device (csrc/gnx_glm.hip, sim/glm.py): one JSON line per measurement.

    python tools/glm_bench.py --part sweep    # gnx_glm_sweep alone at four sizes
    python tools/glm_bench.py --part gea      # a whole run_logistic_gea: n = 8192, L = 10^5

sweep: X = [1 | standard normal columns], B standard normal / 2 (|eta| of order 1, the regime of
a Newton iteration), kernel_ms by HIP events around the call's kernels, best and all repeats
after a warm-up, the whole call by the host clock (it adds the finite checks, the uploads and
the download of the sums).  Beside it elements/s = n m / kernel time, and the share of the fp64
vector peak that implies: elements/s x the fp64 VALU instructions per element of the inner loop
(FP64_PER_ELEMENT, counted in the disassembly of the gfx950 code object: the loop body of
k_glm_sweep<P> holds two rows) over the rate at which the device issues them, 256 CUs x 4 SIMDs
x 16 lanes x 2.4 GHz = 39.3e12 per second (an FMA counts two FLOP: the 78.6 TF of the data
sheet).
gea: bench.py's population walked 20 steps, a random sample of --n individuals, the tested
variable their x coordinate plus noise; the real Species method runs around the bare handle.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import bench  # noqa: E402
from geonomics_amd import _native as nat  # noqa: E402

FP64_ISSUE_RATE = 256 * 4 * 16 * 2.4e9
# fp64 VALU instructions per element (row x fit) in the inner loop, per p; of them 130 are the
# exp, the log1p (77 v_add_f64: ocml's extended-precision logarithm) and the division
FP64_PER_ELEMENT = {1: 152.0, 2: 157.0, 3: 163.0, 4: 170.0, 5: 178.0, 6: 187.0, 7: 197.0,
                    8: 208.0}
ALL_PER_ELEMENT = {1: 171.5, 2: 173.0, 3: 182.5, 4: 188.5, 5: 200.5, 6: 210.5, 7: 218.0,
                   8: 229.5}
SWEEP_SIZES = [(8192, 100000, 2), (8192, 100000, 4), (8192, 100000, 8), (1000000, 100000, 2)]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def sweep(reps):
    dev = nat.Device(8, 8, 1, L=64, cap_inds=64, cap_rows=64, seed=1)
    for n, m, p in SWEEP_SIZES:
        rng = np.random.RandomState(n % 1000 + p)
        X = np.column_stack([np.ones(n), rng.standard_normal((n, p - 1))])
        B = rng.standard_normal((m, p)) / 2.0
        first = dev.glm_sweep(X, B, info=True)                        # the warm-up
        ms, wall = [], []
        for _ in range(reps):
            t, (again, k_ms) = clock(lambda: dev.glm_sweep(X, B))
            wall.append(t)
            ms.append(k_ms)
        assert again.tobytes() == first['sums'].tobytes()
        rate = n * m / (min(ms) * 1e-3)
        emit(what='gnx_glm_sweep', n=n, m=m, p=p, stretch=first['stretch'],
             stretches=first['stretches'], kernel_ms=[round(v, 3) for v in ms],
             kernel_ms_best=min(ms), call_s=[round(v, 3) for v in wall],
             elements_per_s=rate, fp64_instr_per_element=FP64_PER_ELEMENT[p],
             instr_per_element=ALL_PER_ELEMENT[p],
             share_fp64_vector_peak=rate * FP64_PER_ELEMENT[p] / FP64_ISSUE_RATE)
    dev.close()


def gea(n, reps):
    from lmm_bench import stand_in_species
    cfg = bench.WORKLOADS['c4_metric']
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(20, False, True)
    spp = stand_in_species(dev)
    dev.geno_gram(np.arange(2, dtype=np.int64))      # gathers the walked population into [0, N)
    rng = np.random.RandomState(0)
    ids = np.sort(rng.choice(np.sort(dev.download(nat.F_ID)), n, replace=False))
    _, slots = spp._geno_sample(ids)
    x = dev.download(nat.F_X)[slots].astype(np.float64)
    env = (x - x.mean()) / x.std() + rng.standard_normal(n)
    for r in range(reps + 1):                        # the first one is the warm-up
        t, res = clock(lambda: spp._run_logistic_gea(env=env, individs=ids))
        emit(what='run_logistic_gea', r=r, n=n, L=cfg['L'], tested=int(res['tested'].sum()),
             converged=int(res['converged'].sum()), n_iter_max=int(res['n_iter'].max()),
             n_sweeps=res['n_sweeps'], gif=res['gif'], kernel_ms=res['kernel_ms'],
             call_s=round(t, 3))
    t, lin = clock(lambda: spp._run_lfmm(0, env=env, individs=ids, calibrate=False))
    emit(what='run_lfmm K=0 (the linear scan of the same request)', call_s=round(t, 3),
         gif=float(lin['gif'][0]), kernel_ms=lin['kernel_ms'])
    dev.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['sweep', 'gea'], required=True)
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    import torch
    torch.cuda.init()           # torch's HIP runtime first, the library's handles behind it (bench.py)
    if a.part == 'sweep':
        sweep(a.reps)
    else:
        gea(a.n, a.reps)
