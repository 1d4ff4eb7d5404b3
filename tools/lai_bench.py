"""gnx_lai_paint on the device (csrc/gnx_lai.hip): one JSON line per measurement.

    python tools/lai_bench.py                  # n = 8192, L = 10^5, K = 2
    python tools/lai_bench.py --case tiny      # n = 300, L = 2000, K = 2

Random genomes (the time does not depend on the bits), Balding-Nichols frequencies, Dirichlet
priors, a uniform map of 10 Morgans, 10 generations.  Measured: the forward pass alone
(want_post = 0, what gens='fit' evaluates) and the whole painting under several byte budgets;
`kernel_ms` is the HIP-event time of the call's kernels, `call_ms` the host clock around the
synchronous call (uploads, scratch allocation and read-backs included), `scratch_bytes` the
posteriors of one batch.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geonomics_amd import _native as nat  # noqa: E402
from geonomics_amd.sim import lai as LAI  # noqa: E402

LINES = []
CASES = dict(flagship=dict(n=8192, L=100000, K=2), tiny=dict(n=300, L=2000, K=2))
DEFAULT_BUDGET = 4 << 30


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3),
                max=round(max(v), 3))


def run_case(name, n, L, K, reps, budgets):
    side = int(np.ceil(np.sqrt(n / 4.0))) + 1
    dev = nat.Device(side, side, 1, L=L, cap_inds=n + 64, cap_rows=n + 64, seed=3)
    dev.upload_rasters(np.ones((1, side, side), np.float32))
    dev.set_species_params(nat.default_species_params())
    rng = np.random.default_rng(2)
    dev.upload_population(rng.uniform(0, side, n).astype(np.float32),
                          rng.uniform(0, side, n).astype(np.float32), np.zeros(n), np.zeros(n),
                          np.arange(n))
    dev.upload_genomes(rng.integers(0, 2 ** 63, size=(n, 2, dev.W64), dtype=np.int64)
                       .view(np.uint64))
    p = rng.uniform(0.1, 0.9, L)
    F = LAI.clip_freqs(rng.beta(p * 4.0, (1.0 - p) * 4.0, size=(K, L)).T)
    Q = rng.dirichlet(np.ones(K), size=n)
    sw, stay = LAI.switch_probs(np.linspace(0.0, 10.0, L), 10.0)
    emit(case=name, what='setup', n=n, L=L, K=K, haplotypes=2 * n,
         posterior_bytes_all=2 * n * L * K * 8)
    runs = [('forward', dict(want_post=False), None)] + \
        [('paint', dict(budget=b), b) for b in budgets]
    for what, kw, b in runs:
        got = dev.lai_paint(F, sw, stay, Q, **kw)                # warm-up
        k_ms, c_ms = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = dev.lai_paint(F, sw, stay, Q, **kw)
            c_ms.append((time.perf_counter() - t0) * 1e3)
            k_ms.append(got['kernel_ms'])
        line = dict(case=name, what=what, kernel_ms=stats(k_ms), call_ms=stats(c_ms),
                    batches=got['batches'],
                    haplotype_loci_per_s=2.0 * n * L / (statistics.median(k_ms) * 1e-3))
        if b is not None:
            per = L * K * 8
            nb = min((2 * n + 63) // 64 * 64, (b or DEFAULT_BUDGET) // per // 64 * 64)
            line.update(budget=b or DEFAULT_BUDGET, batch_haplotypes=nb, scratch_bytes=nb * per)
        emit(**line)
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='flagship', choices=sorted(CASES))
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--budgets', default='0,1,16',
                    help='GiB of scratch per batch, comma-separated (0: the default)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lai_bench.txt'))
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    c = CASES[a.case]
    run_case(a.case, c['n'], c['L'], c['K'], a.reps,
             [int(float(g) * (1 << 30)) for g in a.budgets.split(',')])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('# python tools/lai_bench.py on one MI355X: gnx_lai_paint, the forward pass alone '
                'and the whole painting under\n# several byte budgets (HIP-event kernel time and '
                'host clock); %d repetitions after a warm-up\n' % a.reps)
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
