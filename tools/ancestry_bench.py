"""One EM sweep of the admixture model on the device (csrc/gnx_admix.hip) beside the same sweep
written in torch fp64 on the same GPU: one JSON line per measurement, printed and written to
--out.

    python tools/ancestry_bench.py                   # both cases
    python tools/ancestry_bench.py --case fit        # n = 2 000, L = 10^5, K = 5
    python tools/ancestry_bench.py --case project    # n = 10^5, L = 10^4, K = 5, F held

A planted sample (Balding-Nichols frequencies, Fst 0.2; two thirds of the individuals unadmixed)
is drawn on the host straight into packed genomes and uploaded.  `kernel_ms` is the HIP-event
time of the call's kernels (gnx_admix_info), `call_ms` the host clock around the synchronous
call; `reps` repetitions after a warm-up, median and range.
The baseline is what a user has without the kernel: the dosage matrix unpacked on the GPU to an
n x L fp64 tensor (timed apart: `unpack_ms`) and the sweep in torch - two products for p and r,
two quotients, four products for A and B - timed with torch's events.
flop: 8 K per genotype and pass (K FMAs each for p, r and the two accumulations; the pass for B
recomputes p and r), divisions and logarithms not counted; the share of the vector-fp64 peak is
of 78.6 TFLOP/s.
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
from geonomics_amd.sim import ancestry as AN  # noqa: E402

PEAK_FP64 = 78.6e12
LINES = []
CASES = dict(fit=dict(n=2000, L=100000, K=5, hold=False),
             project=dict(n=100000, L=10000, K=5, hold=True),
             tiny=dict(n=300, L=2000, K=5, hold=False))


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def planted_packed(n, L, K, W64, seed=1, block=512):
    """(packed genomes uint64 [n][2][W64], Q, F) of a planted sample, drawn block by block"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, L)
    c = (1.0 - 0.2) / 0.2
    F = np.clip(rng.beta(p * c, (1.0 - p) * c, size=(K, L)), AN.EPS, 1.0 - AN.EPS)
    Q = np.zeros((n, K))
    pure = (2 * n) // 3
    Q[np.arange(pure), np.arange(pure) % K] = 1.0
    Q[pure:] = rng.dirichlet(np.ones(K), size=n - pure)
    out = np.zeros((n, 2, W64), np.uint64)
    F32 = F.astype(np.float32)
    for i0 in range(0, n, block):
        P = Q[i0:i0 + block].astype(np.float32) @ F32
        m = P.shape[0]
        bits = np.zeros((m, 2, W64 * 64), np.uint8)
        for h in range(2):
            bits[:, h, :L] = rng.random((m, L), dtype=np.float32) < P
        out[i0:i0 + m] = np.packbits(bits, axis=2, bitorder='little').view('<u8').reshape(
            m, 2, W64)
    return out, Q, F


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3),
                max=round(max(v), 3))


def unpack_dosages(torch, packed_t, L, block=4096):
    """D fp64 [n][L] on the device from the packed genomes int64 [n][2][W64] on the device"""
    n = packed_t.shape[0]
    sh = torch.arange(64, device=packed_t.device, dtype=torch.int64)
    D = torch.empty((n, L), dtype=torch.float64, device=packed_t.device)
    for i0 in range(0, n, block):
        w = packed_t[i0:i0 + block]
        b = ((w.unsqueeze(-1) >> sh) & 1).reshape(w.shape[0], 2, -1)[:, :, :L]
        D[i0:i0 + block] = (b[:, 0] + b[:, 1]).to(torch.float64)
    return D


def torch_sweep(torch, D, Q, F, want_B, want_ll):
    G = 1.0 - F
    p, r = Q @ F, Q @ G
    u, v = D / p, (2.0 - D) / r
    A = u @ F.T + v @ G.T
    B1 = B0 = ll = None
    if want_B:
        B1, B0 = Q.T @ u, Q.T @ v
    if want_ll:
        ll = (D * torch.log(p) + (2.0 - D) * torch.log(r)).sum()
    return A, B1, B0, ll


def run_case(torch, name, n, L, K, hold, reps):
    tdev = torch.device('cuda', 0)
    side = int(np.ceil(np.sqrt(n / 4.0))) + 1
    dev = nat.Device(side, side, 1, L=L, cap_inds=n + 64, cap_rows=n + 64, seed=3)
    dev.upload_rasters(np.ones((1, side, side), np.float32))
    dev.set_species_params(nat.default_species_params())
    rng = np.random.RandomState(2)
    dev.upload_population(rng.uniform(0, side, n).astype(np.float32),
                          rng.uniform(0, side, n).astype(np.float32), np.zeros(n), np.zeros(n),
                          np.arange(n))
    t0 = time.perf_counter()
    packed, Qt, Ft = planted_packed(n, L, K, dev.W64)
    dev.upload_genomes(packed)
    emit(case=name, what='setup', n=n, L=L, K=K, hold=hold,
         host_s=round(time.perf_counter() - t0, 1))
    Q0, F0 = AN.init_random(n, L, K, seed=5)
    Q, F = torch.as_tensor(Q0, device=tdev), torch.as_tensor(F0, device=tdev)
    cells = float(n) * L
    out = {}
    for want_ll in (False, True):
        fn = lambda: dev.admix_sweep(Q, F, None, None, want_ll, None, not hold)
        out[want_ll] = fn()                                      # warm-up
        k_ms, c_ms = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            c_ms.append((time.perf_counter() - t0) * 1e3)
            k_ms.append(dev.admix_info()['kernel_ms'])
        flop = 8.0 * K * cells * (1 if hold else 2)
        rate = flop / (statistics.median(k_ms) * 1e-3)
        emit(case=name, what='kernel', loglik=want_ll, kernel_ms=stats(k_ms), call_ms=stats(c_ms),
             info=dev.admix_info(), flop=flop, tflops=round(rate / 1e12, 2),
             share_of_fp64_vector_peak=round(rate / PEAK_FP64, 3),
             genotypes_per_s=cells / (statistics.median(k_ms) * 1e-3))
    # ---- the torch baseline on the unpacked dosages
    packed_t = torch.as_tensor(packed.view(np.int64), device=tdev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    unpack_dosages(torch, packed_t[:64], L)
    torch.cuda.synchronize()
    ev[0].record()
    D = unpack_dosages(torch, packed_t, L)
    ev[1].record()
    torch.cuda.synchronize()
    unpack_ms = ev[0].elapsed_time(ev[1])
    del packed_t
    base = {}
    for want_ll in (False, True):
        ref = torch_sweep(torch, D, Q, F, not hold, want_ll)     # warm-up
        torch.cuda.synchronize()
        t_ms = []
        for _ in range(reps):
            ev[0].record()
            torch_sweep(torch, D, Q, F, not hold, want_ll)
            ev[1].record()
            torch.cuda.synchronize()
            t_ms.append(ev[0].elapsed_time(ev[1]))
        base[want_ll] = statistics.median(t_ms)
        got = out[want_ll]
        diff = dict(A=float(((got['A'] - ref[0]).abs() / ref[0]).max()))
        if not hold:
            diff['B1'] = float(((got['B1'] - ref[1]).abs() / ref[1].clamp_min(1e-300)).max())
            diff['B0'] = float(((got['B0'] - ref[2]).abs() / ref[2].clamp_min(1e-300)).max())
        if want_ll:
            diff['loglik'] = abs(got['loglik'] - float(ref[3])) / abs(float(ref[3]))
        emit(case=name, what='torch', loglik=want_ll, sweep_ms=stats(t_ms),
             unpack_ms=round(unpack_ms, 3), dosage_bytes=int(cells * 8), max_rel_diff=diff)
        del ref
    del D
    torch.cuda.empty_cache()
    dev.close()
    return out, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='both', choices=['both'] + sorted(CASES))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ancestry_bench.txt'))
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    names = ['fit', 'project'] if a.case == 'both' else [a.case]
    for name in names:
        c = CASES[name]
        run_case(torch, name, c['n'], c['L'], c['K'], c['hold'], a.reps)
    k = {(json.loads(l)['case'], json.loads(l)['loglik']): json.loads(l) for l in LINES
         if json.loads(l)['what'] == 'kernel'}
    for l in [json.loads(x) for x in LINES if json.loads(x)['what'] == 'torch']:
        mine = k[(l['case'], l['loglik'])]['kernel_ms']['median']
        emit(case=l['case'], what='ratio', loglik=l['loglik'], kernel_ms=mine,
             torch_ms=l['sweep_ms']['median'],
             torch_over_kernel=round(l['sweep_ms']['median'] / mine, 2))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('# python tools/ancestry_bench.py on one MI355X: one sweep of gnx_admix_sweep '
                '(HIP-event kernel time and host\n# clock) beside the same sweep in torch fp64 on '
                'the unpacked dosages; %d repetitions after a warm-up\n' % a.reps)
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
