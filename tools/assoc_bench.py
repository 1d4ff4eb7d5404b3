"""gnx_assoc_cross on the device (csrc/gnx_assoc.hip): one JSON line per measurement, to stdout
and to profiles/assoc_bench.txt (--out).

    python tools/assoc_bench.py                       # c4_metric: 10^6 individuals, L = 10^5
    python tools/assoc_bench.py --workload c2 --reps 2

bench.py's population walked a few steps (blocks shared with parents).  For a sample of --n
individuals and for everybody, and for m = 8, 16, 24 and 32 columns of a random Y:
  kernel_ms    the HIP-event time of the call's two kernels (the cross-products, the sum over the
               stretches), median, min and max of --reps calls after a warm-up
  call_ms      the host clock around the synchronous call (upload of Y, scratch, read-backs)
  fma          the fp64 fused multiply-adds the kernel issues per lane: n L times m rounded up
               to the column block (8 or 16), and their rate as 2 fma / kernel time against the
               part's fp64 vector peak (78.6 TFLOP/s, data sheet)
  genome_bytes the packed genomes read, once per column block (2 n W64 8 bytes each), and their
               rate against the HBM peak (8 TB/s data sheet; re-reads may be served by the caches)
  rmatmul_ms   gnx_geno_rmatmul (fp32, device tensors) at the same n and k = m beside it: the
               host clock around the synchronous call, the yardstick of what fp64 costs
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

import bench  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12     # FLOP/s
HBM_PEAK = 8.0e12              # bytes/s


def stats(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3),
                max=round(max(v), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c4_metric', choices=sorted(bench.WORKLOADS))
    ap.add_argument('--n', type=int, default=8192)
    ap.add_argument('--ms', default='8,16,24,32')
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'assoc_bench.txt'))
    a = ap.parse_args()
    import torch
    torch.cuda.init()       # torch's HIP runtime first, the library's handles behind it (bench.py)
    cfg = bench.WORKLOADS[a.workload]
    dev, _, _ = bench.build_device(cfg, 1, 0)
    bench.setup_genomes(dev, cfg, 1)
    dev.walk(a.steps, False, True)
    N, L, W64 = int(dev.N), int(cfg['L']), int(dev.W64)
    lines = ['# tools/assoc_bench.py --workload %s: N = %d, L = %d, walked %d steps; HIP events '
             'around the kernels of gnx_assoc_cross, host clock around the synchronous calls, %d '
             'repetitions after one warm-up' % (a.workload, N, L, a.steps, a.reps)]

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    tdev = torch.device('cuda', int(dev.cfg.device))
    rng = np.random.RandomState(1)
    sample = np.sort(rng.choice(N, min(a.n, N), replace=False)).astype(np.int64)
    for slots in (sample, None):
        n = N if slots is None else int(slots.size)
        for m in [int(x) for x in a.ms.split(',')]:
            Y = rng.standard_normal((n, m))
            Yt = torch.as_tensor(Y, dtype=torch.float32, device=tdev)
            got = dev.assoc_cross(Y, slots)                       # warm-up
            dev.geno_rmatmul(Yt, slots)
            k_ms, c_ms, r_ms = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                got = dev.assoc_cross(Y, slots)
                c_ms.append((time.perf_counter() - t0) * 1e3)
                k_ms.append(got['kernel_ms'])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev.geno_rmatmul(Yt, slots)
                r_ms.append((time.perf_counter() - t0) * 1e3)
            mc = 16 if (m + 15) // 16 * 16 <= (m + 7) // 8 * 8 else 8
            blocks = -(-m // mc)
            sec = statistics.median(k_ms) * 1e-3
            fma = float(n) * L * blocks * mc
            gbytes = float(n) * 2 * W64 * 8 * blocks
            emit(n=n, L=L, m=m, column_block=mc, column_blocks=blocks, stretch=got['stretch'],
                 stretches=got['stretches'], kernel_ms=stats(k_ms), call_ms=stats(c_ms),
                 fma=fma, fp64_tflops=round(2.0 * fma / sec / 1e12, 3),
                 fp64_share_of_vector_peak=round(2.0 * fma / sec / FP64_VECTOR_PEAK, 4),
                 genome_bytes=gbytes, genome_tb_per_s=round(gbytes / sec / 1e12, 3),
                 genome_share_of_hbm_peak=round(gbytes / sec / HBM_PEAK, 4),
                 rmatmul_fp32_call_ms=stats(r_ms))
            del Yt
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
