"""Model.prune_ld / calc_ld_scores on the device (csrc/gnx_ldwin.hip, sim/ldwin.py): one JSON
line per measurement, printed and written to profiles/ldwin_bench.txt (--out).

    python tools/ldwin_bench.py                  # L = 10^5, 20 000 individuals on the handle

The genomes are mosaics of 8 founder haplotypes in stretches of 256 loci, so that linkage
disequilibrium is real and the pair list long.  gnx_ld_window is synchronous and ends with its
downloads: `call_ms` is the host clock around it, `kernel_ms` the HIP-event time of its kernels
(gnx_ld_window_info).
  edges     windows of 100 and 1000 loci, samples of 2000 and 20 000 individuals, the pairs with
            r^2 >= 0.2 among the loci at 5 % (prune_ld's request) without the scores
  scores    the same requests, counts and sums only (calc_ld_scores' request)
  greedy    sim/ldwin.greedy_independent on each of those pair lists, on the host
  host      what there is without the entry point: the sample's genomes downloaded, unpacked,
            and sim/ldwin.brute_window over blocks of 1024 loci with their window's halo; timed
            on --host-blocks blocks and scaled to all of them
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from geonomics_amd import _native as nat  # noqa: E402
from geonomics_amd.sim import ld as LD  # noqa: E402
from geonomics_amd.sim import ldwin as LW  # noqa: E402

BIG = 1 << 60
LINES = []


def emit(**kw):
    LINES.append(json.dumps(kw))
    print(LINES[-1], flush=True)


def mosaic(n, L, W64, seed, founders=8, seg_words=4):
    """uint64 [n][2][W64]: every chromosome copies one of `founders` random haplotypes per
    stretch of seg_words words; the bits past L are 0"""
    rng = np.random.RandomState(seed)
    nseg = (W64 + seg_words - 1) // seg_words
    F = rng.randint(0, 1 << 32, size=(founders, nseg, seg_words, 2)).astype(np.uint64)
    F = (F[..., 0] << np.uint64(32)) | F[..., 1]
    idx = rng.randint(0, founders, size=(2 * n, nseg))
    G = F[idx, np.arange(nseg)[None, :]].reshape(2 * n, nseg * seg_words)[:, :W64].copy()
    full, rest = divmod(L, 64)
    if rest:
        G[:, full] &= np.uint64((1 << rest) - 1)
        full += 1
    G[:, full:] = 0
    return G.reshape(n, 2, W64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--L', type=int, default=100000)
    ap.add_argument('--N', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-blocks', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ldwin_bench.txt'))
    a = ap.parse_args()
    N, L = a.N, a.L
    dev = nat.Device(64, 64, 1, L=L, n_traits=0, cap_inds=N + 64, cap_rows=N + 64, seed=1)
    dev.upload_rasters(np.ones((1, 64, 64), np.float32))
    dev.set_species_params(nat.default_species_params())
    rng = np.random.RandomState(0)
    dev.upload_population(rng.uniform(0, 64, N).astype(np.float32),
                          rng.uniform(0, 64, N).astype(np.float32), np.zeros(N), np.zeros(N),
                          np.arange(N))
    dev.upload_genomes(mosaic(N, L, dev.W64, 2))
    loci, pos = np.arange(L), np.arange(L, dtype=np.float64)
    lists = {}
    for n in sorted({min(2000, N), N}):
        slots = np.sort(rng.choice(N, n, replace=False)).astype(np.int64)
        mm = LD.min_minor(0.05, 2 * n)
        for window in (100.0, 1000.0):
            for what, r2, cap, scores in (('edges', 0.2, 1 << 25, False),
                                          ('scores', 0.0, 0, True)):
                def call():
                    return dev.ld_window(loci, pos, window, slots, mm, r2, cap, BIG, scores)
                try:
                    got = call()
                except nat.GnxError as err:
                    emit(what=what, n=n, window=window, refused=str(err))
                    continue
                t, k = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    call()
                    t.append(time.perf_counter() - t0)
                    k.append(dev.ld_window_info()['kernel_ms'])
                nq = (2 * n + 63) // 64
                emit(what=what, n=n, L=L, window=window, chromosome_words=nq,
                     kept=int((np.minimum(got['c1'], 2 * n - got['c1']) >= mm).sum()),
                     tiles=got['work'] // nq, work_tile_words=got['work'],
                     n_edges=got['n_edges'], call_ms=[round(x * 1e3, 2) for x in t],
                     kernel_ms=[round(x, 3) for x in k], info=dev.ld_window_info(),
                     popcount_words_per_s=got['work'] * 4096 / (min(k) * 1e-3))
                if what == 'edges':
                    lists[(n, window)] = (got, slots, mm)
    for (n, window), (got, slots, mm) in sorted(lists.items()):
        rank = LW.maf_rank(got['c1'], 2 * n)
        t0 = time.perf_counter()
        keep, _ = LW.greedy_independent(L, got['ei'], got['ej'], rank)
        emit(what='greedy', n=n, window=window, n_edges=got['n_edges'],
             seconds=round(time.perf_counter() - t0, 3),
             kept=int((keep & (np.minimum(got['c1'], 2 * n - got['c1']) >= mm)).sum()))
    # ---- the host route at the smallest request
    (n, window), (got, slots, mm) = sorted(lists.items())[0]
    t0 = time.perf_counter()
    P = dev.download_genomes(slots)
    t_down = time.perf_counter() - t0
    block, halo = 1024, int(window)
    n_blocks = (L + block - 1) // block
    t_blocks = []
    for b in range(min(a.host_blocks, n_blocks)):
        t0 = time.perf_counter()
        j0, j1 = b * block, min(L, (b + 1) * block + halo)
        w0, w1 = j0 // 64, (j1 + 63) // 64
        by = np.ascontiguousarray(P[:, :, w0:w1]).view(np.uint8).reshape(2 * n, -1)
        bits = np.unpackbits(by, axis=1, bitorder='little')[:, j0 - 64 * w0:j1 - 64 * w0]
        ref = LW.brute_window(bits, pos[j0:j1], window, mm, 0.2)
        t_blocks.append(time.perf_counter() - t0)
        sel = (got['ei'] >= j0) & (got['ei'] < min(L, (b + 1) * block))
        own = ref['ei'] < block
        assert (got['ei'][sel] - j0 == ref['ei'][own]).all() and \
            got['er2'][sel].tobytes() == ref['er2'][own].tobytes()
    emit(what='host', n=n, window=window, download_s=round(t_down, 3),
         genome_bytes=int(P.nbytes), block_loci=block, blocks_timed=len(t_blocks),
         block_s=[round(x, 2) for x in t_blocks], blocks=n_blocks,
         scaled_s=round(t_down + n_blocks * min(t_blocks), 1))
    dev.close()
    with open(a.out, 'w') as f:
        f.write('# python tools/ldwin_bench.py on one MI355X (L = %d, %d individuals on the '
                'handle); host clock around the\n# synchronous calls and HIP-event kernel time '
                '(gnx_ld_window_info), %d repetitions\n' % (L, N, a.reps))
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
