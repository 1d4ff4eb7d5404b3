"""Introductions on the device (csrc/gnx_transplant.hip): one JSON line per measurement.

    python tools/add_individuals_bench.py --part c2       # C2: 10^5 x 10^4 into a second C2 handle
    python tools/add_individuals_bench.py --part metric   # c4_metric source, a smaller recipient

The source is bench.py's workload walked 20 steps, so that blocks are shared with parents.  n of
its individuals (random slots) are transplanted into a second handle of the same genome length:
the synchronous call is timed by the host clock around it, best of 5 after 2 warm-ups; between
two calls the newcomers are removed again (gnx_op_mortality, not timed).  Per run: the
milliseconds, D = distinct physical blocks copied, bytes moved = D x 2 x block bytes (read and
written), TB/s over the whole call, and beside it the box's own streaming rate
(gnx_measure_copy).  The same individuals then take the route through the host the library had
before (download_genomes + tile_import + set_z_range), timed the same way.

metric: two c4_metric handles (10^6 individuals, 2 x 10^6 genome rows of 25 KB each) may not
fit one device side by side; the recipient here is a c4_metric landscape with 10^5 individuals
and room for 10^5 more.  What happened at creation is part of the output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from geonomics_amd import _native as nat  # noqa: E402


NEXT_ID = [10 ** 9]          # ids for the next newcomers: above everything handed out so far


def emit(**kw):
    print(json.dumps(kw), flush=True)


def make(cfg, seed, steps, cap_factor=2.0):
    dev, _, _ = bench.build_device(cfg, seed, 0, cap_factor=cap_factor)
    bench.setup_genomes(dev, cfg, seed)
    if steps:
        dev.walk(steps, False, True)
    return dev


def remove_newcomers(dst, first_slot):
    dead = np.zeros(dst.N, np.uint8)
    dead[first_slot:] = 1
    dst.op_mortality(dead)
    assert dst.N == first_slot


def device_route(dst, src, slots, x, y, ids):
    t0 = time.perf_counter()
    out = dst.transplant(src, slots, x, y, ids)
    return time.perf_counter() - t0, out


def host_route(dst, src, slots, x, y, ids):
    """what a caller had to do before: genomes and columns through host buffers"""
    t0 = time.perf_counter()
    geno = src.download_genomes(slots)
    rec = np.zeros(slots.size, nat.IND_REC)
    rec['x'], rec['y'] = x, y
    rec['age'] = src.download(nat.F_AGE)[slots]
    rec['sex'] = src.download(nat.F_SEX)[slots]
    rec['id'] = ids + np.arange(slots.size)
    rec['fit'] = 1.0
    N0 = dst.N
    dst.tile_import(rec, None, geno)
    dst.set_z_range(N0, slots.size)
    return time.perf_counter() - t0, dict(first_slot=N0)


def measure(name, dst, src, n, copy_gbps, reps=5, warm=2):
    info = src.genome_info()
    block_bytes = info['BW'] * 8
    rng = np.random.RandomState(n)
    slots = np.sort(rng.choice(src.N, n, replace=False)).astype(np.int64)
    x = (rng.rand(n) * dst.W * 0.999).astype(np.float32)
    y = (rng.rand(n) * dst.H * 0.999).astype(np.float32)
    next_id = NEXT_ID
    res = {}
    for route, fn in (('device', device_route), ('host', host_route)):
        t, outs = [], []
        for r in range(warm + reps):
            dt, out = fn(dst, src, slots, x, y, next_id[0])
            next_id[0] += n
            remove_newcomers(dst, out['first_slot'])
            if r >= warm:
                t.append(dt)
                outs.append(out)
        res[route] = min(t)
        line = dict(workload=name, route=route, n=n, N_source=src.N, N_recipient=dst.N,
                    ms=[round(v * 1e3, 3) for v in t], ms_best=round(min(t) * 1e3, 3))
        if route == 'device':
            D = outs[int(np.argmin(t))]['blocks_copied']
            moved = D * 2.0 * block_bytes
            line.update(D=D, logical_blocks=outs[0]['blocks_linked'],
                        shared_fraction=round(1 - D / outs[0]['blocks_linked'], 4),
                        block_bytes=block_bytes, bytes_moved=moved,
                        tb_per_s=round(moved / min(t) / 1e12, 4),
                        measured_copy_tb_per_s=round(copy_gbps / 1e3, 3),
                        collections=[o['collections'] for o in outs],
                        flat_bytes_host_route=n * 2 * src.W64 * 8)
        emit(**line)
    emit(workload=name, what='host_over_device', n=n,
         ratio=round(res['host'] / res['device'], 1))


def blocks(name, dev):
    rows, broken, _, used, free, total = (int(v) for v in dev.debug_halves())
    emit(workload=name, what='source_blocks', N=dev.N, logical_blocks=2 * rows,
         live_physical_blocks=used, shared_fraction=round(1 - used / (2.0 * rows), 4))


def part_c2(copy_gbps):
    cfg = bench.WORKLOADS['c2']
    src = make(cfg, 1, 20)
    blocks('c2', src)
    # (room for the source's 10^5 besides its own 10^5)
    dst = make(cfg, 2, 0, cap_factor=2.3)
    for n in (1000, 100000):
        measure('c2', dst, src, min(n, src.N), copy_gbps)
    dst.close()
    src.close()


def part_metric(copy_gbps):
    cfg = bench.WORKLOADS['c4_metric']
    src = make(cfg, 1, 20)
    blocks('c4_metric', src)
    info = src.genome_info()
    emit(workload='c4_metric', what='source_handle', row_spread=info['row_spread'], NB=info['NB'],
         BW_words=info['BW'])
    small = dict(cfg, N=100_000)
    dst = make(small, 2, 0, cap_factor=2.3)
    emit(workload='c4_metric', what='recipient', N=dst.N, cap_rows=int(dst.cfg.cap_rows),
         row_spread=dst.genome_info()['row_spread'])
    for n in (1000, 100000):
        measure('c4_metric', dst, src, n, copy_gbps)
    dst.close()
    # a second handle of the metric size beside the first: tried only when the device reports
    # the room for its genome table (compact, row_spread 1) and its per-slot arrays
    import torch
    free_b, total_b = torch.cuda.mem_get_info()
    cap = int(cfg['N'] * 2.0) + 1024
    need = cap * (2 * info['NB'] * info['BW'] * 8 + 2048)
    line = dict(workload='c4_metric', what='second_metric_handle', free_gb=round(free_b / 1e9, 1),
                total_gb=round(total_b / 1e9, 1), need_gb=round(need / 1e9, 1))
    if free_b < 1.1 * need:
        emit(fits=False, tried=False, **line)
    else:
        try:
            twin = make(cfg, 2, 0)
            out = twin.transplant(src, np.arange(1000), np.full(1000, 5.0), np.full(1000, 5.0),
                                  NEXT_ID[0])
            emit(fits=True, tried=True, row_spread=twin.genome_info()['row_spread'],
                 transplant_1000=out, **line)
            twin.close()
        except nat.GnxError as e:
            emit(fits=False, tried=True, error=str(e)[:200], **line)
    src.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['c2', 'metric'], required=True)
    a = ap.parse_args()
    import torch
    torch.cuda.init()           # torch's HIP runtime first, the library's handles behind it (bench.py)
    gbps = nat.measure_copy()
    emit(what='measured_copy', gb_per_s=round(gbps, 1))
    part_c2(gbps) if a.part == 'c2' else part_metric(gbps)
