"""gnx_circuit_matrix (csrc/gnx_circuit.hip) against the host restatement: one JSON line per case.

    python tools/circuit_bench.py                          # the 66 x 70 cases, 256^2, 1024^2
    python tools/circuit_bench.py --sides 256 --no-host    # the device alone
    python tools/circuit_bench.py --lib path/to/libgnxhip.so --sides 256
                                                   # a variant build (another CIRC_CHECK)
    python tools/circuit_bench.py --out profiles/circuit_bench.txt

The serpentine cases are those of tests/test_gpu_circuit.py (14 focal cells, 11 systems).  The
square cases: R = 1 / max(U(0, 1), 0.05), 64 focal cells drawn without replacement, res (1, 1).
Every call is synchronous and ends with its download: the host clock around the call is the
time to solution (one warm-up, then the best of `reps`); kernel_ms, launches and iterations are
gnx_circuit_info's.  The host's time is sim/circuit.numpy_resistance_matrix (one splu
factorisation of the grounded Laplacian and 64 solves).  The rate is the bytes one iteration
must move per system and cell - k_circ_dir reads r and p and writes p' and L p', k_circ_update
reads p', L p', x and r and writes x and r: 10 doubles - over the kernel time, and that as a
fraction of the library's copy rate (gnx_measure_copy, read + write bytes); the conductance
rasters, shared by all systems, are not counted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))      # tests/test_gpu_parity.py imports it

from geonomics_amd import _native as nat  # noqa: E402
from geonomics_amd.sim import circuit as Q  # noqa: E402

LINES = []


def emit(**kw):
    line = json.dumps(kw)
    LINES.append(line)
    print(line, flush=True)


def device(H, W):
    dev = nat.Device(W, H, 1)
    dev.upload_rasters(np.ones((1, H, W), np.float32))
    return dev


def timed(fn, reps):
    fn()
    best = np.inf
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t)
    return out, best


def case(label, R, res, cells, reps, host, copy):
    dev = device(*R.shape)
    try:
        got, t_dev = timed(lambda: dev.circuit_matrix(R, res, cells), reps)
        info = dev.circuit_info()
    finally:
        dev.close()
    n_sys = int(np.isfinite(got[0]).sum()) - 1
    moved = 10 * 8 * R.size * n_sys * info['iterations']
    rate = moved / (info['kernel_ms'] * 1e-3) / 1e9
    out = dict(case=label, shape=list(R.shape), res=list(res), cells=int(len(cells)),
               device_s=round(t_dev, 5), kernel_ms=round(info['kernel_ms'], 3),
               launches=info['launches'], iterations=info['iterations'],
               restarts=info['restarts'], worst_residual=info['worst_residual'],
               GBps=round(rate, 1), of_copy=None if not copy else round(rate / copy, 3))
    if host:
        t = time.perf_counter()
        ref = Q.numpy_resistance_matrix(R, res, cells)
        out['host_s'] = round(time.perf_counter() - t, 4)
        ok = np.isfinite(ref)
        out['max_rel_diff'] = float((np.abs(got[ok] - ref[ok]) / np.maximum(ref[ok], 1e-300)).max())
    emit(**out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sides', type=int, nargs='*', default=[256, 1024])
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--no-snake', action='store_true')
    ap.add_argument('--no-copy', action='store_true')
    ap.add_argument('--lib', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.lib:
        nat.LIB_PATH = os.path.abspath(a.lib)
    copy = None if a.no_copy else nat.measure_copy()
    emit(lib=os.path.relpath(nat.LIB_PATH, ROOT), copy_GBps=copy)
    if not a.no_snake:
        from test_gpu_circuit import RES, serpentine
        R, cells = serpentine()
        for res in RES:
            case('serpentine', R, res, cells, a.reps, not a.no_host, copy)
    for side in a.sides:
        rng = np.random.RandomState(side)
        R = 1.0 / np.maximum(rng.rand(side, side), 0.05)
        cells = np.sort(rng.choice(side * side, 64, replace=False)).astype(np.int32)
        case('random', R, (1.0, 1.0), cells, a.reps, not a.no_host, copy)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
