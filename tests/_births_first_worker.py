"""The late-launch scenarios of test_gpu_births_first.py, run in a process of their own.

Which handles hold the crossover back for the next step's pair list (xo_launch_late) is decided
at gnx_create from GNX_DD_MAX_CAP, which the library reads once per process: the test starts this
file with GNX_DD_MAX_CAP=1024 and GNX_DD=0, so that handles of a few thousand slots take the
path bench.py's 2^20 slots take, and compares what it leaves (one .npz) with twins it makes
itself under the default threshold.

    python tests/_births_first_worker.py OUT.npz

The helpers (make_main, state, advance) are the test's as well."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, 'oracle'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

# the issue's model: a 256 x 256 two-layer landscape, ~8 000 individuals, 2 048 loci, 2 traits of
# 8 loci, conductance-surface movement, sparse recombination paths
CFG = dict(W=256, H=256, L=2048, n_traits=2, loci_per_trait=8, n_paths=256)
CAP = 32768
_cache = {}


def _shared(W64):
    if not _cache:
        import bench
        lyr0 = bench.smooth_field(CFG['W'], CFG['H'], 1) * 0.5 + 0.5
        lyr1 = np.tile(np.linspace(0, 1, CFG['W'], dtype=np.float32), (CFG['H'], 1))
        _cache['rasts'] = np.stack([lyr0, lyr1])
        _cache['paths'] = bench.sparse_paths(CFG['n_paths'], CFG['L'], 43, W64)
    return _cache


def make_main(cap_inds=CAP, N=8000, seed=42):
    """three burn-in steps, then genomes assigned (bench.build_device + bench.setup_genomes)"""
    from geonomics_amd import _native as nat
    L = CFG['L']
    sh = _shared(nat.load().gnx_words_per_hom(L))
    rasts = sh['rasts']
    dev = nat.Device(CFG['W'], CFG['H'], 2, L=L, n_traits=CFG['n_traits'], cap_inds=cap_inds,
                     cap_rows=cap_inds, seed=seed)
    dev.upload_rasters(rasts)
    dev.set_species_params(nat.default_species_params(
        mating_radius=10.0, K_layer=0, K_factor=N / float(rasts[0].sum()),
        move_surf=nat.SURF_MIXTURE, move_surf_layer=0, move_surf_kappa=12.0))
    rng = np.random.RandomState(seed)
    n = CFG['loci_per_trait']
    loci = np.sort(rng.choice(L, CFG['n_traits'] * n, replace=False)).reshape(CFG['n_traits'], -1)
    for t in range(CFG['n_traits']):
        alpha = 0.1 * np.array([1 - (i % 2) * 2 for i in range(n)], float)
        dev.set_trait(t, np.sort(loci[t]), alpha, 1, 0.05, 1.0, False)
    dev.init_population(N)
    for _ in range(3):
        dev.step(True, False)
    dev.set_recomb_paths(sh['paths'])
    dev.assign_genomes(np.full(L, dev.N, dtype=np.int32))
    dev.reset_path_counts()
    return dev, nat


def state(dev, nat):
    """every column and every living genome, id by id"""
    ids = dev.download(nat.F_ID)
    o = np.argsort(ids)
    return dict(ids=ids[o], x=dev.download(nat.F_X)[o], y=dev.download(nat.F_Y)[o],
                age=dev.download(nat.F_AGE)[o], sex=dev.download(nat.F_SEX)[o],
                fit=dev.download(nat.F_FIT)[o], z=dev.download(nat.F_Z)[:, o],
                e=dev.download(nat.F_E)[:, o], g=dev.download(nat.F_GENO)[o])


def advance(dev, plan):
    """plan: ('walk', T) and ('step', T) pieces; (N at the start, births, deaths) of every step"""
    hist = []
    for via, T in plan:
        if via == 'walk':
            dev.walk(T, False, True)
            hist += [tuple(int(v) for v in r) for r in zip(*dev.walk_history())]
        else:
            for _ in range(T):
                n0 = dev.N
                dev.step(False, True)
                hist.append((n0,) + tuple(int(v) for v in dev.counts()[1:]))
    return np.array(hist, np.int64)


PLAN = [('walk', 9), ('step', 1), ('walk', 5)]


def _put(out, tag, st, hist=None, pc=None):
    for k, v in st.items():
        out['%s/%s' % (tag, k)] = v
    if hist is not None:
        out['%s/hist' % tag] = hist
    if pc is not None:
        out['%s/pc' % tag] = np.array([pc[k] for k in sorted(pc)], np.int64)
        out['pc_names'] = np.array(sorted(pc))


def scenario_walk(out):
    """walk(9), one gnx_step, walk(5); and 15 single steps of a twin - both on the late path"""
    for tag, plan in (('walk', PLAN), ('steps', [('step', 15)])):
        dev, nat = make_main()
        hist = advance(dev, plan)
        assert dev.genome_info()['deferred'] == 0
        _put(out, tag, state(dev, nat), hist, dev.path_counts())
        assert dev.debug_halves()[1] == 0
        dev.close()


def scenario_walk_many(out):
    """two handles side by side; each against its own single-handle walk (the test's side)"""
    a, nat = make_main(seed=42)
    b, _ = make_main(seed=7)
    nat.walk_many([a, b], 4, False, True)
    hists = [np.array([tuple(int(v) for v in r) for r in zip(*dev.walk_history())], np.int64)
             for dev in (a, b)]
    for _ in range(2):                    # ... and gnx_step_many: all begins, all mids, all ends
        nat.step_many([a, b], False, True)
    for dev, tag, hist in ((a, 'many42', hists[0]), (b, 'many7', hists[1])):
        _put(out, tag, state(dev, nat), hist, dev.path_counts())
        dev.close()
    for seed in (42, 7):
        dev, nat = make_main(seed=seed)
        hist = advance(dev, [('walk', 4)])
        advance(dev, [('step', 2)])
        _put(out, 'alone%d' % seed, state(dev, nat), hist, dev.path_counts())
        dev.close()


def scenario_no_pairs(out):
    """a step without a single pair right behind a step with births: the births' crossover is
    still held back when gnx_l_mate returns early, and must be launched there - once.  b = 0
    for that step: the keep draws u < b keep nobody whatever the seed (the oracle's
    D.keep_draws(seed, ids, step, 0.0) is all False, asserted).  The oracle replays every
    crossover from the births a twin driven through the split step reads out, as
    test_gpu_product_path.py does."""
    import gnx_draws as D
    from test_gpu_product_path import _make, _paths, HostGenomes, _split_step, N0
    from geonomics_amd import _native as nat
    paths = _paths(False)
    a, g = _make(paths, cap_inds=8192)
    b, _ = _make(paths)
    a.reset_path_counts()
    host = HostGenomes(np.arange(N0), g, paths)
    rec = []
    for t in range(7):
        if t in (3, 4):
            sp = nat.default_species_params(mating_radius=3.0, K_factor=1.0, max_age=-1,
                                            b=0.0 if t == 3 else 0.2)
            for dev in (a, b):
                dev.set_species_params(sp)
        if t == 3:
            assert not D.keep_draws(29, a.download(nat.F_ID), a.step_index, 0.0).any()
        p0 = a.path_counts()
        a.step(False, True)
        p1 = a.path_counts()
        _split_step(b, host, t)
        assert a.counts() == b.counts(), t
        rec.append((a.counts()[1], p1['xo_launch_p2'] - p0['xo_launch_p2'],
                    p1['xo_flush'] - p0['xo_flush']))
        if t == 3:
            # the offspring of step 2 that lived: their genomes, right behind the step without pairs
            host.check(a, nat, 'behind the step without pairs')
        assert a.genome_info()['deferred'] == 0
    host.check(a, nat, 'late path, 7 steps')
    host.check(b, nat, 'split step, 7 steps')
    out['nopairs/rec'] = np.array(rec, np.int64)
    a.close()
    b.close()


def scenario_capacity(out):
    """b = 1 for one step on a handle with room for a usual step only: the births do not fit, the
    step returns the capacity code (2) with the last step's crossover still held back - and the
    living's genomes are what a twin holds before that step"""
    from test_gpu_product_path import _make, _paths
    from geonomics_amd import _native as nat
    paths = _paths(False)
    a, _ = _make(paths, cap_inds=2300)
    b, _ = _make(paths, cap_inds=8192)
    for _ in range(3):
        a.step(False, True)
        b.step(False, True)
    sp = nat.default_species_params(mating_radius=3.0, K_factor=1.0, max_age=-1, b=1.0)
    a.set_species_params(sp)
    a.reset_path_counts()
    rc = a.lib.gnx_step(a.h, 0, 1)
    out['cap/rc'] = np.array([rc])
    out['cap/err'] = np.array(a.lib.gnx_last_error().decode())
    pc = a.path_counts()
    out['cap/p2_flush'] = np.array([pc['xo_launch_p2'], pc['xo_flush']], np.int64)
    for dev, tag in ((a, 'cap/a'), (b, 'cap/b')):
        ids = dev.download(nat.F_ID)
        o = np.argsort(ids)
        out[tag + '_ids'] = ids[o]
        out[tag + '_g'] = dev.download_genomes(o.astype(np.int64))
    out['cap/deferred'] = np.array([a.genome_info()['deferred']])
    a.close()
    b.close()


def main(path):
    assert os.environ.get('GNX_DD_MAX_CAP') == '1024' and os.environ.get('GNX_DD') == '0'
    out = {}
    scenario_walk(out)
    scenario_walk_many(out)
    scenario_no_pairs(out)
    scenario_capacity(out)
    np.savez(path, **out)


if __name__ == '__main__':
    main(sys.argv[1])
