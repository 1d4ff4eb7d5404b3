"""The next step's movement launched by the lazy mortality (gnx_l_move_ahead).

Inside gnx_walk of ONE handle every step but the last leaves its dead in their slots, and the
movement of the step after it is enqueued right behind the death draws, on the side stream,
where it runs beside the crossover's job builder.  Every draw is keyed by (seed, id, step, op) and
no kernel's arithmetic changes, so a walk must equal the same number of single gnx_step calls
bit for bit: every column by id, the counts of every step, every genome.  The path counters
prove which path a handle took.

The model is the benchmark's own at a size a test can afford (bench.WORKLOADS['small']: a
256 x 256 two-layer landscape, ~20 000 individuals, 10 000 loci, 4 traits of 10 loci,
conductance-surface movement, sparse paths, genomes assigned after three burn-in steps); the
capacity only sizes allocations and picks the path (above 600 000 slots: the 512-thread job
builder and the crossover launched behind the next step's pair list).  Only there does the
movement run ahead: where the crossover is launched as soon as its jobs are built (small
capacities, crossover overlap mode 1) it is on the side stream first, and a movement behind it
would make the next cell sort wait for the whole crossover.

Not covered: a walk on a handle with ghosts - the bindings import ghosts through the tile
protocol only (tile_import_ghosts between gnx_tile_* calls), and tiles never move ahead.
Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

CFG = dict(W=256, H=256, L=10_000, n_traits=4, loci_per_trait=10, n_paths=1_000)
BIG = 1 << 20          # slots: the path bench.py's metric workload takes
SMALL = 16384          # ... and the host-driven small path (GNX_DD=0), 256-thread job builder
_cache = {}


def _shared(W64):
    """rasters and recombination paths, made once"""
    if not _cache:
        import bench
        lyr0 = bench.smooth_field(CFG['W'], CFG['H'], 1) * 0.5 + 0.5
        lyr1 = np.tile(np.linspace(0, 1, CFG['W'], dtype=np.float32), (CFG['H'], 1))
        _cache['rasts'] = np.stack([lyr0, lyr1])
        _cache['paths'] = bench.sparse_paths(CFG['n_paths'], CFG['L'], 43, W64)
    return _cache


def _make(cap_inds, N=20_000, seed=42, late_sp=None, overlap=0, **sp_kw):
    """bench.build_device + bench.setup_genomes of the small workload, with a capacity of the
    test's choosing (and few genome rows: 2^20 of them would be 2.6 GB for nothing);
    late_sp: species parameters set after the genomes are assigned"""
    from geonomics_amd import _native as nat
    L = CFG['L']
    sh = _shared(nat.load().gnx_words_per_hom(L))
    rasts = sh['rasts']
    dev = nat.Device(CFG['W'], CFG['H'], 2, L=L, n_traits=CFG['n_traits'], cap_inds=cap_inds,
                     cap_rows=min(cap_inds, 65536), seed=seed)
    dev.upload_rasters(rasts)
    kw = dict(mating_radius=10.0, K_layer=0, K_factor=N / float(rasts[0].sum()),
              move_surf=nat.SURF_MIXTURE, move_surf_layer=0, move_surf_kappa=12.0)
    kw.update(sp_kw)
    dev.set_species_params(nat.default_species_params(**kw))
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
    if late_sp:
        kw.update(late_sp)
        dev.set_species_params(nat.default_species_params(**kw))
    if overlap:
        dev.set_crossover_overlap(overlap)
    dev.reset_path_counts()
    return dev, nat


def _state(dev, nat, genomes=True):
    ids = dev.download(nat.F_ID)
    o = np.argsort(ids)
    out = dict(ids=ids[o], x=dev.download(nat.F_X)[o], y=dev.download(nat.F_Y)[o],
               age=dev.download(nat.F_AGE)[o], sex=dev.download(nat.F_SEX)[o],
               fit=dev.download(nat.F_FIT)[o], z=dev.download(nat.F_Z)[:, o],
               e=dev.download(nat.F_E)[:, o])
    if genomes and ids.size:
        out['g'] = dev.download(nat.F_GENO)[o]
    return out


def _advance(dev, via, T):
    """T steps through gnx_walk or as single gnx_step calls; (N at the start, births, deaths)"""
    if via == 'walk':
        dev.walk(T, False, True)
        return [tuple(int(v) for v in r) for r in zip(*dev.walk_history())]
    hist = []
    for _ in range(T):
        n0 = dev.N
        dev.step(False, True)
        hist.append((n0,) + tuple(dev.counts()[1:]))
    return hist


def _mutate_and_collect(dev, nat):
    """one host-side mutation of a few living individuals, picked by id, and a forced collection
    of the shared genome blocks"""
    rng = np.random.RandomState(17)
    have = dev.download(nat.F_ID)
    o = np.argsort(have)
    pick = rng.choice(have[o], 8, replace=False)
    loci = rng.randint(1, CFG['L'], 8).astype(np.int32)
    homs = rng.randint(0, 2, 8).astype(np.uint8)
    dev.mutate(o[np.searchsorted(have[o], pick)].astype(np.int64), loci, homs)
    rows, broken, _, used, free, total = (int(v) for v in dev.debug_halves())
    assert broken == 0 and used + free == total


def _run(via, cap_inds, pieces, between=False, genomes=True, **mk):
    dev, nat = _make(cap_inds, **mk)
    hist = []
    for k, T in enumerate(pieces):
        if k and between:
            _mutate_and_collect(dev, nat)
        hist += _advance(dev, via, T)
    out = _state(dev, nat, genomes)
    out['hist'] = hist
    pc = dev.path_counts()
    assert dev.debug_halves()[1] == 0          # no broken block references
    dev.close()
    return out, pc


def _same(a, b, what=''):
    assert a['hist'] == b['hist'], what
    assert set(a) == set(b), what
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s %s' % (what, k))


@pytest.mark.parametrize('case', ['big', 'small', 'overlap1'])
def test_walk_equals_steps_on_the_benchmark_path(case, monkeypatch):
    """walk(5), a mutation, a forced block collection, walk(4) against nine gnx_step calls with
    the same in between: every column by id, the counts of every step and every genome.
    big: 2^20 slots, the 512-thread job builder, the crossover behind the next pair list - the
    movement runs ahead in every step of a walk but its last.
    small: 16 384 slots with GNX_DD=0, the host-driven walk of the small path, 256-thread builder
    (8 000 individuals: 20 000 and a step's births do not fit 16 384 slots).  The crossover is
    launched on the side stream as soon as its jobs are built, so nothing moves ahead (it would
    wait behind that crossover): lazy steps as before, same results.
    overlap1: 2^20 slots with the narrow crossover that stretches over the whole next step
    (gnx_set_crossover_overlap 1), launched at once as well: nothing moves ahead either."""
    cap_inds = SMALL if case == 'small' else BIG
    if case == 'small':
        monkeypatch.setenv('GNX_DD', '0')
    N = 8_000 if case == 'small' else 20_000
    overlap = 1 if case == 'overlap1' else 0
    a, pa = _run('walk', cap_inds, (5, 4), between=True, N=N, overlap=overlap)
    b, pb = _run('step', cap_inds, (5, 4), between=True, N=N, overlap=overlap)
    assert a['ids'].size > 0.7 * N
    _same(a, b)
    assert pa['lazy_mortalities'] == 4 + 3 and pa['moves_ahead'] == (7 if case == 'big' else 0), pa
    assert pa['sort_hist_gather'] >= 7 and pa['make_dense'] == 0, pa
    if case == 'small':
        assert pa['jobs_lanes_256'] > 0 and pa['jobs_lanes_512'] == 0, pa
    else:
        assert pa['jobs_lanes_512'] > 0 and pa['jobs_lanes_256'] == 0, pa
    assert (pa['xo_launch_p2'] > 0) == (case == 'big'), pa
    assert pb['moves_ahead'] == 0 and pb['lazy_mortalities'] == 0, pb


@pytest.mark.parametrize('T', [1, 2])
def test_the_last_step_never_moves_ahead(T):
    """walk(1) launches no movement ahead, walk(2) exactly one; a movement applied one step early
    (or twice) would show as ages off by one and other positions"""
    a, pa = _run('walk', BIG, (T,), genomes=False)
    b, _ = _run('step', BIG, (T,), genomes=False)
    assert pa['moves_ahead'] == T - 1 and pa['lazy_mortalities'] == T - 1, pa
    _same(a, b)


def test_several_handles_never_move_ahead():
    """gnx_walk_many stops every handle when one fails: with two handles nobody's next step is
    certain, nobody moves ahead, and each equals its own single-handle walk (which does)"""
    a, nat = _make(BIG, seed=42)
    b, _ = _make(BIG, seed=7)
    nat.walk_many([a, b], 3, False, True)
    for dev, seed in ((a, 42), (b, 7)):
        pc = dev.path_counts()
        assert pc['moves_ahead'] == 0 and pc['lazy_mortalities'] == 2, pc
        got = _state(dev, nat)
        got['hist'] = [tuple(int(v) for v in r) for r in zip(*dev.walk_history())]
        dev.close()
        alone, pal = _run('walk', BIG, (3,), seed=seed)
        assert pal['moves_ahead'] == 2, pal
        _same(got, alone, 'seed %d' % seed)


@pytest.mark.parametrize('case', ['no_movement', 'panmixia'])
def test_paths_that_stay_off(case):
    """a species that does not move and one that mates at any distance take no lazy step, so
    nothing is launched ahead - and the walk equals the steps"""
    kw = dict(move=0) if case == 'no_movement' else dict(mating_radius=-1.0)
    a, pa = _run('walk', BIG, (4,), genomes=False, **kw)
    b, _ = _run('step', BIG, (4,), genomes=False, **kw)
    assert pa['moves_ahead'] == 0 and pa['lazy_mortalities'] == 0, pa
    _same(a, b)
    assert a['ids'].size > 10_000


def test_extinction_inside_a_walk():
    """death probabilities of 0.99 .. 1 from the first main step on: 20 000 -> ~100 -> ~1 -> 0.
    The mortality that kills the last ones has already launched the next movement (every slot is
    flagged dead: it writes nothing); the walk goes on without an error, its history equals the
    steps', and a walk of the empty handle is a no-op."""
    deadly = dict(d_min=0.99, d_max=1.0)
    a, nat = _make(BIG, late_sp=deadly)
    b, _ = _make(BIG, late_sp=deadly)
    ha = _advance(a, 'walk', 6)
    hb = _advance(b, 'step', 6)
    assert ha == hb and ha[0][0] > 15_000
    assert a.N == 0 and b.N == 0
    pa = a.path_counts()
    # every step up to and including the one that killed the last individuals launched the next
    # movement (none of them was the walk's last): the extinction step's own is the no-op
    k = 1 + next(i for i, (n0, bb, dd) in enumerate(ha) if n0 + bb - dd == 0)
    assert 2 <= k <= 5 and pa['moves_ahead'] == k and pa['make_dense'] == 0, pa
    assert _advance(a, 'walk', 2) == _advance(b, 'step', 2) == [(0, 0, 0)] * 2
    assert a.N == 0 and a.path_counts()['moves_ahead'] == pa['moves_ahead']
    a.close()
    b.close()
