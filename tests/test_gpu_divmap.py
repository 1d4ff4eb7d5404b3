"""gnx_divmap_sums (csrc/gnx_divmap.hip) and what stands on it - Device.divmap_sums,
Species._calc_diversity_map, Model.calc_diversity_map - against the four integers per window
taken with numpy from the downloaded genomes.  Every comparison of the integer rasters is
integer equality.  Needs an MI355X.

The counter flushes after 511 individuals of a map cell (GC_CHUNK); a fuller cell spans several
chunks, whose counts meet in the atomic adds.  A locus tile is a run of whole 64-locus words;
max_counts forces several."""
import ctypes as C

import numpy as np
import pytest

import gnx_oracle as O
from test_divmap_host import sums_numpy
from test_gpu_fst import _handle, _random_gts, _unpack
from test_gpu_parity import native
from geonomics_amd.sim import divmap as DM

pytestmark = pytest.mark.gpu

KEYS = ('n', 'S', 'sum_het', 'sum_cc')


def _grouped(lab, cells):
    order = np.argsort(lab, kind='stable')
    return order, np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=cells))])


def _expected(dev, slots, lab_sorted, nx, ny, r, loci=None):
    gts = _unpack(dev.download_genomes(np.asarray(slots, np.int64)), dev.L)
    return sums_numpy(gts, lab_sorted, nx, ny, r, loci)


def _same(got, want):
    for k in KEYS:
        assert got[k].dtype == (np.int32 if k in ('n', 'S') else np.int64), k
        assert got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _check(dev, lab, nx, ny, r, mask=None, loci=None, **kw):
    """the call on slots 0 .. len(lab) - 1 labelled lab, against numpy"""
    order, cs = _grouped(lab, nx * ny)
    got = dev.divmap_sums(order, cs, nx, ny, r, locus_mask=mask, **kw)
    _same(got, _expected(dev, order, lab[order], nx, ny, r, loci))
    return got


def _mask(dev, loci):
    loci = np.asarray(loci, np.int64)
    m = np.zeros(dev.W64, np.uint64)
    np.bitwise_or.at(m, loci >> 6, np.uint64(1) << (loci & 63).astype(np.uint64))
    return m


@pytest.fixture(scope='module')
def small():
    """L = 200 (the last word partial), n = 131, labels on a 5 x 4 map with empty cells"""
    nat = native()
    gts = _random_gts(np.random.RandomState(1), 131, 200)
    dev = _handle(nat, gts)
    lab = np.random.RandomState(2).choice([0, 1, 2, 4, 6, 7, 11, 12, 13, 18, 19], 131)
    yield nat, dev, gts, lab
    dev.close()


def test_small_map_with_empty_cells_twice(small):
    nat, dev, gts, lab = small
    got = _check(dev, lab, 5, 4, 1)
    assert (np.bincount(lab, minlength=20) == 0).sum() == 9 and got['S'].max() > 0
    again = _check(dev, lab, 5, 4, 1)                          # back to back: the same
    _same(again, got)
    # the upload itself, not only the download, is what was counted
    _same(got, sums_numpy(gts, lab, 5, 4, 1))
    np.testing.assert_array_equal(got['n'], DM.box_sum(np.bincount(lab, minlength=20).reshape(4, 5), 1))
    info = dev.divmap_info()
    assert info == dict(tiles=1, chunks=11, launches=3), info
    # individuals in no cell are absent, slots in no order
    keep = np.random.RandomState(3).permutation(131)[:90]
    order, cs = _grouped(lab[keep], 20)
    got = dev.divmap_sums(keep[order], cs, 5, 4, 2)
    _same(got, sums_numpy(gts[keep], lab[keep], 5, 4, 2))


def test_radius_zero_is_group_counts_reduced(small):
    nat, dev, gts, lab = small
    got = _check(dev, lab, 5, 4, 0)
    order, cs = _grouped(lab, 20)
    c1, ch = dev.stats_group_counts(order, cs)
    c1, ch, n = c1.astype(np.int64), ch.astype(np.int64), np.diff(cs)
    m = 2 * n[:, None]
    np.testing.assert_array_equal(got['n'].ravel(), n)
    np.testing.assert_array_equal(got['S'].ravel(), ((c1 > 0) & (c1 < m)).sum(axis=1))
    np.testing.assert_array_equal(got['sum_het'].ravel(), ch.sum(axis=1))
    np.testing.assert_array_equal(got['sum_cc'].ravel(), (c1 * (m - c1)).sum(axis=1))


@pytest.mark.parametrize('r', [5, 6, 1000, 2 ** 31 - 1])
def test_radius_past_the_map_is_the_whole_population(small, r):
    nat, dev, gts, lab = small
    got = _check(dev, lab, 5, 4, r)
    c1, ch = (a.astype(np.int64) for a in dev.stats_locus_counts())
    N = dev.N
    assert (got['n'] == N).all()
    assert (got['S'] == ((c1 > 0) & (c1 < 2 * N)).sum()).all()
    assert (got['sum_het'] == ch.sum()).all()
    assert (got['sum_cc'] == (c1 * (2 * N - c1)).sum()).all()


@pytest.mark.parametrize('nx,ny', [(1, 1), (1, 7), (7, 1)])
def test_degenerate_maps(small, nx, ny):
    nat, dev, gts, lab = small
    lab = lab % (nx * ny)
    for r in (0, 1, 3):
        _check(dev, lab, nx, ny, r)


def test_a_column_longer_than_one_batch_of_windows(small):
    """ny = 1030 > 1024: the column's partial sums go through LDS in two batches, the running
    sums carried across; most windows are empty"""
    nat, dev, gts, lab = small
    lab = np.random.RandomState(8).randint(0, 2 * 1030, 131)
    lab[:6] = [2 * 1023, 2 * 1023 + 1, 2 * 1024, 2 * 1024 + 1, 2 * 1029 + 1, 0]   # at the seam
    for r in (0, 2):
        got = _check(dev, lab, 2, 1030, r)
        assert (got['n'] == 0).any() and got['S'][1020:1028].any()


@pytest.fixture(scope='module')
def wide():
    """L = 4097: 65 words, one past a wave's 64-word tile.  A 3 x 3 map: one cell holds 541
    individuals (two chunks), one a single individual, one nobody"""
    nat = native()
    sizes = [541, 1, 0, 9, 30, 12, 3, 17, 2]
    gts = _random_gts(np.random.RandomState(5), sum(sizes), 4097)
    gts[:, -1] = np.random.RandomState(6).randint(0, 2, (sum(sizes), 2))
    dev = _handle(nat, gts)
    lab = np.random.RandomState(7).permutation(np.repeat(np.arange(9), sizes))
    yield nat, dev, gts, lab
    dev.close()


def test_locus_tiles(wide):
    nat, dev, gts, lab = wide
    one = _check(dev, lab, 3, 3, 1)
    assert dev.divmap_info() == dict(tiles=1, chunks=9, launches=3)
    assert one['S'].max() > 0 and one['n'][0, 0] == 541 + 1 + 9 + 30
    for max_counts, tiles in ((9 * 64 * 25, 3), (9 * 64 * 64, 2), (1, 65)):
        got = _check(dev, lab, 3, 3, 1, max_counts=max_counts)
        info = dev.divmap_info()
        assert info['tiles'] == tiles and info['launches'] == 3 * tiles, info
        _same(got, one)
    _same(one, sums_numpy(gts, lab, 3, 3, 1))


def test_locus_mask(wide):
    nat, dev, gts, lab = wide
    # inside one word; across the border of the 25-word tiles (loci 1599 | 1600); the last locus
    for loci in ([70, 71, 100], [1598, 1599, 1600, 1601], [3, 64, 1599, 1600, 4095, 4096],
                 np.arange(0, 4097, 3)):
        mask = _mask(dev, loci)
        got = _check(dev, lab, 3, 3, 1, mask=mask, loci=loci, max_counts=9 * 64 * 25)
        assert dev.divmap_info()['tiles'] == 3
        assert got['S'].max() <= len(loci)
        _same(got, _check(dev, lab, 3, 3, 1, mask=mask, loci=loci))
    # bits past L in the mask count for nothing
    mask = _mask(dev, [4096])
    mask[64] |= np.uint64(0xFF00)
    mask[70] = np.uint64(2 ** 64 - 1)
    _check(dev, lab, 3, 3, 0, mask=mask, loci=[4096])
    none = dev.divmap_sums(*_grouped(lab, 9), 3, 3, 1, locus_mask=np.zeros(dev.W64, np.uint64))
    assert none['n'].sum() > 0 and not none['S'].any() and not none['sum_cc'].any()


def test_walked_relatives_across_blocks_with_a_pending_crossover():
    """the walk of test_gpu_fst's section: lazy mortality, children sharing blocks with their
    parents, mutations, this step's offspring still waiting for their genomes - then the map"""
    nat = native()
    L = 10000
    rng = np.random.RandomState(7)
    cross = (rng.rand(64, L) < 1.0 / L).astype(np.uint8)
    cross[:, 0] = 0
    paths = O.pack_bits(O.recomb_paths(cross))
    dev = _handle(nat, _random_gts(rng, 700, L), W=28, H=28, cap=1 << 20, cap_rows=4096,
                  paths=paths)
    try:
        info = dev.genome_info()
        assert info['NB'] > 1 and info['BW'] < 64, info     # a wave's 64 words cross blocks
        dev.set_defer_crossover(True)
        for T in (3, 2, 3):
            dev.walk(T, False, False)
            who = rng.choice(dev.N, 5, replace=False).astype(np.int64)
            dev.mutate(who, rng.randint(1, L, 5).astype(np.int32),
                       rng.randint(0, 2, 5).astype(np.uint8))
        dev.age()
        dev.move()
        dev.pop_dynamics_mate(False)
        N = dev.N
        assert dev.counts()[1] > 0 and dev.genome_info()['deferred'] == 1
        assert dev.totals()['deaths'] > 0
        assert dev.path_counts()['lazy_mortalities'] > 0
        assert N >= 511 + 60, N
        lab = rng.randint(1, 16, N)
        lab[rng.permutation(N)[:530]] = 0                  # two chunks in map cell 0
        order, cs = _grouped(lab, 16)
        got = dev.divmap_sums(order, cs, 4, 4, 1, max_counts=16 * 64 * 60)
        assert dev.genome_info()['deferred'] == 0          # the call cut the pending births
        assert dev.path_counts()['make_dense'] == 0        # ... and found the living in [0, N)
        assert dev.divmap_info()['tiles'] == 3 and dev.N == N
        _same(got, _expected(dev, order, lab[order], 4, 4, 1))
    finally:
        dev.close()


def test_every_refusal_leaves_the_handle_alone(small):
    nat, dev, gts, lab = small
    before = dev.stats_locus_counts()
    N = dev.N
    ok, cs6 = np.arange(10), [0, 2, 2, 5, 7, 9, 10]
    for slots, cs, nx, ny, r, msg in (
            (ok, cs6, 0, 6, 1, 'nx, ny at least 1'),
            (ok, cs6, 6, -1, 1, 'nx, ny at least 1'),
            (ok, cs6, 1025, 1024, 1, 'at most 1048576'),
            (ok, cs6, 3, 2, -1, 'r >= 0'),
            (ok, [1, 2, 2, 5, 7, 9, 10], 3, 2, 1, 'start at 0'),
            (ok, [0, 2, 2, 5, 7, 9, 9], 3, 2, 1, 'end at n'),
            (ok, [0, 2, 1, 5, 7, 9, 10], 3, 2, 1, 'decreases at map cell 1'),
            (np.array([0, 1, N]), [0, 3], 1, 1, 0, 'slot out of range'),
            (np.array([0, -1, 2]), [0, 3], 1, 1, 0, 'slot out of range'),
            (np.array([0, 2 ** 40]), [0, 2], 1, 1, 0, 'slot out of range')):
        with pytest.raises(nat.GnxError, match=msg):
            dev.divmap_sums(slots, cs, nx, ny, r)
    with pytest.raises(ValueError, match='cell_start'):
        dev.divmap_sums(ok, [0, 10], 3, 2, 1)
    with pytest.raises(ValueError, match='locus_mask'):
        dev.divmap_sums(ok, cs6, 3, 2, 1, locus_mask=np.zeros(3, np.uint64))

    # through the library itself: the window sizes are checked before any slot is read, so one
    # slot stands in for the 2^30 the call announces; nothing is written to the outputs
    def raw(n, slots, nx, ny, cs, r, outs=None):
        o = [np.full(nx * ny, -7, np.int32), np.full(nx * ny, -7, np.int32),
             np.full(nx * ny, -7, np.int64), np.full(nx * ny, -7, np.int64)] if outs is None else outs
        rc = dev.lib.gnx_divmap_sums(
            dev.h, C.c_int64(n), nat._ptr(slots), C.c_int32(nx), C.c_int32(ny),
            nat._ptr(cs), C.c_int32(r), None, C.c_int64(0),
            nat._ptr(o[0]), nat._ptr(o[1]), nat._ptr(o[2]),
            nat._ptr(o[3]))
        assert all(a is None or (a == -7).all() for a in o)
        return rc, dev.lib.gnx_last_error()
    one = np.zeros(1, np.int32)
    half = 2 ** 29
    rc, err = raw(2 * half, one, 2, 1, np.array([0, half, 2 * half], np.int64), 1)
    assert rc == 1 and b'window of map cell (0, 0) holds 2^30 individuals or more' in err
    # the same cells apart (r = 0): no window reaches 2^30, but 200 * (2^29)^2 >= 2^63
    rc, err = raw(2 * half, one, 2, 1, np.array([0, half, 2 * half], np.int64), 0)
    assert rc == 1 and b"L' * n_max^2" in err and b'2^63' in err
    # within both limits (200 * 2^54 < 2^63) the slots are looked at next
    rc, err = raw(2 ** 27, np.full(1, -1, np.int32), 1, 1, np.array([0, 2 ** 27], np.int64), 0)
    assert rc == 1 and b'slot out of range' in err
    cs1 = np.array([0, 1], np.int64)
    for args in ((1, None, 1, 1, cs1, 0), (1, one, 1, 1, None, 0), (-1, one, 1, 1, cs1, 0)):
        rc, err = raw(*args)
        assert rc == 1 and b'null argument or n < 0' in err
    for k in range(4):
        outs = [np.full(1, -7, np.int32), np.full(1, -7, np.int32), np.full(1, -7, np.int64),
                np.full(1, -7, np.int64)]
        outs[k] = None
        rc, err = raw(1, one, 1, 1, cs1, 0, outs)
        assert rc == 1 and b'null argument or n < 0' in err
    # no genomes
    bare = nat.Device(16, 16, 1, L=100, cap_inds=64, cap_rows=64, seed=1)
    bare.upload_rasters(np.ones((1, 16, 16), np.float32))
    bare.set_species_params(nat.default_species_params())
    bare.upload_population(np.ones(4), np.ones(4), np.zeros(4), np.zeros(4), np.arange(4))
    with pytest.raises(nat.GnxError, match='genomes not assigned'):
        bare.divmap_sums(np.arange(4), [0, 4], 1, 1, 0)
    bare.close()
    # nobody: all-zero rasters
    got = dev.divmap_sums(np.zeros(0, np.int64), np.zeros(21, np.int64), 5, 4, 1)
    for k in KEYS:
        assert got[k].shape == (4, 5) and not got[k].any()
    assert dev.divmap_info() == dict(tiles=0, chunks=0, launches=0)
    after = dev.stats_locus_counts()
    np.testing.assert_array_equal(before[0], after[0])
    np.testing.assert_array_equal(before[1], after[1])


def test_model_calc_diversity_map():
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    mod = gnx.make_model(small_params(T=6))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(4, 'main', verbose=False)
    gts = mod.get_genotypes(biallelic=True).astype(np.uint8)
    nn, L = gts.shape[:2]
    lab = mod.group_by_grid(4, 3)
    want = sums_numpy(gts, lab, 4, 3, 1)
    min_n = int(np.median(want['n']))                      # masks the corners' windows
    assert (want['n'] < min_n).any() and (want['n'] >= min_n).any() and want['n'].max() < nn
    res = mod.calc_diversity_map(grid=(4, 3), win=3, min_n=min_n)
    np.testing.assert_array_equal(res['n'], want['n'])
    np.testing.assert_array_equal(res['S'], want['S'])
    st = DM.window_stats(want['n'], want['S'], want['sum_het'], want['sum_cc'], L, min_n=min_n)
    for k in DM.FLOAT_KEYS:
        np.testing.assert_array_equal(res[k], st[k], err_msg=k)
        assert np.isnan(res[k][want['n'] < min_n]).all()
    assert np.isfinite(res['pi'][want['n'] >= min_n]).all()
    assert res['grid'] == (4, 3) and res['win'] == 3 and res['n_loci'] == L
    # one window over everybody is calc_diversity's single group
    whole = mod.calc_diversity_map(grid=(1, 1), win=1)
    d = mod.calc_diversity()
    assert whole['n'][0, 0] == nn == d['n'][0] and whole['S'][0, 0] == d['S'][0]
    for k in ('pi', 'Ho', 'He'):
        assert abs(whole[k][0, 0] - d[k][0]) <= 2 * L * 2.0 ** -53 * d[k][0], k
    # a subset of the loci and of the individuals, the default grid
    ids = np.array([*mod.comm[0]])
    sub = mod.calc_diversity_map(loci=np.arange(5, 40), individs=ids[::2], win=5)
    dim = mod.land.dim
    assert sub['grid'] == (min(dim[0], 64), min(dim[1], 64)) and sub['n_loci'] == 35
    labd = mod.group_by_grid(*sub['grid'])
    wsub = sums_numpy(gts[::2], labd[::2], sub['grid'][0], sub['grid'][1], 2, np.arange(5, 40))
    np.testing.assert_array_equal(sub['n'], wsub['n'])
    np.testing.assert_array_equal(sub['S'], wsub['S'])
    np.testing.assert_array_equal(
        sub['pi'], DM.window_stats(wsub['n'], wsub['S'], wsub['sum_het'], wsub['sum_cc'], 35)['pi'])
