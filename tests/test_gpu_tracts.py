"""Model.calc_roh and Model.calc_ibs_sharing on the device (csrc/gnx_tracts.hip, sim/tracts.py):
gnx_tracts_self and gnx_tracts_pairs against the numpy restatement
geonomics_amd/sim/tracts.brute_self / brute_pairs (which tests/test_tracts_host.py checks against a
locus-by-locus loop), and the public calls against the restatement applied to the downloaded
genotypes.  Needs an MI355X.

Every output is an integer function of the qualifying tracts: every comparison is
assert_array_equal, and every call is repeated once and must be bit-equal."""
import numpy as np
import pytest

import _tracts as T
from test_gpu_parity import native
from geonomics_amd.sim import tracts as TR

pytestmark = pytest.mark.gpu

BIG = 1 << 50
SELF_KEYS = ('per', 'hist', 'cover')
PAIR_KEYS = ('cnt', 'len', 'longest', 'hist', 'cover')


def _upload(nat, haps, seed=20):
    """explicit haplotypes [n][2][L] on a handle (test_gpu_mmrr._handle uploads dosages, which
    cannot be phased)"""
    import gnx_oracle as O
    n, _, L = haps.shape
    dev = nat.Device(24, 24, 1, L=L, cap_inds=n + 64, cap_rows=n + 64, seed=seed)
    dev.upload_rasters(np.ones((1, 24, 24), np.float32))
    dev.set_species_params(nat.default_species_params())
    rng = np.random.RandomState(seed)
    dev.upload_population(rng.uniform(0, 24, n).astype(np.float32),
                          rng.uniform(0, 24, n).astype(np.float32), np.zeros(n), np.zeros(n),
                          np.arange(n))
    dev.upload_genomes(O.pack_genomes(np.transpose(haps, (0, 2, 1))))
    return dev


def _packed(dev, brk):
    return None if brk is None else TR.pack_breaks(brk, dev.W64)


def _self(dev, haps, pos, brk, min_loci, min_len, edges, slots=None, label=''):
    ref = TR.brute_self(haps if slots is None else haps[slots], pos, brk, min_loci, min_len,
                        edges, True)
    got = dev.tracts_self(pos, _packed(dev, brk), min_loci, min_len, edges, slots, True)
    for k in SELF_KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg='%s: %s' % (label, k))
    info = dev.tracts_info()
    assert info['launches'] == 2 and info['bytes_read'] == ref['per'].shape[0] * 2 * \
        ((haps.shape[2] + 63) // 64) * 8                 # uploaded genomes share no block
    again = dev.tracts_self(pos, _packed(dev, brk), min_loci, min_len, edges, slots, True)
    for k in SELF_KEYS:
        assert again[k].tobytes() == got[k].tobytes(), (label, k)
    return got, ref


def _pairs(dev, haps, pos, brk, min_loci, min_len, edges, slots=None, label=''):
    h = haps if slots is None else haps[slots]
    ref = TR.brute_pairs(h, pos, brk, min_loci, min_len, edges, True)
    got = dev.tracts_pairs(pos, _packed(dev, brk), min_loci, min_len, edges, slots, True, BIG)
    for k in PAIR_KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg='%s: %s' % (label, k))
    n = h.shape[0]
    assert got['cnt'].dtype == np.int32
    assert got['work'] == ref['work'] == (2 * n * (n - 1) + n) * ((haps.shape[2] + 63) // 64)
    for k in ('cnt', 'len', 'longest'):
        assert (got[k] == got[k].T).all(), (label, k)
    assert got['cover'].max() <= 2 * n * (n - 1)
    again = dev.tracts_pairs(pos, _packed(dev, brk), min_loci, min_len, edges, slots, True, BIG)
    for k in PAIR_KEYS:
        assert again[k].tobytes() == got[k].tobytes(), (label, k)
    return got, ref


# ------------------------------------------------------------------ case A
@pytest.fixture(scope='module')
def case_a():
    """67 mosaic individuals and the three planted ones, L = 4000: 62 full words and 32 bits in
    rows of 64 words, two blocks per homologue"""
    nat = native()
    haps, pos, brk = T.case_a()
    dev = _upload(nat, haps)
    assert dev.blocks_per_hom == 2 and dev.W64 == 64
    yield nat, dev, haps, pos, brk
    dev.close()


SETS_A = [(ml, mlen, b) for ml, mlen in T.threshold_sets() for b in (True, False)
          if b or ml in (1, 63)]


@pytest.mark.parametrize('min_loci,min_len,with_brk', SETS_A)
def test_case_a_self_scan(case_a, min_loci, min_len, with_brk):
    nat, dev, haps, pos, brk = case_a
    b = brk if with_brk else None
    label = 'case A self %r' % ((min_loci, min_len, with_brk),)
    got, ref = _self(dev, haps, pos, b, min_loci, min_len, T.edges_a(), label=label)
    assert ref['per'][:, 0].sum() > 0 and ref['hist'][:, 0].sum() == ref['per'][:, 0].sum()
    assert ref['cover'].max() >= 1
    # the planted individuals: identical homologues, complementary ones
    if min_loci <= 200:
        assert got['per'][-3, 0] == (4 if with_brk else 1) and got['per'][-2, 0] == 0
    slots = np.random.RandomState(4).permutation(haps.shape[0])[:33].astype(np.int64)
    _self(dev, haps, pos, b, min_loci, min_len, T.edges_a(), slots, label + ', 33 slots')
    # without edges and cover
    bare = dev.tracts_self(pos, _packed(dev, b), min_loci, min_len)
    assert bare['hist'] is None and bare['cover'] is None
    np.testing.assert_array_equal(bare['per'], ref['per'])
    assert dev.tracts_info()['launches'] == 1


@pytest.mark.parametrize('min_loci,min_len,with_brk', SETS_A)
def test_case_a_pair_scan(case_a, min_loci, min_len, with_brk):
    """70 individuals: two 64-tiles with a ragged edge"""
    nat, dev, haps, pos, brk = case_a
    b = brk if with_brk else None
    label = 'case A pairs %r' % ((min_loci, min_len, with_brk),)
    got, ref = _pairs(dev, haps, pos, b, min_loci, min_len, T.edges_a(), label=label)
    off = ~np.eye(haps.shape[0], dtype=bool)
    assert ref['cnt'][off].sum() > 0 and ref['cover'].max() > 1
    assert ref['hist'][:, 0].sum() * 2 == ref['cnt'][off].sum()
    # the diagonal is the self call
    own = dev.tracts_self(pos, _packed(dev, b), min_loci, min_len)['per']
    np.testing.assert_array_equal(np.diag(got['cnt']), own[:, 0])
    np.testing.assert_array_equal(np.diag(got['len']), own[:, 2])
    np.testing.assert_array_equal(np.diag(got['longest']), own[:, 3])


def test_case_a_pair_scan_of_five_slots_and_the_work(case_a):
    nat, dev, haps, pos, brk = case_a
    slots = np.array([69, 3, 68, 40, 67], np.int64)          # among them the planted three
    got, ref = _pairs(dev, haps, pos, brk, 40, 0, T.edges_a(), slots, 'case A, 5 slots')
    assert ref['cnt'].sum() > 0
    work = (2 * 5 * 4 + 5) * 63
    only = dev.tracts_pairs(pos, _packed(dev, brk), 40, 0, T.edges_a(), slots, True)
    assert only['work'] == work and only['cnt'] is None and only['cover'] is None
    assert dev.tracts_info()['launches'] == 0
    exact = dev.tracts_pairs(pos, _packed(dev, brk), 40, 0, T.edges_a(), slots, True, work)
    assert exact['len'].tobytes() == got['len'].tobytes()
    with pytest.raises(nat.GnxError, match='exceed max_work = %d' % (work - 1)):
        dev.tracts_pairs(pos, _packed(dev, brk), 40, 0, T.edges_a(), slots, True, work - 1)
    assert dev.tracts_info()['launches'] == 0
    # no histogram, no cover
    bare = dev.tracts_pairs(pos, _packed(dev, brk), 40, 0, None, slots, False, BIG)
    assert bare['hist'] is None and bare['cover'] is None
    np.testing.assert_array_equal(bare['cnt'], ref['cnt'])
    # min_loci <= 0 means 1
    one = dev.tracts_pairs(pos, None, 1, 0, None, slots, False, BIG)
    for ml in (0, -5):
        z = dev.tracts_pairs(pos, None, ml, 0, None, slots, False, BIG)
        assert z['cnt'].tobytes() == one['cnt'].tobytes()


# ------------------------------------------------------------------ case B
def test_case_b_the_metric_block_geometry():
    """L = 41000: 641 words in nine blocks of 80, the last of which reaches past the homologue;
    long mosaic segments, and one individual with identical homologues: one tract 0..L-1"""
    nat = native()
    rng = np.random.RandomState(11)
    n, L = 9, 41000
    haps = T.mosaic(rng, n, L, mean_seg=3000)
    haps[5, 1] = haps[5, 0]
    pos = np.cumsum(rng.randint(0, 4, L)).astype(np.int64)   # (ties among them)
    dev = _upload(nat, haps)
    try:
        assert dev.blocks_per_hom == 9
        edges = np.array([0, 100, 1000, 5000, T.INT64_MAX], np.int64)
        for ml, mlen in ((1, 0), (63, 0), (50, 300), (2000, 0)):
            label = 'case B %r' % ((ml, mlen),)
            got, ref = _self(dev, haps, pos, None, ml, mlen, edges, label=label)
            assert got['per'][5].tolist() == [1, L, pos[-1] - pos[0], pos[-1] - pos[0]]
            pg, pr = _pairs(dev, haps, pos, None, ml, mlen, edges, label=label)
            assert pr['cnt'].sum() > 0
        brk = np.zeros(L, bool)
        brk[[5120, 20000, 40960]] = True                     # a block boundary, mid-word, the last word
        _self(dev, haps, pos, brk, 63, 0, edges, label='case B, breaks')
        _pairs(dev, haps, pos, brk, 63, 0, edges, label='case B, breaks')
    finally:
        dev.close()


# ------------------------------------------------------------------ case C
@pytest.mark.parametrize('L', [1, 64])
def test_case_c_one_individual(L):
    nat = native()
    pos = np.arange(L, dtype=np.int64) * 5
    edges = np.array([0, 1, T.INT64_MAX], np.int64)
    for differ in (False, True):
        haps = np.zeros((1, 2, L), np.uint8)
        haps[0, :, ::3] = 1
        if differ:
            haps[0, 1, L - 1] ^= 1
        dev = _upload(nat, haps)
        try:
            got, _ = _self(dev, haps, pos, None, 1, 0, edges, label='case C')
            pg, _ = _pairs(dev, haps, pos, None, 1, 0, edges, label='case C')
            if differ:
                want = [0, 0, 0, 0] if L == 1 else [1, L - 1, 5 * (L - 2), 5 * (L - 2)]
            else:
                want = [1, L, 5 * (L - 1), 5 * (L - 1)]
            assert got['per'].tolist() == [want]
            assert pg['cnt'].tolist() == [[want[0]]] and pg['len'].tolist() == [[want[2]]]
            assert pg['work'] == 1 and not pg['cover'].any() and not pg['hist'].any()
        finally:
            dev.close()


# ------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch_and_leave_the_handle_as_it_was(case_a):
    nat, dev, haps, pos, brk = case_a
    edges = T.edges_a()
    before = dev.tracts_self(pos, None, 40, 0, edges, None, True)
    assert dev.tracts_info()['launches'] == 2

    def refused(match, f, *a, **kw):
        with pytest.raises(nat.GnxError, match=match):
            f(*a, **kw)
        assert dev.tracts_info()['launches'] == 0

    for f, tail in ((dev.tracts_self, ()), (dev.tracts_pairs, (False, BIG))):
        refused('slot 7 is listed twice', f, pos, None, 40, 0, edges, np.array([7, 3, 7]), *tail)
        refused('slot out of range', f, pos, None, 40, 0, edges, np.array([0, dev.N]), *tail)
        refused('slot out of range', f, pos, None, 40, 0, edges, np.array([-1, 3]), *tail)
        refused('individuals', f, pos, None, 40, 0, edges, np.zeros(0, np.int64), *tail)
        p = pos.copy()
        p[50] = p[49] - 1
        refused(r'non-decreasing \(pos\[50\]', f, p, None, 40, 0, edges, None, *tail)
        refused('min_len >= 0', f, pos, None, 40, -1, edges, None, *tail)
        for e in ([0, 5, 5], [3, 2], [0, 10, 9, 20]):
            refused('strictly ascending', f, pos, None, 40, 0, np.array(e), None, *tail)
        refused('2..65 edges', f, pos, None, 40, 0, np.array([1]), None, *tail)
        refused('2..65 edges', f, pos, None, 40, 0, np.arange(66), None, *tail)
    refused('1..4096 individuals', dev.tracts_pairs, pos, None, 40, 0, edges,
            np.zeros(4097, np.int64), False, BIG)
    refused('1..33554432 individuals', dev.tracts_self, pos, None, 40, 0, edges,
            np.zeros(2 ** 25 + 1, np.int64))
    with pytest.raises(ValueError, match='pos'):
        dev.tracts_self(pos[:-1])
    with pytest.raises(ValueError, match='brk'):
        dev.tracts_self(pos, np.zeros(3, np.uint64))
    full = dev.tracts_self(pos, None, 40, 0, np.arange(65))               # 64 bins are taken
    assert full['hist'].shape == (64, 2)
    after = dev.tracts_self(pos, None, 40, 0, edges, None, True)
    assert all(after[k].tobytes() == before[k].tobytes() for k in SELF_KEYS)
    empty = nat.Device(16, 16, 1, L=96, cap_inds=256, cap_rows=256, seed=1)
    empty.upload_rasters(np.ones((1, 16, 16), np.float32))
    empty.set_species_params(nat.default_species_params())
    empty.upload_population(np.ones(10), np.ones(10), np.zeros(10), np.zeros(10), np.arange(10))
    for f, tail in ((empty.tracts_self, ()), (empty.tracts_pairs, (False, BIG))):
        with pytest.raises(nat.GnxError, match='genomes not assigned'):
            f(np.arange(96), None, 1, 0, None, None, *tail)
    empty.close()
    tile = _upload(nat, haps[:10])
    rec = np.zeros(1, nat.IND_REC)
    rec['x'], rec['y'], rec['id'] = 1.0, 1.0, 10 ** 6
    tile.tile_import_ghosts(rec)
    for f, tail in ((tile.tracts_self, ()), (tile.tracts_pairs, (False, BIG))):
        with pytest.raises(nat.GnxError, match='ghost records'):
            f(pos, None, 1, 0, None, np.arange(10, dtype=np.int64), *tail)
    tile.close()


# ------------------------------------------------------------------ the public calls
def _tract_params(seed, T_=6, stats=None):
    from test_gpu_model_api import small_params
    p = small_params(seed=seed, L=4000, T=T_)
    ga = p['comm']['species']['spp_0']['gen_arch']
    ga['r_distr_alpha'] = 0.0005                    # sparse recombination: two crossovers a gamete
    if stats is not None:
        from geonomics_amd.sim.params import ParametersDict
        p['model']['stats'] = ParametersDict(stats)
    return p


def _haps_of(mod, ids=None):
    gts = mod.get_genotypes(biallelic=True) if ids is None else \
        mod.get_genotypes(individs=ids, biallelic=True)
    return np.transpose(gts, (0, 2, 1)).astype(np.uint8)


def test_model_calc_roh_and_calc_ibs_sharing_after_real_steps():
    """genomes that went through the deferred crossover, in blocks that parents and offspring
    share"""
    import geonomics_amd as gnx
    mod = gnx.make_model(_tract_params(8, T_=40))
    for f in (mod.calc_roh, mod.calc_ibs_sharing):
        with pytest.raises(ValueError, match='burn the model in first'):
            f()
    mod.walk(10000, 'burn', verbose=False)
    spp = mod.comm[0]
    rec = spp.gen_arch.recombinations
    rates = np.zeros(4000)
    rates[rec._positions] = rec._rates
    assert rates[0] == 0 and (rates[1:] == 0.0005).all()
    pos, brk, glen = TR.tract_map(rates, 'morgans')
    assert spp._dev.blocks_per_hom == 2 and not brk.any()
    skipped = []
    for steps in (5, 25):
        mod.walk(steps, 'main', verbose=False)
        ids = np.array([*spp])
        n = ids.size
        haps = _haps_of(mod)
        ml = TR.to_units(0.002, 'morgans')
        res = mod.calc_roh(min_len=0.002, min_loci=8, edges=[0.0, 0.005, 0.02, np.inf],
                           cover=True)
        info = spp._dev.tracts_info()
        ref = TR.brute_self(haps, pos, None, 8, ml,
                            [0, TR.to_units(0.005, 'morgans'), TR.to_units(0.02, 'morgans'),
                             T.INT64_MAX], True)
        assert (res['ids'] == ids).all() and ref['per'][:, 0].sum() > n
        np.testing.assert_array_equal(res['n_roh'], ref['per'][:, 0])
        np.testing.assert_array_equal(res['roh_loci'], ref['per'][:, 1])
        np.testing.assert_array_equal(res['roh_len'], ref['per'][:, 2] / 2 ** 32)
        np.testing.assert_array_equal(res['longest'], ref['per'][:, 3] / 2 ** 32)
        np.testing.assert_array_equal(res['f_roh'], ref['per'][:, 2] / glen)
        np.testing.assert_array_equal(res['hist']['tracts'], ref['hist'][:, 0])
        np.testing.assert_array_equal(res['cover'], ref['cover'])
        assert res['mean_f_roh'] == res['f_roh'].mean() and res['genome_len'] == glen / 2 ** 32
        full = n * 2 * 63 * 8
        print('after %d more steps: n = %d, %d runs, mean F_ROH %.4f, longest %.4f M; the scan '
              'read %d of %d bytes' % (steps, n, ref['per'][:, 0].sum(), res['mean_f_roh'],
                                       res['longest'].max(), info['bytes_read'], full))
        assert 0 < info['bytes_read'] <= full
        skipped.append(full - info['bytes_read'])
        # the defaults, and a sample
        dflt = mod.calc_roh()
        ref = TR.brute_self(haps, pos, None, 50, TR.to_units(0.01, 'morgans'))
        np.testing.assert_array_equal(dflt['n_roh'], ref['per'][:, 0])
        assert 'hist' not in dflt and 'cover' not in dflt and dflt['unit'] == 'morgans'
        sub = mod.calc_roh(min_len=6, min_loci=6, unit='loci', individs=ids[::7])
        ref = TR.brute_self(haps[::7], np.arange(4000), None, 6, 6)
        np.testing.assert_array_equal(sub['roh_loci'], ref['per'][:, 1])
        np.testing.assert_array_equal(sub['f_roh'], ref['per'][:, 1] / 4000)
        # ---- sharing: 64 sampled individuals
        sh = mod.calc_ibs_sharing(n=64, min_len=0.002, min_loci=8, max_dist=12.0, n_classes=5,
                                  tract_edges=[0.0, 0.01, np.inf], cover=True)
        assert sh['ids'].size == 64 and np.isin(sh['ids'], ids).all()
        hs = _haps_of(mod, sh['ids'])
        ref = TR.brute_pairs(hs, pos, None, 8, ml, [0, TR.to_units(0.01, 'morgans'),
                                                    T.INT64_MAX], True)
        off = ~np.eye(64, dtype=bool)
        assert ref['cnt'][off].sum() > 64
        np.testing.assert_array_equal(sh['n_tracts'], ref['cnt'])
        np.testing.assert_array_equal(sh['shared_len'], ref['len'] / 2 ** 32)
        np.testing.assert_array_equal(sh['longest'], ref['longest'] / 2 ** 32)
        np.testing.assert_array_equal(sh['hist']['tracts'], ref['hist'][:, 0])
        np.testing.assert_array_equal(sh['cover'], ref['cover'])
        assert sh['work'] == ref['work']
        rows = np.searchsorted(ids, sh['ids'])
        want = TR.sharing_stats(mod.get_x()[rows], mod.get_y()[rows], ref['cnt'], ref['len'],
                                sh['by_dist']['edges'])
        np.testing.assert_array_equal(sh['by_dist']['pairs'], want['pairs'])
        np.testing.assert_array_equal(sh['by_dist']['mean_tracts'], want['mean_tracts'])
        np.testing.assert_array_equal(sh['by_dist']['mean_len'], want['mean_len'] / 2 ** 32)
        assert sh['by_dist']['pairs'].sum() > 100
    # an inbred individual's homologues are one physical block in places (measured: 496 bytes,
    # the 31 words of one individual's second block, after the first 5 steps): the scan has
    # skipped them, and the results above are the restatement's all the same
    assert max(skipped) > 0 and all(v % 8 == 0 for v in skipped)
    with pytest.raises(ValueError, match='exceed max_work = 1.*n=.*max_work'):
        mod.calc_ibs_sharing(n=20, max_work=1)
    with pytest.raises(ValueError, match='unit'):
        mod.calc_roh(unit='cM')


def test_the_roh_statistic_writes_one_value_per_sampling_step(tmp_path, monkeypatch):
    import csv
    import geonomics_amd as gnx
    monkeypatch.chdir(tmp_path)
    mod = gnx.make_model(_tract_params(9, T_=7, stats={
        'Nt': {'calc': True, 'freq': 1},
        'roh': {'calc': True, 'freq': 3, 'min_len': 0.002, 'min_loci': 8}}))
    mod.run()
    base = tmp_path / 'GNX_mod-api_test' / 'it-0' / 'spp-spp_0'
    rows = list(csv.DictReader(open(base / 'mod-api_test_it-0_spp-spp_0_OTHER_STATS.csv')))
    assert [int(r['t']) for r in rows] == list(range(7))
    sampled = [int(r['t']) for r in rows if r['roh'] != '']
    assert sampled == [0, 3, 6]                                 # every third step and the last
    vals = [float(r['roh']) for r in rows if r['roh'] != '']
    assert all(0 < v < 1 for v in vals), vals
    last = mod.calc_roh(min_len=0.002, min_loci=8)['mean_f_roh']
    assert abs(vals[-1] - last) <= 1e-5                          # (the file keeps 5 decimals)
