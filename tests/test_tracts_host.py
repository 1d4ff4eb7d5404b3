"""Identity tracts, host side (geonomics_amd/sim/tracts.py and the Species methods over a numpy
device): the numpy restatement of gnx_tracts_self / gnx_tracts_pairs against an independent
locus-by-locus Python loop (tests/_tracts.py) and against hand-worked rows, the integer map, the
statistics, the argument checks.  No GPU."""
import types

import numpy as np
import pytest

import _tracts as T
from geonomics_amd.sim import tracts as TR
from geonomics_amd.structs.analyses import SpeciesAnalyses


@pytest.fixture(scope='module')
def data():
    """case A cut down to 21 mosaic individuals and the three planted ones (276 pairs), with
    every tract list by the per-locus loop, with and without breaks"""
    haps, pos, brk = T.case_a()
    haps = np.concatenate([haps[:21], haps[-3:]])
    lists = {}
    for tag, b in (('brk', brk), ('none', None)):
        own = [T.loop_tracts(h[0], h[1], b) for h in haps]
        lists[tag] = (b, own, T.all_pair_tracts(haps, b))
    return haps, pos, lists


def test_the_data_holds_every_category_the_tests_claim(data):
    haps, pos, lists = data
    brk, own, pairs = lists['brk']
    every = [t for o in own[:21] for t in o] + [t for four in pairs.values() for f in four
                                                 for t in f]
    count = np.array([e - s + 1 for s, e in every])
    s = np.array([t[0] for t in every])
    e = np.array([t[1] for t in every])
    length = pos[e] - pos[s]
    print('%d tracts: >= 40 loci %d, >= 63 %d, >= 64 %d, >= 200 %d, longest %d loci; crossing a '
          'word boundary %d, the block boundary %d, ending at L - 1 %d'
          % (count.size, (count >= 40).sum(), (count >= 63).sum(), (count >= 64).sum(),
             (count >= 200).sum(), count.max(), ((s >> 6) != (e >> 6)).sum(),
             ((s <= 2047) & (e >= 2048)).sum(), (e == T.L_A - 1).sum()))
    assert count.size > 100000
    for lo in (40, 63, 64, 200):
        assert (count >= lo).sum() > 0 and (count == lo - 1).sum() + (count < lo).sum() > 0
    assert ((s >> 6) != (e >> 6)).sum() > 100              # tracts across a word boundary
    assert ((e >> 6) - (s >> 6) >= 2).sum() > 10           # with a whole word inside
    assert ((s <= 2047) & (e >= 2048)).sum() > 0           # across the block boundary
    assert (e == T.L_A - 1).sum() > 0 and (s == 0).sum() > 0
    assert ((e & 63) == 63).sum() > 0 and ((s & 63) == 0).sum() > 0
    for b in T.BREAKS_A:                                   # tracts cut by every break
        assert (s == b).sum() > 0 and (e == b - 1).sum() > 0
    assert not ((s < 2560) & (e >= 2560)).any()
    # the length threshold of the last set cuts through the tracts that pass the count
    assert 0 < (length >= 150).sum() < count.size
    # without breaks there are tracts across where the breaks were
    _, own0, pairs0 = lists['none']
    assert any(s0 < 2560 <= e0 for four in pairs0.values() for f in four for s0, e0 in f)


def test_the_restatement_agrees_with_the_locus_by_locus_loop(data):
    haps, pos, lists = data
    n = haps.shape[0]
    edges = T.edges_a()
    for tag, (brk, own, pairs) in lists.items():
        for min_loci, min_len in T.threshold_sets(pos):
            label = (tag, min_loci, min_len)
            want = T.loop_self(own, pos, min_loci, min_len, edges, T.L_A)
            got = TR.brute_self(haps, pos, brk, min_loci, min_len, edges, cover=True)
            for k in ('per', 'hist', 'cover'):
                np.testing.assert_array_equal(got[k], want[k], err_msg=str(label + (k,)))
            want = T.loop_pairs(own, pairs, n, pos, min_loci, min_len, edges, T.L_A)
            got = TR.brute_pairs(haps, pos, brk, min_loci, min_len, edges, cover=True)
            for k in ('cnt', 'len', 'longest', 'hist', 'cover'):
                np.testing.assert_array_equal(got[k], want[k], err_msg=str(label + (k,)))
            assert got['cnt'].dtype == np.int32 and got['work'] == (2 * n * (n - 1) + n) * 63
            assert got['cover'].max() <= 2 * n * (n - 1)
            if min_loci <= 64:
                assert want['cnt'].sum() > 0, label
    # min_loci <= 0 means 1; no edges, no cover
    a = TR.brute_self(haps, pos, None, 0, 0)
    b = TR.brute_self(haps, pos, None, 1, 0)
    assert (a['per'] == b['per']).all() and a['hist'] is None and a['cover'] is None


def _row(D, pos=None, brk=None, min_loci=1, min_len=0, **kw):
    """brute_self of one haplotype pair with differences D"""
    D = np.asarray(D, np.uint8)
    haps = np.stack([np.zeros_like(D), D])[None]
    pos = np.arange(D.size) if pos is None else pos
    return TR.brute_self(haps, pos, brk, min_loci, min_len, **kw)


def test_hand_worked_rows():
    # two identical haplotypes with two breaks give three tracts
    brk = np.zeros(100, bool)
    brk[[30, 64]] = True                       # mid-word, and at a word boundary
    r = _row(np.zeros(100), brk=brk, cover=True, edges=[0, 30, 35, 100])
    assert r['per'].tolist() == [[3, 100, 29 + 33 + 35, 35]]
    assert r['hist'].tolist() == [[1, 29], [1, 33], [1, 35]]
    assert (r['cover'] == 1).all()
    # ... and one tract 0..L-1 without them; bit 0 of brk is ignored
    brk0 = np.zeros(100, bool)
    brk0[0] = True
    assert _row(np.zeros(100), brk=brk0)['per'].tolist() == [[1, 100, 99, 99]]
    # complementary haplotypes give none
    r = _row(np.ones(100), cover=True)
    assert r['per'].tolist() == [[0, 0, 0, 0]] and not r['cover'].any()
    # a tract ending at bit 63 and one starting at bit 64 (a difference before and after)
    D = np.ones(200, np.uint8)
    D[50:64] = 0
    assert _row(D)['per'].tolist() == [[1, 14, 13, 13]]
    D = np.ones(200, np.uint8)
    D[64:80] = 0
    r = _row(D, cover=True)
    assert r['per'].tolist() == [[1, 16, 15, 15]]
    assert r['cover'][64:80].all() and not r['cover'][:64].any() and not r['cover'][80:].any()
    # both at once are one tract, unless a break stands at 64
    D[50:64] = 0
    assert _row(D)['per'].tolist() == [[1, 30, 29, 29]]
    brk = np.zeros(200, bool)
    brk[64] = True
    assert _row(D, brk=brk)['per'].tolist() == [[2, 30, 13 + 15, 15]]
    # a tract of exactly min_loci loci and one of min_loci - 1
    D = np.ones(300, np.uint8)
    D[10:50] = 0                               # 40 loci
    D[100:139] = 0                             # 39 loci
    assert _row(D, min_loci=40)['per'].tolist() == [[1, 40, 39, 39]]
    assert _row(D, min_loci=39)['per'].tolist() == [[2, 79, 39 + 38, 39]]
    assert _row(D, min_loci=41)['per'].tolist() == [[0, 0, 0, 0]]
    # a tract of exactly min_len and one a unit less
    pos = np.cumsum(np.r_[0, np.full(299, 3)])
    pos[120:] -= 1                             # the second tract is one unit shorter
    D = np.ones(300, np.uint8)
    D[10:50] = 0                               # length 39 * 3 = 117
    D[100:140] = 0                             # 40 loci too, length 116
    assert _row(D, pos=pos, min_len=117)['per'].tolist() == [[1, 40, 117, 117]]
    assert _row(D, pos=pos, min_len=116)['per'].tolist() == [[2, 80, 233, 117]]
    assert _row(D, pos=pos, min_len=118)['per'].tolist() == [[0, 0, 0, 0]]
    # hist: edges[b] <= length < edges[b + 1]
    r = _row(D, pos=pos, edges=[0, 116, 117, 118])
    assert r['hist'].tolist() == [[0, 0], [1, 116], [1, 117]]
    assert _row(D, pos=pos, edges=[0, 117])['hist'].tolist() == [[1, 116]]
    # a tract reaching L - 1 with L not a multiple of 64
    D = np.ones(100, np.uint8)
    D[70:] = 0
    r = _row(D, cover=True)
    assert r['per'].tolist() == [[1, 30, 29, 29]] and r['cover'][99] == 1
    # a single locus
    assert _row([0])['per'].tolist() == [[1, 1, 0, 0]]
    assert _row([1])['per'].tolist() == [[0, 0, 0, 0]]


def test_the_planted_individuals_of_case_a():
    haps, pos, brk = T.case_a()
    ident, compl, t = haps[-3:]
    four = [(0, 999), (1000, 2559), (2560, 3332), (3333, 3999)]
    assert T.loop_tracts(ident[0], ident[1], brk) == four
    assert T.loop_tracts(ident[0], ident[1], None) == [(0, 3999)]
    assert T.loop_tracts(compl[0], compl[1], brk) == []
    assert T.loop_tracts(t[0], t[1], brk) == list(T.PLANTED)
    got = TR.brute_self(haps[-3:], pos, brk, 1, 0)['per']
    assert got[0].tolist() == [4, 4000, sum(pos[e] - pos[s] for s, e in four),
                               max(pos[e] - pos[s] for s, e in four)]
    assert got[1].tolist() == [0, 0, 0, 0] and got[2, 0] == len(T.PLANTED)
    # T's tracts that pass each threshold set, counted by hand from PLANTED
    # (the 200 loci of 1100..1299 are 199 increments of at least 1: random, but far above 400)
    want = {(1, 0): 12, (40, 0): 11, (63, 0): 7, (64, 0): 6, (200, 400): 2,
            (1, 150): sum(pos[e] - pos[s] >= 150 for s, e in T.PLANTED)}
    assert pos[1299] - pos[1100] >= 400 and 3 <= want[(1, 150)] <= 9
    sets = T.threshold_sets(pos)
    assert sets[4] == (200, 400) and pos[2200] - pos[2000] == 399
    for ml, mlen in sets:
        assert TR.brute_self(haps[-1:], pos, brk, ml, mlen)['per'][0, 0] == want[(ml, mlen)]


def test_tract_map():
    rates = np.r_[0.0, np.full(9, 0.01), 0.5, np.full(5, 0.02), 0.7, 0.0, 0.0]
    pos, brk, glen = TR.tract_map(rates, 'morgans')
    m = TR._ld.map_positions(rates)
    assert pos.dtype == np.int64 and (pos == np.rint(m * 2 ** 32)).all()
    assert (np.abs(pos / 2 ** 32 - m) <= 2.0 ** -33).all() and (np.diff(pos) >= 0).all()
    assert np.flatnonzero(brk).tolist() == [10, 16] and pos[17] == pos[18] == pos[16]
    assert glen == (pos[9] - pos[0]) + (pos[15] - pos[10]) + (pos[18] - pos[16])
    assert pos[10] - pos[9] == 40 * 2 ** 32
    pl, bl, gl = TR.tract_map(rates, 'loci')
    assert (pl == np.arange(19)).all() and (bl == brk).all() and gl == 9 + 5 + 2
    # free recombination: every locus is a break
    pf, bf, gf = TR.tract_map(np.r_[0.0, np.full(7, 0.5)], 'morgans')
    assert bf[1:].all() and not bf[0] and gf == 0
    # a rate at locus 0 never makes a break
    assert not TR.tract_map(np.full(4, 0.5), 'loci')[1][0]
    with pytest.raises(ValueError, match='unit'):
        TR.tract_map(rates, 'c')
    assert TR.to_units(0.01, 'morgans') == 42949673 and TR.to_units(0.5, 'morgans') == 2 ** 31
    assert TR.to_units(50, 'loci') == 50 and TR.to_units(2.5, 'loci') == 3
    assert TR.to_units(np.inf, 'loci') == 2 ** 63 - 1
    for bad in (np.nan, 1e300):
        with pytest.raises(ValueError):
            TR.to_units(bad, 'morgans')
    assert TR.from_units([2 ** 31, 0], 'morgans').tolist() == [0.5, 0.0]
    w = TR.pack_breaks(brk, 16)
    assert w.dtype == np.uint64 and w[0] == (1 << 10) | (1 << 16) and not w[1:].any()
    b = np.zeros(130, bool)
    b[[64, 129]] = True
    assert TR.pack_breaks(b, 16)[:3].tolist() == [0, 1, 2]
    for bad in ([1], [3, 3], [5, 2]):
        with pytest.raises(ValueError, match='tract edges'):
            TR.check_tract_edges(bad)


def test_roh_and_sharing_statistics_on_made_up_sums():
    f, mean = TR.roh_stats([10, 0, 50], [2 ** 31, 0, 2 ** 32], 2 ** 33, 100, 'morgans')
    assert f.tolist() == [0.25, 0.0, 0.5] and mean == 0.25
    f, mean = TR.roh_stats([10, 0, 50], [2 ** 31, 0, 2 ** 32], 2 ** 33, 100, 'loci')
    assert f.tolist() == [0.1, 0.0, 0.5] and mean == pytest.approx(0.2)
    assert np.isnan(TR.roh_stats([1], [0], 0, 5, 'morgans')[0]).all()
    # four individuals on a line at 0, 1, 3, 7: distances 1, 3, 7, 2, 6, 4
    x, y = np.array([0, 1, 3, 7], np.float32), np.zeros(4, np.float32)
    cnt = np.array([[9, 2, 0, 1], [2, 9, 4, 0], [0, 4, 9, 0], [1, 0, 0, 9]])
    ln = cnt * 10
    s = TR.sharing_stats(x, y, cnt, ln, [1.0, 3.0, 7.0])
    assert s['pairs'].tolist() == [2, 3]                      # {1, 2} and {3, 6, 4}; 7 is outside
    assert s['mean_tracts'].tolist() == [(2 + 4) / 2, 0.0]
    assert s['mean_len'].tolist() == [30.0, 0.0]
    assert s['share_with_tract'].tolist() == [1.0, 0.0]
    assert s['mean_dist'].tolist() == [1.5, 13 / 3]
    e = TR.sharing_stats(x, y, cnt, ln, [10.0, 20.0])
    assert e['pairs'].tolist() == [0] and np.isnan(e['mean_tracts']).all()
    # distances are fp64 from the fp32 coordinates
    x2 = np.array([0.1, 0.4], np.float32)
    r = float(x2[1]) - float(x2[0])
    assert TR.sharing_stats(x2, np.zeros(2), np.ones((2, 2)), np.ones((2, 2)),
                            [r, r + 1])['pairs'].tolist() == [1]


# ---------------------------------------------------------------------- the public calls
class _Dev:
    """the device's tract calls in numpy (brute_self / brute_pairs), haplotypes in slot order"""

    def __init__(self, haps):
        self.haps = haps
        self.L = haps.shape[2]
        self.W64 = (self.L + 1023) // 1024 * 16

    def _brk(self, brk):
        bits = np.unpackbits(np.asarray(brk, '<u8').view(np.uint8), bitorder='little')
        return bits[:self.L].astype(bool)

    def tracts_self(self, pos, brk=None, min_loci=1, min_len=0, edges=None, slots=None,
                    cover=False):
        h = self.haps if slots is None else self.haps[slots]
        return TR.brute_self(h, pos, self._brk(brk), min_loci, min_len, edges, cover)

    def tracts_pairs(self, pos, brk=None, min_loci=1, min_len=0, edges=None, slots=None,
                     cover=False, max_work=0):
        from geonomics_amd import _native as nat
        h = self.haps if slots is None else self.haps[slots]
        work = TR.pairs_work(h.shape[0], self.L)
        if work > max_work:
            raise nat.GnxError('gnx_tracts_pairs: %d word steps of work exceed max_work = %d'
                               % (work, max_work))
        return TR.brute_pairs(h, pos, self._brk(brk), min_loci, min_len, edges, cover)


class _Species(SpeciesAnalyses):
    """a Species stand-in: the real _calc_roh and _calc_ibs_sharing over the numpy device"""

    def __init__(self, haps, ids, rates, xy):
        self._dev = _Dev(haps)
        self.ids = np.asarray(ids)
        self.xy = xy
        self.gen_arch = types.SimpleNamespace(recombinations=types.SimpleNamespace(
            _positions=np.arange(haps.shape[2]), _rates=np.asarray(rates, dtype=float)))
        self._genomes_assigned = True
        self._land_ref = types.SimpleNamespace(dim=(40, 40))

    def _geno_sample(self, individs):
        order = np.argsort(self.ids)
        if individs is None:
            return self.ids[order], order
        ids = np.sort(np.asarray(individs))
        return ids, order[np.searchsorted(self.ids[order], ids)]

    def _field(self, f):
        from geonomics_amd import _native as nat
        return self.xy[:, 0 if f == nat.F_X else 1]


def _stand_in():
    rng = np.random.RandomState(3)
    n, L = 30, 500
    haps = T.mosaic(rng, n, L, mean_seg=120)
    haps[4, 1] = haps[4, 0]
    ids = rng.permutation(n) * 2 + 11
    rates = np.r_[0.0, np.full(L - 1, 0.001)]
    rates[250] = 0.5
    xy = rng.uniform(0, 40, (n, 2)).astype(np.float32)
    return _Species(haps, ids, rates, xy), haps, ids, rates, xy


def test_species_methods_over_a_numpy_device():
    spp, haps, ids, rates, xy = _stand_in()
    order = np.argsort(ids)
    pos, brk, glen = TR.tract_map(rates, 'morgans')
    res = spp._calc_roh(min_len=0.02, min_loci=10, edges=[0.0, 0.05, 0.1, np.inf], cover=True)
    ref = TR.brute_self(haps[order], pos, brk, 10, TR.to_units(0.02, 'morgans'),
                        [0, TR.to_units(0.05, 'morgans'), TR.to_units(0.1, 'morgans'),
                         2 ** 63 - 1], True)
    assert (res['ids'] == ids[order]).all() and res['unit'] == 'morgans'
    np.testing.assert_array_equal(res['n_roh'], ref['per'][:, 0])
    np.testing.assert_array_equal(res['roh_loci'], ref['per'][:, 1])
    np.testing.assert_array_equal(res['roh_len'], ref['per'][:, 2] / 2 ** 32)
    np.testing.assert_array_equal(res['longest'], ref['per'][:, 3] / 2 ** 32)
    np.testing.assert_array_equal(res['f_roh'], ref['per'][:, 2] / glen)
    assert res['mean_f_roh'] == res['f_roh'].mean() > 0 and res['genome_len'] == glen / 2 ** 32
    np.testing.assert_array_equal(res['hist']['tracts'], ref['hist'][:, 0])
    np.testing.assert_array_equal(res['cover'], ref['cover'])
    who = int(np.flatnonzero(ids[order] == ids[4])[0])         # the identical homologues
    assert res['n_roh'][who] == 2 and res['f_roh'][who] == 1.0
    lo = spp._calc_roh(min_len=20, min_loci=10, unit='loci', individs=ids[:7])
    ref = TR.brute_self(haps[:7][np.argsort(ids[:7])], np.arange(500), brk, 10, 20)
    np.testing.assert_array_equal(lo['roh_len'], ref['per'][:, 2].astype(float))
    np.testing.assert_array_equal(lo['f_roh'], ref['per'][:, 1] / 500)
    assert 'hist' not in lo and 'cover' not in lo and lo['genome_len'] == 498.0
    # ---- sharing
    sh = spp._calc_ibs_sharing(min_len=0.03, min_loci=10, n_classes=4, max_dist=30.0,
                               tract_edges=[0.0, 0.1, np.inf], cover=True)
    ml = TR.to_units(0.03, 'morgans')
    ref = TR.brute_pairs(haps[order], pos, brk, 10, ml,
                         [0, TR.to_units(0.1, 'morgans'), 2 ** 63 - 1], True)
    np.testing.assert_array_equal(sh['n_tracts'], ref['cnt'])
    np.testing.assert_array_equal(sh['shared_len'], ref['len'] / 2 ** 32)
    np.testing.assert_array_equal(sh['longest'], ref['longest'] / 2 ** 32)
    np.testing.assert_array_equal(sh['hist']['tracts'], ref['hist'][:, 0])
    np.testing.assert_array_equal(sh['cover'], ref['cover'])
    assert sh['work'] == ref['work'] and ref['cnt'].sum() > 0
    by = sh['by_dist']
    edges = np.exp(np.linspace(0.0, np.log(30.0), 5))
    edges[0], edges[-1] = 1.0, 30.0
    np.testing.assert_array_equal(by['edges'], edges)
    want = TR.sharing_stats(xy[order, 0], xy[order, 1], ref['cnt'], ref['len'], edges)
    np.testing.assert_array_equal(by['pairs'], want['pairs'])
    np.testing.assert_array_equal(by['mean_tracts'], want['mean_tracts'])
    np.testing.assert_array_equal(by['mean_len'], want['mean_len'] / 2 ** 32)
    assert by['pairs'].sum() > 100
    no = spp._calc_ibs_sharing(min_len=30, min_loci=10, unit='loci', individs=ids[:5])
    assert no['hist'] is None and no['cover'] is None and no['n_tracts'].shape == (5, 5)


def test_species_methods_refuse_what_they_cannot_do():
    spp = _stand_in()[0]
    for f in (spp._calc_roh, spp._calc_ibs_sharing):
        with pytest.raises(ValueError, match='unit'):
            f(unit='c')
        for bad in (-0.1, np.inf, np.nan, True):
            with pytest.raises(ValueError, match='min_len'):
                f(min_len=bad)
        for bad in (0, -3, 2.5, True):
            with pytest.raises(ValueError, match='min_loci'):
                f(min_loci=bad)
    for bad in ([0.1], [0.2, 0.1], [-1.0, 2.0], [0.0, np.nan]):
        with pytest.raises(ValueError, match='tract length edges'):
            spp._calc_roh(edges=bad)
        with pytest.raises(ValueError, match='tract length edges'):
            spp._calc_ibs_sharing(tract_edges=bad)
    with pytest.raises(ValueError, match='edges or max_dist'):
        spp._calc_ibs_sharing(edges=[1.0, 2.0], max_dist=5.0)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='max_work'):
            spp._calc_ibs_sharing(max_work=bad)
    with pytest.raises(ValueError, match='calc_ibs_sharing.*exceed max_work = 9.*n=.*max_work'):
        spp._calc_ibs_sharing(max_work=9)
    # more than 4096 individuals: the advice is n=
    real = spp._geno_sample
    spp._geno_sample = lambda individs: (np.arange(4097), np.arange(4097))
    with pytest.raises(ValueError, match='calc_ibs_sharing: 1..4096 individuals.*n='):
        spp._calc_ibs_sharing()
    spp._geno_sample = real
    spp._genomes_assigned = False
    for f in (spp._calc_roh, spp._calc_ibs_sharing):
        with pytest.raises(ValueError, match='burn the model in first'):
            f()
    spp.gen_arch = None
    for f in (spp._calc_roh, spp._calc_ibs_sharing):
        with pytest.raises(ValueError, match='no genomes'):
            f()


def test_signatures_the_tiled_refusal_the_statistic_and_the_binding():
    import inspect
    from geonomics_amd import _native
    from geonomics_amd.sim import stats as ST
    from geonomics_amd.sim.model import Model
    from geonomics_amd.structs.species import Species
    from geonomics_amd.structs.tiled import TiledSpecies
    assert list(inspect.signature(Model.calc_roh).parameters) == [
        'self', 'spp', 'min_len', 'min_loci', 'unit', 'individs', 'n', 'edges', 'cover']
    assert list(inspect.signature(Model.calc_ibs_sharing).parameters) == [
        'self', 'spp', 'min_len', 'min_loci', 'unit', 'individs', 'n', 'edges', 'n_classes',
        'max_dist', 'tract_edges', 'cover', 'max_work']
    d = {k: v.default for k, v in inspect.signature(Model.calc_roh).parameters.items()}
    assert (d['min_len'], d['min_loci'], d['unit']) == (0.01, 50, 'morgans')
    d = {k: v.default for k, v in inspect.signature(Model.calc_ibs_sharing).parameters.items()}
    assert (d['min_len'], d['min_loci'], d['n_classes']) == (0.02, 50, 10)
    assert 'free recombination' in Species._calc_roh.__doc__
    assert 'free recombination' in Species._calc_ibs_sharing.__doc__
    for f in (TiledSpecies._calc_roh, TiledSpecies._calc_ibs_sharing):
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            f(object())
    sc = ST._StatsCollector
    assert sc.calc_fn_dict['roh'] is ST._calc_roh and 'roh' in sc._needs_genome
    assert sc.file_suffix_dict['roh'] == sc.file_suffix_dict['Nt']
    spp = _stand_in()[0]
    assert ST._calc_roh(spp, min_len=0.02, min_loci=10) == \
        spp._calc_roh(min_len=0.02, min_loci=10)['mean_f_roh']
    for name in ('gnx_tracts_self', 'gnx_tracts_pairs', 'gnx_tracts_info'):
        assert name in _native.EXPORTS
    assert TR.POS_PER_MORGAN == 2 ** 32
