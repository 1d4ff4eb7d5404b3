"""Haplotype sweep scans, host side (geonomics_amd/sim/sweeps.py and the Species methods over a
numpy device): the numpy restatement of gnx_sweeps_scan against an independent loop over explicit
pairs (tests/_sweeps.py), a hand-worked example, metamorphic properties of the definition, a
planted sweep, the statistics, the integer map, the argument checks.  No GPU."""
import types

import numpy as np
import pytest

import _sweeps as W
from geonomics_amd.sim import sweeps as SW
from geonomics_amd.structs.analyses import SpeciesAnalyses


def _same(got, ref, label=''):
    for k in W.KEYS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg='%s: %s' % (label, k))


# ------------------------------------------------------------------ against explicit pairs
@pytest.fixture(scope='module')
def host_case():
    rows, pos, brk = W.case_host()
    kw = dict(min_minor=4, cut_num=1, cut_den=20)
    return rows, pos, brk, kw, SW.brute_scan(rows, pos, brk, **kw)


def test_brute_scan_equals_the_loop_over_explicit_pairs(host_case):
    rows, pos, brk, kw, got = host_case
    ref = W.loop_scan(rows, pos, brk, **kw)
    _same(got, ref, 'every kept core')
    kept = got['kept']
    st = got['status'][kept]
    share0 = (st == 0).mean()
    print('%d of %d loci kept; %.0f %% of scans end at the cutoff; mean %.1f steps'
          % (kept.sum(), kept.size, 100 * share0, got['steps'][kept].mean()))
    assert kept.sum() >= 300 and (got['status'][~kept] == 5).all()
    assert share0 >= 0.5 and got['steps'][kept].mean() >= 20
    assert (st == 1).any()                       # the break and the two ends
    j = int(np.flatnonzero(kept)[200])
    one = SW.brute_scan(rows, pos, brk, cores=[j], curve=True, **kw)
    for d in (0, 1):
        for c in (0, 1):
            P = ref['curves'][(j, d, c)]
            np.testing.assert_array_equal(one['curve'][d, c, :len(P)], P)
            assert (one['curve'][d, c, len(P):] == -1).all()
    assert one['work'] == 4 * 2 * (kept.sum() - 1) and got['work'] == one['work'] * kept.sum()


@pytest.mark.parametrize('kw', [dict(max_gap=3), dict(max_extent=40), dict(max_gap=3, max_extent=25),
                                dict(cut_num=0), dict(cut_num=1, cut_den=1)])
def test_brute_scan_with_gap_and_extent_limits(host_case, kw):
    rows, pos, brk, base, full = host_case
    cores = list(range(5, 400, 9))
    args = dict(base, **kw)
    got = SW.brute_scan(rows, pos, brk, cores=cores, **args)
    _same(got, W.loop_scan(rows, pos, brk, cores=cores, **args), repr(kw))
    st = got['status'][cores]
    if 'max_gap' in kw:
        assert (st == 2).any()
    if 'max_extent' in kw:
        assert (st == 3).any() and (got['area'] <= full['area']).all()
    if kw.get('cut_num') == 0:
        assert (st[st < 5] == 1).all()


def test_brute_scan_with_a_class_row(host_case):
    rows, pos, brk, kw, _ = host_case
    rng = np.random.RandomState(5)
    cls = rng.choice(np.array([0, 1, 255], np.uint8), rows.shape[0], p=[0.4, 0.4, 0.2])
    cores = list(range(3, 400, 11))
    got = SW.brute_scan(rows, pos, brk, cls, cores, **kw)
    _same(got, W.loop_scan(rows, pos, brk, cls, cores, **kw), 'cls')
    assert (got['status'][cores] == 0).any()
    # the ignored chromosomes count for c1 and the kept loci, and for nothing else
    sub = rows[cls != 255]
    alone = SW.brute_scan(sub, pos, brk, cls[cls != 255], None, min_minor=2, cut_num=1, cut_den=20)
    both = np.flatnonzero(alone['kept'] & got['kept'])
    assert both.size > 300
    cls[rng.permutation(rows.shape[0])[:65]] = 1          # one chromosome left in class 0
    one = SW.brute_scan(rows, pos, brk, cls, cores, **kw)
    kept = one['kept'][cores]
    assert (one['status'][cores][kept][:, :, 0] == 4).all()
    assert (one['status'][cores][kept][:, :, 1] < 4).all()


# ------------------------------------------------------------------ by hand
def test_the_worked_example():
    R, pos = W.WORKED, W.WORKED_POS
    got = SW.brute_scan(R, pos, cores=[3], curve=True)           # cutoff 0: every scan to the edge
    assert got['c1'].tolist() == [3, 4, 5, 4, 1, 4, 4]
    assert got['kept'].tolist() == [True, True, True, True, False, True, True]
    # class 1 = chromosomes 0..3, class 0 = chromosomes 4..7: T = 6 each
    # right of the core (locus 4 is not kept): locus 5, then locus 6
    #   class 1: {0, 1}, {2, 3} -> 2 pairs; then all apart -> 0
    #   class 0: {4, 7}, {5, 6} -> 2;       then all apart -> 0
    # left: locus 2, 1, 0
    #   class 1: all equal -> 6; {0, 1}, {2, 3} -> 2; {0, 1}, {2}, {3} -> 1
    #   class 0: {4, 5, 6}, {7} -> 3; {4, 5}, {6}, {7} -> 1; all apart -> 0
    assert got['curve'][1, 1].tolist() == [6, 2, 0, -1, -1, -1, -1]
    assert got['curve'][1, 0].tolist() == [6, 2, 0, -1, -1, -1, -1]
    assert got['curve'][0, 1].tolist() == [6, 6, 2, 1, -1, -1, -1]
    assert got['curve'][0, 0].tolist() == [6, 3, 1, 0, -1, -1, -1]
    # areas: sum of (P_{s-1} + P_s) x gap, pos = 0 1 2 4 5 7 10
    assert got['area'][3].tolist() == [[(6 + 3) * 2 + (3 + 1) + (1 + 0), (6 + 6) * 2 + (6 + 2) + (2 + 1)],
                                       [(6 + 2) * 3 + (2 + 0) * 3, (6 + 2) * 3 + (2 + 0) * 3]]
    assert got['steps'][3].tolist() == [[3, 3], [2, 2]] and (got['status'][3] == 1).all()
    assert (got['status'][[0, 1, 2, 4, 5, 6]] == 5).all() and got['work'] == 4 * 1 * 5
    np.testing.assert_array_equal(SW.ihh(got['area'][3], 6), got['area'][3] / 12.0)
    # cutoff 1/4: 2 / 6 passes, 1 / 6 and 0 do not; the step that falls below is not integrated
    q = SW.brute_scan(R, pos, cores=[3], cut_num=1, cut_den=4, curve=True)
    assert q['area'][3].tolist() == [[18, 32], [24, 24]]
    assert q['steps'][3].tolist() == [[1, 2], [1, 1]] and (q['status'][3] == 0).all()
    assert q['curve'][0, 1].tolist() == [6, 6, 2, 1, -1, -1, -1]
    # cutoff 1/2: the right scans stop at their first step
    h = SW.brute_scan(R, pos, cores=[3], cut_num=1, cut_den=2)
    assert h['area'][3].tolist() == [[18, 24], [0, 0]] and h['steps'][3].tolist() == [[1, 1], [0, 0]]
    # a break on the locus that is not kept is inherited by the next kept one
    brk = np.zeros(7, np.uint8)
    brk[4] = 1
    b = SW.brute_scan(R, pos, brk, cores=[3])
    assert b['area'][3].tolist() == [[23, 35], [0, 0]] and (b['status'][3] == 1).all()
    _same(b, W.loop_scan(R, pos, brk, cores=[3]))
    # limits: the step to locus 5 is 3 long, the one from locus 2 to locus 3 is 2 long
    g = SW.brute_scan(R, pos, cores=[3], max_gap=2)
    assert g['status'][3].tolist() == [[1, 1], [2, 2]] and g['area'][3, 0].tolist() == [23, 35]
    e = SW.brute_scan(R, pos, cores=[3], max_extent=3)
    assert e['status'][3].tolist() == [[3, 3], [3, 3]] and e['steps'][3].tolist() == [[2, 2], [1, 1]]
    # two populations: the core's own column is not compared
    cls = np.array([0, 0, 0, 255, 1, 1, 1, 1], np.uint8)
    x = SW.brute_scan(R, pos, None, cls, [3], curve=True)
    assert x['curve'][1, 0].tolist() == [3, 1, 0, -1, -1, -1, -1]      # {0, 1}, {2}; all apart
    assert x['curve'][0, 1].tolist() == [6, 3, 1, 0, -1, -1, -1]       # loci 2, 1, 0 of 4..7
    with pytest.raises(ValueError, match='one core'):
        SW.brute_scan(R, pos, cores=[2, 3], curve=True)


# ------------------------------------------------------------------ metamorphic
def test_reversing_permuting_and_complementing(host_case):
    rows, pos, brk, kw, ref = host_case
    # reversed locus order: pos reflected, brk shifted by one; left and right swap
    rb = np.zeros_like(brk)
    rb[1:] = brk[:0:-1]
    rev = SW.brute_scan(rows[:, ::-1], pos[-1] - pos[::-1], rb, **kw)
    for k in ('area', 'steps', 'status'):
        np.testing.assert_array_equal(rev[k][::-1, ::-1], ref[k], err_msg='reversed: ' + k)
    np.testing.assert_array_equal(rev['c1'][::-1], ref['c1'])
    # a permuted sample
    perm = np.random.RandomState(8).permutation(rows.shape[0])
    _same(SW.brute_scan(rows[perm], pos, brk, **kw), ref, 'permuted')
    # every allele complemented: the classes swap
    comp = SW.brute_scan(1 - rows, pos, brk, **kw)
    for k in ('area', 'steps', 'status'):
        np.testing.assert_array_equal(comp[k][:, :, ::-1], ref[k], err_msg='complemented: ' + k)
    np.testing.assert_array_equal(comp['c1'], rows.shape[0] - ref['c1'])


# ------------------------------------------------------------------ a planted sweep
@pytest.mark.parametrize('seed', [100, 102, 105])
def test_a_planted_sweep_stands_out(seed):
    R, core = W.planted_sweep(seed)
    num, den = SW.cutoff_fraction(0.05)
    got = SW.brute_scan(R, np.arange(R.shape[1]), min_minor=6, cut_num=num, cut_den=den)
    unstd, h1, h0 = SW.ihs_unstandardized(got['area'], got['status'], got['c1'], R.shape[0])
    ok = np.isfinite(unstd)
    rank = int((unstd[ok] > unstd[core]).sum())
    print('seed %d: ihs_unstd at the core %.2f, rank %d among %d defined of %d kept cores'
          % (seed, unstd[core], rank, ok.sum(), got['kept'].sum()))
    assert got['c1'][core] == 48 and unstd[core] > 2 and rank <= 4
    assert ok.sum() >= 0.7 * got['kept'].sum()


# ------------------------------------------------------------------ the other host functions
def test_ihs_and_its_nan_rules():
    area = np.zeros((4, 2, 2), np.int64)
    area[:, :, 1], area[:, :, 0] = 30, 10
    status = np.zeros((4, 2, 2), np.uint8)
    status[1, 0, 1] = 1
    status[2, 1, 0] = 3
    status[3] = 5
    c1 = np.array([4, 4, 4, 4])
    u, h1, h0 = SW.ihs_unstandardized(area, status, c1, 8)
    assert u[0] == np.log((60 / 12.0) / (20 / 12.0)) and h1[0] == 5.0
    assert np.isnan(u[1]) and u[2] == u[0] and np.isnan(u[3])
    u2, _, _ = SW.ihs_unstandardized(area, status, c1, 8, keep_edge=True)
    assert u2[1] == u[0] and np.isnan(u2[3])
    area[0, :, 0] = 0
    assert np.isnan(SW.ihs_unstandardized(area, status, c1, 8)[0][0])   # an iHH of 0
    assert np.isnan(SW.ihh(5, 0))


def test_standardize_cutoff_and_map():
    x = np.array([1.0, 3.0, np.nan, 10.0, 20.0, 7.0])
    f = np.array([0.1, 0.2, 0.2, 0.6, 0.7, 1.0])
    z = SW.standardize_by_frequency(x, f, 2)
    np.testing.assert_array_equal(z[:2], [-1.0, 1.0])
    assert np.isnan(z[2])
    m, sd = np.mean([10.0, 20.0, 7.0]), np.std([10.0, 20.0, 7.0])
    np.testing.assert_array_equal(z[3:], (np.array([10.0, 20.0, 7.0]) - m) / sd)
    assert np.isnan(SW.standardize_by_frequency(x, f, 10)).all()             # one value a bin
    np.testing.assert_array_equal(SW.standardize(np.array([2.0, np.nan, 4.0])), [-1, np.nan, 1])
    assert np.isnan(SW.standardize(np.array([2.0, 2.0]))).all()
    assert SW.cutoff_fraction(0.05) == (52429, 2 ** 20) and SW.cutoff_fraction(0) == (0, 2 ** 20)
    assert SW.cutoff_fraction(1.0) == (2 ** 20, 2 ** 20)
    for bad in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='cutoff'):
            SW.cutoff_fraction(bad)
    rates = np.array([0.0, 0.01, 0.5, 0.01, 0.6])
    pos, brk, scale = SW.sweep_map(rates, 'morgans')
    assert scale == 2 ** 24 and brk.tolist() == [0, 0, 1, 0, 1] and brk.dtype == np.uint8
    step = -0.5 * np.log1p(-0.02)
    assert pos[1] == int(np.rint(step * 2 ** 24)) and pos[2] - pos[1] == 40 * 2 ** 24
    assert pos.dtype == np.int64 and (np.diff(pos) >= 0).all()
    pos, brk, scale = SW.sweep_map(rates, 'loci')
    assert pos.tolist() == [0, 1, 2, 3, 4] and scale == 1 and brk.tolist() == [0, 0, 1, 0, 1]
    pos, _, _ = SW.sweep_map(rates, 'sites', kept=[False, True, False, True, True])
    assert pos.tolist() == [0, 0, 0, 1, 2]
    with pytest.raises(ValueError, match='kept'):
        SW.sweep_map(rates, 'sites')
    with pytest.raises(ValueError, match='unit'):
        SW.sweep_map(rates, 'cM')


# ------------------------------------------------------------------ the Species methods
class _Dev:
    """the device's sweep call in numpy (brute_scan), haplotypes in slot order"""

    def __init__(self, haps):
        self.haps = haps
        self.L = haps.shape[2]
        self.W64 = (self.L + 1023) // 1024 * 16
        self.calls = []

    def sweeps_scan(self, loci, pos, brk=None, cls=None, cores=None, slots=None, min_minor=2,
                    cut_num=0, cut_den=1, max_gap=0, max_extent=0, max_work=0, curve=False):
        from geonomics_amd import _native as nat
        self.calls.append(dict(max_work=max_work, max_gap=max_gap, max_extent=max_extent))
        h = self.haps if slots is None else self.haps[slots]
        R = W.chromosomes(h)[:, loci]
        if max_work <= 0:
            c1 = R.sum(axis=0, dtype=np.int64)
            return dict(work=0, c1=c1, area=None, steps=None, status=None, curve=None)
        got = SW.brute_scan(R, pos, brk, cls, cores, min_minor, cut_num, cut_den, max_gap,
                            max_extent, curve)
        if got['work'] > max_work:
            raise nat.GnxError('gnx_sweeps_scan: %d word steps of work exceed max_work = %d'
                               % (got['work'], max_work))
        return got


class _Species(SpeciesAnalyses):
    """a Species stand-in: the real _calc_ihs, _calc_xpehh and _calc_ehh over the numpy device"""

    def __init__(self, haps, ids, rates):
        self._dev = _Dev(haps)
        self.ids = np.asarray(ids)
        self.gen_arch = types.SimpleNamespace(recombinations=types.SimpleNamespace(
            _positions=np.arange(haps.shape[2]), _rates=np.asarray(rates, dtype=float)))
        self._genomes_assigned = True

    def _geno_sample(self, individs):
        order = np.argsort(self.ids)
        if individs is None:
            return self.ids[order], order
        ids = np.sort(np.asarray(individs))
        return ids, order[np.searchsorted(self.ids[order], ids)]


def _stand_in():
    rng = np.random.RandomState(3)
    n, L = 40, 300
    haps = W.mosaic(rng, n, L, n_founders=6, mean_seg=50, mu=1 / 200)
    ids = rng.permutation(n) * 2 + 11
    rates = np.r_[0.0, np.full(L - 1, 0.001)]
    rates[170] = 0.5
    return _Species(haps, ids, rates), haps, ids, rates


def test_species_methods_over_a_numpy_device():
    spp, haps, ids, rates = _stand_in()
    order = np.argsort(ids)
    R = W.chromosomes(haps[order])
    pos, brk, scale = SW.sweep_map(rates, 'morgans')
    num, den = SW.cutoff_fraction(0.05)
    ref = SW.brute_scan(R, pos, brk, min_minor=4, cut_num=num, cut_den=den)
    res = spp._calc_ihs()
    assert (res['ids'] == ids[order]).all() and res['unit'] == 'morgans' and res['n_chrom'] == 80
    for k in ('area', 'steps', 'status', 'c1', 'kept'):
        if k in res:
            np.testing.assert_array_equal(res[k], ref[k])
    u, h1, h0 = SW.ihs_unstandardized(ref['area'], ref['status'], ref['c1'], 80)
    np.testing.assert_array_equal(res['ihs_unstd'], u)
    np.testing.assert_array_equal(res['ihh1'], h1 / 2 ** 24)
    np.testing.assert_array_equal(res['pos'], pos / 2.0 ** 24)
    np.testing.assert_array_equal(res['ihs'], SW.standardize_by_frequency(u, ref['c1'] / 80.0, 20))
    assert np.isfinite(u).sum() > 50 and (ref['status'][ref['kept']] == 1).any()
    # nSL: a probe for c1, then ranks among the kept loci; a subset of loci; the limits
    loci = np.arange(20, 280, 2)
    nsl = spp._calc_ihs(unit='sites', loci=loci, max_gap=1, max_extent=30, keep_edge=True)
    assert [c['max_work'] for c in spp._dev.calls[-2:]] == [0, spp._SWEEP_MAX_WORK]
    assert spp._dev.calls[-1]['max_gap'] == 1 and spp._dev.calls[-1]['max_extent'] == 30
    Rs = R[:, loci]
    kept = SW.kept_loci(Rs.sum(axis=0), 80, 4)
    sb = np.zeros(loci.size, np.uint8)
    sb[np.searchsorted(loci, 170)] = 1
    rs = SW.brute_scan(Rs, np.maximum(np.cumsum(kept) - 1, 0), sb, min_minor=4, cut_num=num,
                       cut_den=den, max_gap=1, max_extent=30)
    np.testing.assert_array_equal(nsl['status'], rs['status'])
    np.testing.assert_array_equal(
        nsl['ihs_unstd'], SW.ihs_unstandardized(rs['area'], rs['status'], rs['c1'], 80, True)[0])
    assert (nsl['loci'] == loci).all() and (rs['status'] == 3).any()
    # XP-EHH of two groups given by labels; a third group is refused
    lab = (np.arange(40) % 2).astype(np.int64)
    xp = spp._calc_xpehh(lab, unit='loci', min_maf=0.1)
    cls = np.repeat(lab, 2).astype(np.uint8)
    rx = SW.brute_scan(R, np.arange(300), brk, cls, None, min_minor=8, cut_num=num, cut_den=den)
    np.testing.assert_array_equal(xp['status'], rx['status'])
    ha, hb = SW.ihh_both(rx['area'], rx['status'], 780, 780)
    np.testing.assert_array_equal(xp['xpehh_unstd'], SW.log_ratio(ha, hb))
    np.testing.assert_array_equal(xp['xpehh'], SW.standardize(SW.log_ratio(ha, hb)))
    assert xp['names'] == [0, 1] and xp['n_a'] == xp['n_b'] == 20 and np.isfinite(ha).sum() > 50
    sub = spp._calc_xpehh({'a': ids[order][:10], 'b': ids[order][10:30]}, individs=ids[order][5:25])
    assert (sub['n_a'], sub['n_b'], sub['ids'].size) == (5, 15, 20)
    with pytest.raises(ValueError, match='exactly two groups'):
        spp._calc_xpehh(np.arange(40) % 3)
    with pytest.raises(ValueError, match='exactly two groups'):
        spp._calc_xpehh(np.zeros(40, np.int64))
    # EHH of one core
    core = int(np.flatnonzero(ref['kept'])[60])
    eh = spp._calc_ehh(core)
    one = SW.brute_scan(R, pos, brk, cores=[core], min_minor=4, cut_num=num, cut_den=den,
                        curve=True)
    np.testing.assert_array_equal(eh['status'], one['status'][core])
    assert eh['ehh1'][core] == 1.0 and eh['ehh0'][core] == 1.0 and eh['c1'] == ref['c1'][core]
    kidx = np.flatnonzero(ref['kept'])
    kc = int(np.searchsorted(kidx, core))
    T1 = SW.class_pairs(ref['c1'][core])
    ns = int((one['curve'][1, 1] >= 0).sum())
    np.testing.assert_array_equal(eh['ehh1'][kidx[kc:kc + ns]], one['curve'][1, 1, :ns] / float(T1))
    assert np.isnan(eh['ehh1'][~ref['kept']]).all() and np.isnan(eh['ehh1'][kidx[kc + ns:]]).all()
    assert np.nanmin(eh['ehh1']) < 0.05 <= np.nanmin(eh['ehh1'][kidx[kc:kc + ns - 1]])
    not_kept = int(np.flatnonzero(~ref['kept'])[0])
    with pytest.raises(ValueError, match='is not kept'):
        spp._calc_ehh(not_kept)
    with pytest.raises(ValueError, match='not among the loci'):
        spp._calc_ehh(5, loci=[6, 7, 8])
    # a max_work refusal becomes a ValueError with advice
    with pytest.raises(ValueError, match='exceed max_work = 10.*n=.*loci=.*max_work'):
        spp._calc_ihs(max_work=10)


def test_argument_checks_that_need_no_device():
    import inspect
    from geonomics_amd import _native
    from geonomics_amd.sim.model import Model
    from geonomics_amd.structs.species import Species
    from geonomics_amd.structs.tiled import TiledSpecies
    assert list(inspect.signature(Model.calc_ihs).parameters) == [
        'self', 'spp', 'unit', 'min_maf', 'cutoff', 'max_gap', 'max_extent', 'individs', 'n',
        'loci', 'n_freq_bins', 'keep_edge', 'max_work']
    d = {k: v.default for k, v in inspect.signature(Model.calc_ihs).parameters.items()}
    assert (d['unit'], d['min_maf'], d['cutoff'], d['n_freq_bins'], d['keep_edge']) == \
        ('morgans', 0.05, 0.05, 20, False)
    assert 'unit' not in inspect.signature(Model.calc_nsl).parameters
    assert list(inspect.signature(Model.calc_xpehh).parameters)[:3] == ['self', 'groups', 'spp']
    assert list(inspect.signature(Model.calc_ehh).parameters)[:4] == ['self', 'locus', 'spp', 'unit']
    assert 'its own cutoff' in Model.calc_xpehh.__doc__
    assert 'its own cutoff' in Species._calc_xpehh.__doc__
    for f in (TiledSpecies._calc_ihs, TiledSpecies._calc_xpehh, TiledSpecies._calc_ehh):
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            f(object())
    assert 'gnx_sweeps_scan' in _native.EXPORTS and 'gnx_sweeps_info' in _native.EXPORTS
    spp, haps, ids, rates = _stand_in()
    for f, a in ((spp._calc_ihs, ()), (spp._calc_xpehh, (np.arange(40) % 2,)),
                 (spp._calc_ehh, (100,))):
        with pytest.raises(ValueError, match="unit: 'morgans', 'loci' or 'sites'"):
            f(*a, unit='cM')
        with pytest.raises(ValueError, match='cutoff'):
            f(*a, cutoff=1.2)
        with pytest.raises(ValueError, match='max_gap'):
            f(*a, max_gap=0)
        with pytest.raises(ValueError, match='max_extent'):
            f(*a, max_extent=-1.0)
        with pytest.raises(ValueError, match='max_work'):
            f(*a, max_work=0)
        with pytest.raises(ValueError, match='min_maf'):
            f(*a, min_maf=0.7)
    with pytest.raises(ValueError, match='locus'):
        spp._calc_ehh(1.5)
    with pytest.raises(ValueError, match='n_freq_bins'):
        spp._calc_ihs(n_freq_bins=0)
    n_calls = len(spp._dev.calls)
    spp._genomes_assigned = False
    with pytest.raises(ValueError, match='burn the model in first'):
        spp._calc_ihs()
    spp.gen_arch = None
    with pytest.raises(ValueError, match='no genomes'):
        spp._calc_xpehh(np.arange(40) % 2)
    assert len(spp._dev.calls) == n_calls
    big = _Species(np.zeros((2049, 2, 8), np.uint8), np.arange(2049), np.zeros(8))
    with pytest.raises(ValueError, match=r'1\.\.2048 individuals'):
        big._calc_ihs()
