"""Model.calc_ihs, calc_nsl, calc_xpehh and calc_ehh on the device (csrc/gnx_sweeps.hip,
sim/sweeps.py): gnx_sweeps_scan against the numpy restatement geonomics_amd/sim/sweeps.brute_scan
(which tests/test_sweeps_host.py checks against a loop over explicit pairs), and the public calls
against the host formulas applied to the downloaded genotypes.  Needs an MI355X.

Every output is an integer function of the sample: every comparison is assert_array_equal, and
every call is repeated once and must be bit-equal."""
import numpy as np
import pytest

import _sweeps as W
from test_gpu_parity import native
from test_gpu_tracts import _upload
from geonomics_amd.sim import sweeps as SW

pytestmark = pytest.mark.gpu

BIG = W.BIG
OUT = ('c1', 'area', 'steps', 'status')
CUT = dict(min_minor=2, cut_num=1, cut_den=20)


def _haps(seed, n, L, **kw):
    kw = dict(dict(n_founders=6, mean_seg=40, mu=1 / 200), **kw)
    return W.mosaic(np.random.RandomState(seed), n, L, **kw)


def _scan(dev, haps, loci=None, pos=None, brk=None, cls=None, cores=None, slots=None,
          curve=False, label='', **kw):
    """one device call against brute_scan on the same haplotypes, and once more"""
    L = haps.shape[2]
    loci = np.arange(L) if loci is None else np.asarray(loci)
    pos = np.arange(loci.size, dtype=np.int64) if pos is None else pos
    R = W.chromosomes(haps if slots is None else haps[slots])[:, loci]
    ref = SW.brute_scan(R, pos, brk, cls, cores, curve=curve, **kw)
    got = dev.sweeps_scan(loci, pos, brk, cls, cores, slots, max_work=BIG, curve=curve, **kw)
    for k in OUT + (('curve',) if curve else ()):
        np.testing.assert_array_equal(got[k], ref[k], err_msg='%s: %s' % (label, k))
    assert got['work'] == ref['work'], label
    info = dev.sweeps_info()
    assert info['steps_total'] == ref['steps'].sum() and info['launches'] >= 2
    again = dev.sweeps_scan(loci, pos, brk, cls, cores, slots, max_work=BIG, curve=curve, **kw)
    for k in OUT + (('curve',) if curve else ()):
        assert again[k].tobytes() == got[k].tobytes(), (label, k)
    return got, ref


# ------------------------------------------------------------------ sample sizes
@pytest.mark.parametrize('n', [1, 2, 31, 32, 33, 64, 65, 100])
def test_sample_sizes_around_the_chunk_and_word_edges(n):
    """N = 2 n chromosomes: 62, 64, 66 around one list chunk and one bit-row word; 128, 130
    around two; n = 1 and 2 keep no locus or hardly any"""
    nat = native()
    haps = _haps(30 + n, n, 200)
    dev = _upload(nat, haps)
    try:
        pos = np.cumsum(np.random.RandomState(n).randint(0, 4, 200)).astype(np.int64)
        got, ref = _scan(dev, haps, pos=pos, label='n = %d' % n, **CUT)
        if n >= 31:
            kept = ref['kept']
            assert kept.sum() > 150 and (ref['status'][kept] == 0).mean() > 0.3
            assert ref['steps'][kept].mean() > 5
            # a subsample in another order: the classes cross the word edges differently
            slots = np.random.RandomState(n).permutation(n)[:max(2, n - 7)].astype(np.int64)
            _scan(dev, haps, pos=pos, slots=slots, cores=range(40, 200, 9),
                  label='n = %d, slots' % n, **CUT)
        else:
            assert ref['kept'].sum() == (0 if n == 1 else ref['kept'].sum())
            assert (got['status'][~ref['kept']] == 5).all()
    finally:
        dev.close()


def test_the_largest_sample_and_one_above_it():
    nat = native()
    haps = _haps(77, 2049, 48, n_founders=40, mean_seg=12, mu=1 / 50)
    dev = _upload(nat, haps)
    try:
        slots = np.arange(2048, dtype=np.int64)
        got, ref = _scan(dev, haps, slots=slots, cores=range(16, 32), label='n = 2048', **CUT)
        assert ref['kept'][16:32].all() and (ref['steps'][16:32] > 0).any()
        assert np.maximum(ref['c1'], 4096 - ref['c1'])[16:32].max() > 2048   # a list over 32 chunks
        with pytest.raises(nat.GnxError, match=r'1\.\.2048 individuals'):
            dev.sweeps_scan(np.arange(48), np.arange(48), max_work=BIG)
        assert dev.sweeps_info()['launches'] == 0
    finally:
        dev.close()


# ------------------------------------------------------------------ locus counts
@pytest.mark.parametrize('L', [1, 2, 63, 64, 65, 129, 1100])
def test_locus_counts_around_the_word_and_line_edges(L):
    nat = native()
    n = 24
    haps = _haps(200 + L, n, L, mean_seg=25, mu=1 / 100)
    dev = _upload(nat, haps)
    try:
        every = None if L <= 129 else range(3, L, 37)
        got, ref = _scan(dev, haps, cores=every, label='L = %d' % L, **CUT)
        if L >= 63:
            assert (ref['status'] == 0).any() and (ref['status'] == 1).any()
        # loci unordered and a strict subset; cores a subset
        rng = np.random.RandomState(L)
        sub = rng.permutation(L)[:max(1, (2 * L) // 3)]
        pos = np.cumsum(rng.randint(0, 3, sub.size)).astype(np.int64)
        cores = rng.permutation(sub.size)[:min(sub.size, 25)]
        _scan(dev, haps, loci=sub, pos=pos, cores=cores, label='L = %d, subset' % L, **CUT)
    finally:
        dev.close()


# ------------------------------------------------------------------ one handle for the rest
@pytest.fixture(scope='module')
def case():
    """50 mosaic individuals x 300 loci; individuals 40..49 carry one haplotype throughout"""
    nat = native()
    haps = _haps(9, 50, 300)
    haps[40:] = haps[40, 0]
    dev = _upload(nat, haps)
    rng = np.random.RandomState(12)
    pos = np.cumsum(rng.randint(0, 4, 300)).astype(np.int64)
    yield nat, dev, haps, pos
    dev.close()


def test_class_edge_cases(case):
    nat, dev, haps, pos = case
    cores = range(10, 300, 13)
    for m0 in (0, 1):
        cls = np.ones(100, np.uint8)
        cls[:m0] = 0
        cls[50:60] = 255
        got, ref = _scan(dev, haps, pos=pos, cls=cls, cores=cores, label='class of %d' % m0, **CUT)
        kept = ref['kept'][list(cores)]
        assert kept.any() and (got['status'][list(cores)][kept][:, :, 0] == 4).all()
        assert (got['status'][list(cores)][kept][:, :, 1] < 4).all()
        assert (got['area'][:, :, 0] == 0).all() and (got['steps'][:, :, 0] == 0).all()
    # all-identical chromosomes in a class never reach the cutoff: the exact full trapezoid
    cls = np.full(100, 255, np.uint8)
    cls[80:] = 1
    cls[:30] = 0
    got, ref = _scan(dev, haps, pos=pos, cls=cls, cores=cores, label='identical class', **CUT)
    kidx = np.flatnonzero(ref['kept'])
    T1 = 20 * 19 // 2
    for j in cores:
        if ref['kept'][j]:
            assert (got['status'][j, :, 1] == 1).all()
            assert got['area'][j, 0, 1] == 2 * T1 * (pos[j] - pos[kidx[0]])
            assert got['area'][j, 1, 1] == 2 * T1 * (pos[kidx[-1]] - pos[j])
    # cutoff 0: every scan runs to the edge; cutoff 1: status 0 at the first step that splits
    got, ref = _scan(dev, haps, pos=pos, cores=cores, min_minor=2, cut_num=0, cut_den=1,
                     label='cutoff 0')
    st = got['status'][list(cores)]
    assert (st[st < 5] == 1).all() and got['steps'].max() > 200
    got, ref = _scan(dev, haps, pos=pos, cores=cores, min_minor=2, cut_num=7, cut_den=7,
                     label='cutoff 1')
    assert (got['status'][list(cores)] == 0).any()
    _scan(dev, haps, pos=pos, cls=(np.arange(100) % 3 == 0).astype(np.uint8), min_minor=5,
          cut_num=1, cut_den=10, label='two populations, every core')


def test_breaks_limits_equal_positions_and_the_curve(case):
    nat, dev, haps, pos = case
    probe = dev.sweeps_scan(np.arange(300), pos, max_work=0, min_minor=8)
    assert probe['area'] is None and probe['status'] is None and probe['work'] > 0
    np.testing.assert_array_equal(probe['c1'], W.chromosomes(haps).sum(axis=0))
    kept = SW.kept_loci(probe['c1'], 100, 8)
    assert probe['work'] == SW.scan_work(kept.sum(), 100, kept.sum())
    assert dev.sweeps_info()['launches'] == 2 and dev.sweeps_info()['steps_total'] == 0
    off = np.flatnonzero(~kept)
    assert off.size > 3 and (np.diff(pos) == 0).sum() > 20       # equal pos at neighbouring loci
    brk = np.zeros(300, np.uint8)
    brk[[0, 100, 101, int(off[off > 150][0])]] = 1                # one on a locus that is not kept
    kw = dict(min_minor=8, cut_num=1, cut_den=20)
    full, _ = _scan(dev, haps, pos=pos, label='no limits', **kw)
    got, ref = _scan(dev, haps, pos=pos, brk=brk, label='breaks', **kw)
    assert (got['area'] != full['area']).any() and (got['area'] <= full['area']).all()
    for name, hit, miss, code in (('max_gap', 2, int(pos[-1]), 2),
                                   ('max_extent', 30, int(pos[-1]), 3)):
        got, ref = _scan(dev, haps, pos=pos, brk=brk, label=name, **dict(kw, **{name: hit}))
        assert (got['status'] == code).any()
        got, ref = _scan(dev, haps, pos=pos, label=name + ' not hit', **dict(kw, **{name: miss}))
        assert not (got['status'] == code).any()
        for k in OUT:
            np.testing.assert_array_equal(got[k], full[k])
    _scan(dev, haps, pos=pos, brk=brk, max_gap=2, max_extent=45, label='both', **kw)
    # the curve of one core
    core = int(np.flatnonzero(kept)[120])
    got, ref = _scan(dev, haps, pos=pos, brk=brk, cores=[core], curve=True, label='curve', **kw)
    assert got['curve'].shape == (2, 2, 300) and (got['curve'][:, :, 0] > 0).all()
    for d in (0, 1):
        for c in (0, 1):
            ns = got['steps'][core, d, c] + 1 + (got['status'][core, d, c] == 0)
            assert (got['curve'][d, c, :ns] >= 0).all() and (got['curve'][d, c, ns:] == -1).all()
    got, ref = _scan(dev, haps, pos=pos, cores=[int(off[0])], curve=True, label='curve, not kept',
                     **kw)
    assert (got['curve'] == -1).all() and (got['status'] == 5).all()
    with pytest.raises(nat.GnxError, match='n_cores == 1'):
        dev.sweeps_scan(np.arange(300), pos, cores=[core, core + 1], max_work=BIG, curve=True)
    with pytest.raises(nat.GnxError, match='n_cores == 1'):
        dev.sweeps_scan(np.arange(300), pos, max_work=BIG, curve=True)


def test_refusals_come_before_any_launch_and_leave_the_handle_as_it_was(case):
    nat, dev, haps, pos = case
    loci = np.arange(300)
    kw = dict(min_minor=4, cut_num=1, cut_den=20, max_work=BIG)
    before = dev.sweeps_scan(loci, pos, **kw)

    def refused(match, *a, **k):
        with pytest.raises(nat.GnxError, match=match):
            dev.sweeps_scan(*a, **dict(kw, **k))
        assert dev.sweeps_info() == dict(kernel_ms=0.0, launches=0, steps_total=0)
        after = dev.sweeps_scan(loci, pos, **kw)             # the next valid call still succeeds
        assert all(after[q].tobytes() == before[q].tobytes() for q in OUT)

    refused('slot 7 is listed twice', loci, pos, slots=np.array([7, 3, 7]))
    refused('slot out of range', loci, pos, slots=np.array([0, dev.N]))
    refused('slot out of range', loci, pos, slots=np.array([-1, 3]))
    refused(r'1\.\.2048 individuals', loci, pos, slots=np.zeros(0, np.int64))
    refused(r'1\.\.2048 individuals', loci, pos, slots=np.zeros(2049, np.int64))
    refused('at least one locus', np.zeros(0, np.int32), np.zeros(0, np.int64))
    refused('locus out of range', np.array([1, 300]), np.array([0, 1]))
    refused('locus out of range', np.array([-1, 30]), np.array([0, 1]))
    refused('locus 5 is listed twice', np.array([5, 9, 5]), np.array([0, 1, 2]))
    p = pos.copy()
    p[50] = p[49] - 1
    refused(r'non-decreasing \(pos\[50\]', loci, p)
    refused('core out of range', loci, pos, cores=[3, 300])
    refused('core out of range', loci, pos, cores=[-1])
    refused('core 8 is listed twice', loci, pos, cores=[8, 2, 8])
    refused('at least one core', loci, pos, cores=[])
    refused('cutoff', loci, pos, cut_num=-1)
    refused('cutoff', loci, pos, cut_den=0)
    refused('cutoff', loci, pos, cut_num=21)
    cls = np.zeros(100, np.uint8)
    cls[17] = 2
    refused(r'cls holds 0, 1 or 255 \(cls\[17\] = 2\)', loci, pos, cls=cls)
    # the overflow bound N (N - 1) (pos[last] - pos[0]) >= 2^62, N = 100: pos scaled until it trips
    span = -(-2 ** 62 // (100 * 99))                                  # the smallest refused span
    unit = np.r_[0, np.ones(299, np.int64)].cumsum()                  # 0 .. 299
    ok = unit * ((span - 1) // 299)
    assert 100 * 99 * int(ok[-1]) < 2 ** 62
    fine = dev.sweeps_scan(loci, ok, **kw)
    R = W.chromosomes(haps)
    ref = SW.brute_scan(R, ok, min_minor=4, cut_num=1, cut_den=20)
    for q in OUT:
        np.testing.assert_array_equal(fine[q], ref[q], err_msg='near the bound: ' + q)
    assert int(fine['area'].max()) > 2 ** 50
    over = ok.copy()
    over[-1] = span
    refused('>= 2\\^62', loci, over)
    # above max_work: refused after c1 and before the scan
    with pytest.raises(nat.GnxError, match='exceed max_work = 1000'):
        dev.sweeps_scan(loci, pos, **dict(kw, max_work=1000))
    assert dev.sweeps_info()['launches'] == 2
    with pytest.raises(ValueError, match='pos'):
        dev.sweeps_scan(loci, pos[:-1])
    with pytest.raises(ValueError, match='brk'):
        dev.sweeps_scan(loci, pos, np.zeros(3, np.uint8))
    with pytest.raises(ValueError, match='cls'):
        dev.sweeps_scan(loci, pos, cls=np.zeros(99, np.uint8))
    empty = nat.Device(16, 16, 1, L=96, cap_inds=256, cap_rows=256, seed=1)
    empty.upload_rasters(np.ones((1, 16, 16), np.float32))
    empty.set_species_params(nat.default_species_params())
    empty.upload_population(np.ones(10), np.ones(10), np.zeros(10), np.zeros(10), np.arange(10))
    with pytest.raises(nat.GnxError, match='genomes not assigned'):
        empty.sweeps_scan(np.arange(96), np.arange(96), max_work=BIG)
    empty.close()
    tile = _upload(nat, haps[:10])
    rec = np.zeros(1, nat.IND_REC)
    rec['x'], rec['y'], rec['id'] = 1.0, 1.0, 10 ** 6
    tile.tile_import_ghosts(rec)
    with pytest.raises(nat.GnxError, match='ghost records'):
        tile.sweeps_scan(loci, pos, slots=np.arange(10, dtype=np.int64), max_work=BIG)
    tile.close()


def test_the_ld_call_is_unchanged_around_a_sweep_scan(case):
    nat, dev, haps, pos = case
    loci = np.arange(300)
    edges = np.array([0.0, 5.0, 20.0, 100.0, np.inf])
    args = (loci, pos.astype(np.float64), edges, None, 3, False, BIG)
    before = dev.ld_bins(*args)
    dev.sweeps_scan(loci, pos, min_minor=3, cut_num=1, cut_den=20, max_work=BIG)
    after = dev.ld_bins(*args)
    for k in ('c1', 'pairs', 'sum_r2', 'sum_r4', 'sum_d', 'sum_w'):
        assert after[k].tobytes() == before[k].tobytes(), k
    assert before['pairs'].sum() > 10000 and after['work'] == before['work']


# ------------------------------------------------------------------ the public calls
def _sweep_params(seed, T_=40):
    from test_gpu_model_api import small_params
    p = small_params(seed=seed, L=1000, T=T_)
    ga = p['comm']['species']['spp_0']['gen_arch']
    ga['r_distr_alpha'] = 0.002
    return p


def _state(mod):
    return (np.array([*mod.comm[0]]).tobytes(), mod.get_genotypes(biallelic=True).tobytes(),
            mod.get_x().tobytes(), mod.get_y().tobytes())


def _close(a, b, label):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert (np.isnan(a) == np.isnan(b)).all(), label
    ok = ~np.isnan(a)
    np.testing.assert_allclose(a[ok], b[ok], rtol=1e-12, atol=0, err_msg=label)


def test_model_calls_after_real_steps_change_nothing():
    import geonomics_amd as gnx
    a, b = gnx.make_model(_sweep_params(8)), gnx.make_model(_sweep_params(8))
    for f in (a.calc_ihs, a.calc_nsl, lambda: a.calc_ehh(10), lambda: a.calc_xpehh([0, 1])):
        with pytest.raises(ValueError, match='burn the model in first'):
            f()
    for m in (a, b):
        m.walk(10000, 'burn', verbose=False)
        m.walk(6, 'main', verbose=False)
    spp = a.comm[0]
    ids = np.array([*spp])
    ids = np.sort(ids)[::max(1, ids.size // 120)][:120]
    gts = a.get_genotypes(individs=ids, biallelic=True)
    R = W.chromosomes(np.transpose(gts, (0, 2, 1)).astype(np.uint8))
    N = R.shape[0]
    rec = spp.gen_arch.recombinations
    rates = np.zeros(1000)
    rates[rec._positions] = rec._rates
    num, den = SW.cutoff_fraction(0.05)
    mm = max(2, int(np.ceil(0.05 * N - 1e-9)))
    # ---- iHS on the map
    pos, brk, scale = SW.sweep_map(rates, 'morgans')
    assert scale == 2 ** 24 and not brk.any()
    res = a.calc_ihs(individs=ids)
    info = spp._dev.sweeps_info()
    ref = SW.brute_scan(R, pos, brk, min_minor=mm, cut_num=num, cut_den=den)
    assert (res['ids'] == ids).all() and res['n_chrom'] == N
    for k in ('c1', 'status', 'steps', 'kept'):
        np.testing.assert_array_equal(res[k], ref[k], err_msg=k)
    assert info['steps_total'] == ref['steps'].sum() > ref['kept'].sum()
    u, h1, h0 = SW.ihs_unstandardized(ref['area'], ref['status'], ref['c1'], N)
    _close(res['ihh1'], h1 / scale, 'ihh1')
    _close(res['ihh0'], h0 / scale, 'ihh0')
    _close(res['ihs_unstd'], u, 'ihs_unstd')
    _close(res['ihs'], SW.standardize_by_frequency(u, ref['c1'] / float(N), 20), 'ihs')
    _close(res['freq'], ref['c1'] / float(N), 'freq')
    print('n = %d, %d of 1000 loci kept, %d defined scores, %d steps, %.3f ms in %d launches'
          % (ids.size, ref['kept'].sum(), np.isfinite(u).sum(), info['steps_total'],
             info['kernel_ms'], info['launches']))
    assert np.isfinite(u).sum() > 20
    # ---- nSL, with limits and the edge scans kept
    sub = np.arange(100, 900, 2)
    nsl = a.calc_nsl(individs=ids, loci=sub, max_gap=3, max_extent=200, keep_edge=True)
    kept_full = np.zeros(1000, bool)
    kept_full[sub] = ref['kept'][sub]
    spos, _, _ = SW.sweep_map(rates, 'sites', kept=kept_full)
    rs = SW.brute_scan(R[:, sub], spos[sub], None, min_minor=mm, cut_num=num, cut_den=den, max_gap=3,
                       max_extent=200)
    np.testing.assert_array_equal(nsl['status'], rs['status'])
    np.testing.assert_array_equal(nsl['steps'], rs['steps'])
    us = SW.ihs_unstandardized(rs['area'], rs['status'], rs['c1'], N, keep_edge=True)
    _close(nsl['ihs_unstd'], us[0], 'nsl')
    _close(nsl['ihh1'], us[1], 'nsl ihh1')
    assert nsl['unit'] == 'sites'
    # ---- XP-EHH between the two halves of the landscape
    lab = a.group_by_grid(2, 1)
    xp = a.calc_xpehh(lab, unit='loci', individs=ids, loci=sub)
    all_ids = np.sort(np.array([*spp]))
    grp = lab[np.searchsorted(all_ids, ids)]
    assert set(grp.tolist()) == {0, 1} and xp['n_a'] == (grp == 0).sum()
    rx = SW.brute_scan(R[:, sub], sub, None, np.repeat(grp, 2).astype(np.uint8),
                       min_minor=mm, cut_num=num, cut_den=den)
    np.testing.assert_array_equal(xp['status'], rx['status'])
    ha, hb = SW.ihh_both(rx['area'], rx['status'], SW.class_pairs(2 * xp['n_a']),
                         SW.class_pairs(2 * xp['n_b']))
    _close(xp['ihh_a'], ha, 'ihh_a')
    _close(xp['xpehh_unstd'], SW.log_ratio(ha, hb), 'xpehh_unstd')
    _close(xp['xpehh'], SW.standardize(SW.log_ratio(ha, hb)), 'xpehh')
    assert np.isfinite(xp['xpehh']).sum() > 20
    with pytest.raises(ValueError, match='exactly two groups'):
        a.calc_xpehh(a.group_by_grid(2, 2))
    # ---- EHH of one core
    core = int(np.flatnonzero(ref['kept'])[ref['kept'].sum() // 2])
    eh = a.calc_ehh(core, individs=ids)
    one = SW.brute_scan(R, pos, brk, cores=[core], min_minor=mm, cut_num=num, cut_den=den,
                        curve=True)
    T = (SW.class_pairs(N - ref['c1'][core]), SW.class_pairs(ref['c1'][core]))
    e0, e1 = SW.ehh_curve(one['curve'], ref['kept'], core, T, 1000)
    _close(eh['ehh0'], e0, 'ehh0')
    _close(eh['ehh1'], e1, 'ehh1')
    np.testing.assert_array_equal(eh['status'], one['status'][core])
    assert eh['ehh1'][core] == 1.0 and np.isfinite(eh['ehh1']).sum() >= 2
    with pytest.raises(ValueError, match='exceed max_work = 10.*n=.*loci=.*max_work'):
        a.calc_ihs(individs=ids, max_work=10)
    with pytest.raises(ValueError, match='unit'):
        a.calc_ihs(unit='cM')
    # ---- none of which consumed a draw of the device or changed a genome
    assert _state(a) == _state(b)
    for step in range(2):
        a.walk(1, 'main', verbose=False)
        b.walk(1, 'main', verbose=False)
        assert _state(a) == _state(b)
