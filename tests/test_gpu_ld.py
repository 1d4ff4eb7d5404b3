"""Model.calc_ld_decay and Model.calc_ne on the device (csrc/gnx_ld.hip, sim/ld.py,
Species._calc_ld_decay / _calc_ne): gnx_ld_bins against the numpy restatement
geonomics_amd/sim/ld.brute_bins (every pair brute-forced as include/gnx_hip.h specifies), against
the repository's own older path gnx_stats_ld where the two overlap, and the public calls against
the restatement applied to the downloaded genotypes.  Needs an MI355X.

Bounds.  c1, pairs, work and the kept loci are integers: equal.  Every fp64 output is a sum of
the m = pairs terms of its bin.  r2 comes from integers by the same three IEEE roundings on both
sides, r2 r2 by one more, d = pos[j] - pos[i] by one: the terms are bit-equal.  The oracle's sum
is the correctly rounded sum of its terms (math.fsum): at most 1 unit of 2^-53 sum |term|; the
device's sum in any order adds m units (the any-order bound test_gpu_sgs.py uses).  w goes
through expm1 on both sides, each within 1 ulp = 2 units of the true value: 4 more units per
term, as test_gpu_sgs.py grants its logarithm.

    |S - S_ref| <= (m + c) 2^-53 sum |term|,   c = 1, 1, 1, 5  for sum r2, r2^2, d, w.

A bin that holds a pair at distance 0 has sum w = +inf on both sides (not special-cased).  A call
repeated is bit-equal in every output; so is a call under another byte budget in its integers,
and within the bound in its sums (the order of the partials follows the blocks).
Measured on an MI355X, worst error / bound: 0.054 (case A), 0.035 (B), 0.016 (C, in one block and
in four), 0.003 (D); the Model methods agree with the restatement to 2.9e-16 relative."""
import numpy as np
import pytest

import _ld as T
from test_gpu_mmrr import _handle
from test_gpu_parity import native
from geonomics_amd.sim import ld as LD

pytestmark = pytest.mark.gpu

BIG = 1 << 50


def _gts(D):
    """the genotypes _handle uploads for dosages D: homologue 0 = (D >= 1), 1 = (D == 2)"""
    return np.stack([D >= 1, D == 2], axis=2).astype(np.uint8)


def _check(dev, D, loci, pos, edges, min_minor, morgans, slots=None, label=''):
    """one call against the restatement within the bounds of the module's docstring, and
    bit-equal when repeated -> (the call's dict, the restatement's)"""
    gts = _gts(D if slots is None else D[slots])
    bits = T.bits_of(gts)[:, loci]
    ref = LD.brute_bins(bits, pos, edges, min_minor, morgans)
    got = dev.ld_bins(loci, pos, edges, slots, min_minor, morgans, BIG)
    np.testing.assert_array_equal(got['c1'], ref['c1'], err_msg=label)
    np.testing.assert_array_equal(got['pairs'], ref['pairs'], err_msg=label)
    worst = 0.0
    for k, bound in T.sum_bounds(ref).items():
        inf = np.isinf(ref[k])
        assert (got[k][inf] == np.inf).all(), (label, k)
        err = np.abs(got[k][~inf] - ref[k][~inf])
        assert (err <= bound[~inf]).all(), (label, k, err, bound)
        if err.size:
            worst = max(worst, float((err / np.maximum(bound[~inf], 1e-300)).max()))
    n_chrom = bits.shape[0]
    nq = (n_chrom + 63) // 64
    nt = (len(loci) + 63) // 64
    print('%s: %d chromosomes (%d words), %d loci (%d kept), pairs %s, work %d, %s: worst error '
          '/ bound %.3g' % (label, n_chrom, nq, len(loci), ref['kept'].sum(),
                            ref['pairs'].tolist(), got['work'], dev.ld_info(), worst))
    assert got['work'] % nq == 0 and got['work'] <= nt * (nt + 1) // 2 * nq, label
    assert dev.ld_bins(loci, pos, edges, slots, min_minor, morgans)['work'] == got['work']
    again = dev.ld_bins(loci, pos, edges, slots, min_minor, morgans, BIG)
    for k in ('c1', 'pairs') + T.SUMS:
        assert again[k].tobytes() == got[k].tobytes(), (label, k)
    assert again['work'] == got['work']
    return got, ref


def _case_a():
    """131 individuals (262 chromosomes: four full words and 6 bits), L = 130 (two full tiles
    and 2 loci); the rate vector holds two zeros (tied positions) and one 0.5 (a break); loci 5
    and 129 are monomorphic, locus 70 is a singleton (left out by min_minor = 2)"""
    rng = np.random.RandomState(16)
    n, L = 131, 130
    D = rng.binomial(2, rng.uniform(0.1, 0.9, L), size=(n, L))
    D[:, 5], D[:, 129] = 0, 2
    D[:, 70] = 0
    D[17, 70] = 1
    rates = rng.uniform(0.001, 0.05, L)
    rates[0] = rates[40] = rates[41] = 0.0
    rates[90] = 0.5
    return D, rates


EDGES_A = np.array([0.0, 0.01, 0.05, 0.2, 1.0, np.inf])


@pytest.fixture(scope='module')
def case_a():
    nat = native()
    D, rates = _case_a()
    n = D.shape[0]
    rng = np.random.RandomState(1)
    dev = _handle(nat, D, rng.uniform(0, 24, n), rng.uniform(0, 20, n), np.arange(n),
                  np.ones((1, 20, 24)))
    yield nat, dev, D, LD.map_positions(rates)
    dev.close()


def test_case_a_ties_a_break_monomorphic_loci_and_a_singleton(case_a):
    nat, dev, D, pos = case_a
    loci = np.arange(130)
    got, ref = _check(dev, D, loci, pos, EDGES_A, 2, True, label='case A')
    assert pos[39] == pos[40] == pos[41] and pos[90] - pos[89] > 39.0
    assert ref['kept'].sum() == 127 and not ref['kept'][[5, 70, 129]].any()
    assert got['sum_w'][0] == np.inf and np.isfinite(got['sum_w'][1:]).all()   # the ties: d = 0
    assert (ref['pairs'] > 0).all() and ref['pairs'].sum() == 127 * 126 // 2
    assert got['work'] == 6 * 5 and dev.ld_info()['locus_blocks'] == 1
    # min_minor = 1 takes the singleton in; 0 and negative values mean 1
    one, ref1 = _check(dev, D, loci, pos, EDGES_A, 1, True, label='case A, min_minor 1')
    assert ref1['kept'].sum() == 128
    for mm in (0, -3):
        z = dev.ld_bins(loci, pos, EDGES_A, None, mm, True, BIG)
        assert all(z[k].tobytes() == one[k].tobytes() for k in ('pairs',) + T.SUMS)
    # without the map flag the weight is not taken
    _, refn = _check(dev, D, loci, pos, EDGES_A, 2, False, label='case A, no weight')
    assert not refn['sum_w'].any()


def test_case_b_loci_in_any_order_and_a_subset_of_the_individuals(case_a):
    nat, dev, D, pos = case_a
    rng = np.random.RandomState(3)
    # 70 loci in no order, among them both sides of a word boundary and the last valid bit
    rest = rng.permutation([l for l in range(130) if l not in (63, 64, 129)])[:67]
    loci = rng.permutation(np.r_[64, 63, 129, rest])
    assert (np.diff(loci) < 0).sum() > 20 and np.unique(loci).size == 70
    slots = rng.choice(131, 77, replace=False).astype(np.int64)
    # the request's own coordinates, ascending along the request
    p = np.sort(pos[rng.choice(130, 70, replace=False)])
    _check(dev, D, loci, p, EDGES_A, 2, True, slots, label='case B')
    _check(dev, D, loci[:1], p[:1], EDGES_A, 1, True, slots[:1], label='one locus, one individual')
    _check(dev, D, loci[:2], p[:2], np.array([0.0, np.inf]), 1, True, slots[:9], label='two loci')


def test_case_c_several_lds_stages_and_locus_blocks():
    """1100 individuals: 2200 chromosomes = 34 words and 24 bits, two full LDS stages of 16
    words and a partial one (rows of 48 words); L = 200 (four tiles) with the budget of one
    tile per block"""
    nat = native()
    rng = np.random.RandomState(23)
    n, L = 1100, 200
    D = rng.binomial(2, rng.uniform(0.02, 0.98, L), size=(n, L))
    # neighbours in LD: most individuals copy the locus before
    for l in range(1, L, 3):
        same = rng.rand(n) < 0.7
        D[same, l] = D[same, l - 1]
    pos = LD.map_positions(np.r_[0.0, rng.uniform(0.0005, 0.01, L - 1)])
    edges = np.array([0.0, 0.005, 0.02, 0.08, 0.3, 3.0])
    dev = _handle(nat, D, rng.uniform(0, 30, n), rng.uniform(0, 30, n), np.arange(n),
                  np.ones((1, 30, 30)))
    try:
        loci = np.arange(L)
        whole, ref = _check(dev, D, loci, pos, edges, 40, True, label='case C, one block')
        assert dev.ld_info()['locus_blocks'] == 1 and (ref['pairs'] > 0).all()
        dev.ld_budget(2 * 64 * 48 * 8 + 100)              # two blocks of one tile each
        cut, _ = _check(dev, D, loci, pos, edges, 40, True, label='case C, four blocks')
        info = dev.ld_info()
        assert info['locus_blocks'] == 4 >= 3 and info['launches'] > 10
        assert cut['work'] == whole['work']
        dev.ld_budget(3 * 64 * 48 * 8)                    # still one tile: a pair must fit
        assert dev.ld_bins(loci, pos, edges, None, 40, True, BIG)['pairs'].tobytes() == \
            cut['pairs'].tobytes()
        dev.ld_budget(0)
        back = dev.ld_bins(loci, pos, edges, None, 40, True, BIG)
        assert all(back[k].tobytes() == whole[k].tobytes() for k in ('c1', 'pairs') + T.SUMS)
        with pytest.raises(nat.GnxError, match='bytes >= 0'):
            dev.ld_budget(-1)
    finally:
        dev.close()


def test_case_d_whole_separations_on_the_edges_and_a_band():
    """L = 300, pos = the locus number, edges [1, 2, 4, 8, 16, 65): every distance is whole, so
    pairs sit exactly on edges; the even loci are monomorphic, so no kept pair is 1 apart and the
    first bin is empty; pairs 65 or more apart are in no bin and most of their tiles not listed"""
    nat = native()
    rng = np.random.RandomState(29)
    n, L = 97, 300
    D = rng.binomial(2, rng.uniform(0.2, 0.8, L), size=(n, L))
    D[:, ::2] = 0
    pos = np.arange(L, dtype=np.float64)
    edges = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 65.0])
    dev = _handle(nat, D, rng.uniform(0, 20, n), rng.uniform(0, 20, n), np.arange(n),
                  np.ones((1, 20, 20)))
    try:
        got, ref = _check(dev, D, np.arange(L), pos, edges, 1, False, label='case D')
        assert ref['kept'].sum() == 150 and ref['pairs'][0] == 0 and (ref['pairs'][1:] > 0).all()
        # kept pairs exactly 2, 4, 8, 16 apart are in the bin that starts there, 64 in the last
        sep = np.arange(2, 65, 2)
        want = np.array([(150 - s // 2) for s in sep])
        for k in range(1, 5):
            s = (sep >= edges[k]) & (sep < edges[k + 1])
            assert ref['pairs'][k] == want[s].sum()
        nq, nt = (2 * n + 63) // 64, 5
        i, j = np.triu_indices(L, 1)
        binned = ref['kept'][i] & ref['kept'][j] & (j - i < 65)
        tiles = len(set(zip((i[binned] >> 6).tolist(), (j[binned] >> 6).tolist())))
        assert tiles * nq <= got['work'] < nt * (nt + 1) // 2 * nq
        assert got['work'] == 9 * nq               # the diagonal tiles and their right neighbours
        # a band that starts above 0 drops the tiles below it too
        far = dev.ld_bins(np.arange(L), pos, np.array([130.0, 140.0]), None, 1, False)
        assert far['work'] == (3 + 2) * nq       # j-tile = i-tile + 2 or + 3
        _check(dev, D, np.arange(L), pos, np.array([130.0, 140.0]), 1, False, label='far band')
    finally:
        dev.close()


def test_one_bin_over_every_pair_is_the_mean_of_the_older_matrix(case_a):
    nat, dev, D, pos = case_a
    loci = np.arange(130)
    got = dev.ld_bins(loci, np.arange(130.0), np.array([0.0, np.inf]), None, 1, False, BIG)
    old = dev.stats_ld(loci)
    i, j = np.triu_indices(130, 1)
    v = old[i, j]
    ok = np.isfinite(v)
    assert got['pairs'][0] == ok.sum() == 128 * 127 // 2
    mean = got['sum_r2'][0] / got['pairs'][0]
    print('one bin: mean r2 %.15g, the older path %.15g' % (mean, v[ok].mean()))
    assert abs(mean - v[ok].mean()) <= 1e-12 * v[ok].mean()


def test_refusals_come_before_any_launch_and_leave_the_handle_as_it_was(case_a):
    nat, dev, D, pos = case_a
    loci = np.arange(130)
    before = dev.ld_bins(loci, pos, EDGES_A, None, 2, True, BIG)

    def refused(match, *a, **kw):
        with pytest.raises(nat.GnxError, match=match):
            dev.ld_bins(*a, **kw)
        assert dev.ld_info()['launches'] == 0

    only = dev.ld_bins(loci, pos, EDGES_A, None, 2, True)         # max_work <= 0: the work only
    assert only['work'] == before['work'] > 0 and only['pairs'] is None
    assert dev.ld_info()['launches'] == 0
    exact = dev.ld_bins(loci, pos, EDGES_A, None, 2, True, before['work'])
    assert exact['sum_r2'].tobytes() == before['sum_r2'].tobytes()
    refused('exceed max_work = %d' % (before['work'] - 1), loci, pos, EDGES_A, None, 2, True,
            before['work'] - 1)
    refused('slot out of range', loci, pos, EDGES_A, np.array([0, dev.N]), 2, True, BIG)
    refused('slot out of range', loci, pos, EDGES_A, np.array([-1, 3]), 2, True, BIG)
    refused('slot 7 is listed twice', loci, pos, EDGES_A, np.array([7, 3, 7]), 2, True, BIG)
    refused('individuals', loci, pos, EDGES_A, np.zeros(0, np.int64), 2, True, BIG)
    refused('2\\^26 chromosomes', loci, pos, EDGES_A, np.zeros(2 ** 25 + 1, np.int64), 2, True,
            BIG)
    bad = loci.copy()
    bad[9] = 130
    refused('locus out of range', bad, pos, EDGES_A, None, 2, True, BIG)
    bad[9] = -1
    refused('locus out of range', bad, pos, EDGES_A, None, 2, True, BIG)
    bad[9] = 8
    refused('locus 8 is listed twice', bad, pos, EDGES_A, None, 2, True, BIG)
    refused('at least one locus', loci[:0], pos[:0], EDGES_A, None, 2, True, BIG)
    p = pos.copy()
    p[50] = p[49] - 1e-9
    refused(r'non-decreasing \(pos\[50\]', loci, p, EDGES_A, None, 2, True, BIG)
    for v in (np.nan, np.inf):
        p = pos.copy()
        p[-1] = v
        refused('pos must be finite', loci, p, EDGES_A, None, 2, True, BIG)
    for e in ([0.0, 2.0, 2.0], [1.0, 0.5], [0.0, np.nan, 3.0], [0.0, np.inf, np.inf],
              [-np.inf, 1.0]):
        refused('edges must be ascending', loci, pos, np.array(e), None, 2, True, BIG)
    refused('2..65 edges', loci, pos, np.array([1.0]), None, 2, True, BIG)
    refused('2..65 edges', loci, pos, np.arange(66.0), None, 2, True, BIG)
    with pytest.raises(ValueError, match='pos'):
        dev.ld_bins(loci, pos[:-1], EDGES_A, None, 2, True, BIG)
    full = dev.ld_bins(loci, pos, np.arange(65.0), None, 2, True, BIG)       # 64 bins are taken
    assert full['pairs'].shape == (64,)
    after = dev.ld_bins(loci, pos, EDGES_A, None, 2, True, BIG)
    assert all(after[k].tobytes() == before[k].tobytes() for k in ('c1', 'pairs') + T.SUMS)
    empty = nat.Device(16, 16, 1, L=96, cap_inds=256, cap_rows=256, seed=1)
    empty.upload_rasters(np.ones((1, 16, 16), np.float32))
    empty.set_species_params(nat.default_species_params())
    empty.upload_population(np.ones(10), np.ones(10), np.zeros(10), np.zeros(10), np.arange(10))
    with pytest.raises(nat.GnxError, match='genomes not assigned'):
        empty.ld_bins(np.arange(10), np.arange(10.0), EDGES_A, None, 1, False, BIG)
    assert empty.ld_info()['launches'] == 0
    empty.close()
    tile = _handle(nat, D[:10], np.ones(10), np.ones(10), np.arange(10), np.ones((1, 20, 24)))
    ten = np.arange(10, dtype=np.int64)
    tile.ld_bins(loci, pos, EDGES_A, ten, 1, True, BIG)
    assert tile.ld_info()['launches'] > 0                 # (so that the 0 below says something)
    rec = np.zeros(1, nat.IND_REC)
    rec['x'], rec['y'], rec['id'] = 1.0, 1.0, 10 ** 6
    tile.tile_import_ghosts(rec)
    with pytest.raises(nat.GnxError, match='ghost records'):
        tile.ld_bins(loci, pos, EDGES_A, np.arange(10, dtype=np.int64), 1, True, BIG)
    assert tile.ld_info()['launches'] == 0
    tile.close()


# ------------------------------------------------------------------ the public calls
def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert (np.isnan(a) == np.isnan(b)).all(), what
    ok = np.isfinite(b)
    assert (a[~ok & ~np.isnan(b)] == b[~ok & ~np.isnan(b)]).all(), what
    rel = np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300)
    assert (rel <= 1e-9).all(), (what, a, b)
    return float(rel.max()) if rel.size else 0.0


def _ld_params(seed, T_=25, stats=None):
    from test_gpu_model_api import small_params
    p = small_params(seed=seed, L=100, T=T_)
    ga = p['comm']['species']['spp_0']['gen_arch']
    ga['r_distr_alpha'] = 0.02                      # linked loci: adjacent c = 0.02
    if stats is not None:
        from geonomics_amd.sim.params import ParametersDict
        p['model']['stats'] = ParametersDict(stats)
    return p


def test_model_calc_ld_decay_and_calc_ne_after_real_steps():
    import geonomics_amd as gnx
    mod = gnx.make_model(_ld_params(8))
    for f in (mod.calc_ld_decay, mod.calc_ne):
        with pytest.raises(ValueError, match='burn the model in first'):
            f()
    mod.walk(10000, 'burn', verbose=False)
    with pytest.raises(ValueError, match="method: 'ld'"):
        mod.calc_ne(method='temporal')
    mod.walk(20, 'main', verbose=False)
    spp = mod.comm[0]
    gts = mod.get_genotypes(biallelic=True)
    n = gts.shape[0]
    bits = T.bits_of(gts)
    rec = spp.gen_arch.recombinations
    rates = np.zeros(100)
    rates[rec._positions] = rec._rates
    assert rates[0] == 0 and (rates[1:] == 0.02).all()
    pos = LD.map_positions(rates)
    mm = LD.min_minor(0.05, 2 * n)
    # ---- calc_ld_decay with its defaults: 20 bins of c, the last open above
    res = mod.calc_ld_decay()
    edges = LD.default_edges('c', 20)
    np.testing.assert_array_equal(res['edges'], edges)
    ref = LD.brute_bins(bits, pos, LD.c_to_morgans(edges), mm, True)
    want = LD.decay_stats(ref['pairs'], ref['sum_r2'], ref['sum_r4'], ref['sum_d'], ref['sum_w'],
                          True)
    np.testing.assert_array_equal(res['pairs'], ref['pairs'])
    np.testing.assert_array_equal(res['c1'], ref['c1'])
    assert res['n_chrom'] == 2 * n and res['n_loci_kept'] == ref['kept'].sum() > 20
    assert (res['ids'] == np.array([*spp])).all() and (res['loci'] == np.arange(100)).all()
    assert res['pairs'].sum() == ref['kept'].sum() * (ref['kept'].sum() - 1) // 2
    worst = max(_close(res[k], want[k], k)
                for k in ('mean_r2', 'sd_r2', 'mean_dist', 'mean_c', 'expected_w'))
    print('calc_ld_decay: n = %d, %d loci kept, pairs %s: worst relative error %.3g'
          % (n, res['n_loci_kept'], res['pairs'].tolist(), worst))
    # ---- in whole loci, a sample and a subset of the loci
    ids = np.array([*spp])[::3]
    sub = mod.calc_ld_decay(unit='loci', edges=[1, 2, 5, 20, 60], individs=ids,
                            loci=np.arange(10, 90), min_maf=0.1)
    rows = np.searchsorted(np.array([*spp]), ids)
    b2 = T.bits_of(gts[rows])[:, 10:90]
    ref2 = LD.brute_bins(b2, np.arange(10.0, 90.0), [1, 2, 5, 20, 60],
                         LD.min_minor(0.1, 2 * ids.size), False)
    np.testing.assert_array_equal(sub['pairs'], ref2['pairs'])
    _close(sub['mean_r2'], ref2['sum_r2'] / ref2['pairs'], 'mean_r2 (loci)')
    assert np.isnan(sub['mean_c']).all() and np.isnan(sub['expected_w']).all()
    with pytest.raises(ValueError, match='exceed max_work = 1.*n=.*loci=.*max_dist'):
        mod.calc_ld_decay(max_work=1)
    with pytest.raises(ValueError, match='unit'):
        mod.calc_ld_decay(unit='cM')
    # ---- calc_ne: one bin [m(min_c), inf)
    ne = mod.calc_ne()
    lo = float(LD.c_to_morgans(0.05))
    ref3 = LD.brute_bins(bits, pos, [lo, np.inf], mm, True)
    m = int(ref3['pairs'][0])
    assert ne['pairs'] == m > 0 and ne['n_chrom'] == 2 * n and ne['min_c'] == 0.05
    assert ne['n_loci_kept'] == ref3['kept'].sum()
    _close(ne['Ne'], LD.ld_ne(m, ref3['sum_r2'][0], ref3['sum_w'][0], 2 * n), 'Ne')
    _close(ne['mean_r2'], ref3['sum_r2'][0] / m, 'mean_r2')
    _close(ne['r2_drift'], ref3['sum_r2'][0] / m - 1.0 / (2 * n), 'r2_drift')
    print('calc_ne: Ne = %.1f from %d pairs of %d loci, N = %d' % (ne['Ne'], m,
                                                                   ne['n_loci_kept'], n))


def test_the_ne_statistic_writes_one_value_per_sampling_step(tmp_path, monkeypatch):
    import csv
    import geonomics_amd as gnx
    monkeypatch.chdir(tmp_path)
    mod = gnx.make_model(_ld_params(9, T_=7, stats={'Nt': {'calc': True, 'freq': 1},
                                                    'ne': {'calc': True, 'freq': 3,
                                                           'min_c': 0.1}}))
    mod.run()
    base = tmp_path / 'GNX_mod-api_test' / 'it-0' / 'spp-spp_0'
    rows = list(csv.DictReader(open(base / 'mod-api_test_it-0_spp-spp_0_OTHER_STATS.csv')))
    assert [int(r['t']) for r in rows] == list(range(7))
    sampled = [int(r['t']) for r in rows if r['ne'] != '']
    assert sampled == [0, 3, 6]                                 # every third step and the last
    vals = [float(r['ne']) for r in rows if r['ne'] != '']
    assert all(np.isfinite(v) and v > 0 for v in vals), vals
    last = mod.calc_ne(min_c=0.1)['Ne']
    assert abs(vals[-1] - last) <= 1e-5 * max(1.0, last)        # (the file keeps 5 decimals)
