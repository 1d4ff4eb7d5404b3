"""geonomics_amd/sim/ld.py on the host: the Haldane map of the architecture's recombination
rates, the numpy restatement of gnx_ld_bins (brute_bins) against the reference's _calc_ld through
the fixture tests/golden/g22_ld.npz (tests/golden/make_ld_fixture.py), and the estimator ld_ne on
numpy Wright-Fisher populations.  No GPU."""
import warnings

import numpy as np
import pytest

import _ld as T
from geonomics_amd.sim import ld as LD
from geonomics_amd.structs.analyses import SpeciesAnalyses


def test_map_positions_constant_rate_gives_the_product_formula():
    for r in (1e-4, 0.01, 0.2, 0.49):
        m = LD.map_positions(np.r_[0.0, np.full(199, r)])
        i, j = np.triu_indices(200, 1)
        c = LD.morgans_to_c(m[j] - m[i])
        want = 0.5 * (1.0 - (1.0 - 2.0 * r) ** (j - i))
        assert np.abs(c - want).max() <= 1e-14, r


def test_map_positions_ties_breaks_and_bad_rates():
    rates = np.array([0.0, 0.1, 0.0, 0.0, 0.5, 0.02, 0.5, 0.3])
    m = LD.map_positions(rates)
    assert m[0] == 0.0 and m[1] == m[2] == m[3]                  # r = 0: tied positions
    assert (np.diff(m) >= 0).all() and np.isfinite(m).all()
    assert m[4] - m[3] == pytest.approx(LD.BREAK_MORGANS, abs=1e-12)
    assert m[6] - m[5] == pytest.approx(LD.BREAK_MORGANS, abs=1e-12)
    # c is 0.5 to the last bit across a break, whatever lies on either side
    for i in range(4):
        for j in range(4, 8):
            assert LD.morgans_to_c(m[j] - m[i]) == 0.5
    # (behind two breaks the coordinate is 80: its last bit is 1.4e-14)
    assert LD.morgans_to_c(m[7] - m[6]) == pytest.approx(0.3, abs=1e-13)
    # the template's default: 0.5 everywhere
    m = LD.map_positions(np.r_[0.0, np.full(9, 0.5)])
    assert (LD.morgans_to_c(np.diff(m)) == 0.5).all()
    assert LD.drift_weight(0.5) == pytest.approx(1.0 / 3.0, abs=1e-16)
    for bad in ([], [0.0, -0.1], [0.0, np.nan], [0.0, np.inf]):
        with pytest.raises(ValueError):
            LD.map_positions(bad)
    assert LD.c_to_morgans(0.5) == np.inf and LD.c_to_morgans(0.0) == 0.0
    c = np.array([1e-6, 0.01, 0.25, 0.499])
    assert np.abs(LD.morgans_to_c(LD.c_to_morgans(c)) - c).max() <= 1e-15


def test_default_edges_and_min_minor():
    e = LD.default_edges('c', 20)
    assert e.size == 21 and e[0] == 0.0 and e[1] == 1e-3 and e[-1] == 0.5
    assert (np.diff(e) > 0).all()
    assert LD.default_edges('morgans', 5, 1.0)[-1] == 1.0
    e = LD.default_edges('loci', 10, n_loci=300)
    assert e[0] == 1 and e[-1] == 300 and (e == np.round(e)).all() and (np.diff(e) > 0).all()
    with pytest.raises(ValueError):
        LD.default_edges('cM')
    with pytest.raises(ValueError):
        LD.default_edges('c', 20, 0.7)
    assert LD.min_minor(0.05, 400) == 20 and LD.min_minor(0.05, 262) == 14
    assert LD.min_minor(0.0, 100) == 1
    for bad in ([1.0], [0.0, 0.0], [0.0, np.inf, np.inf], [0.0, np.nan], [2.0, 1.0]):
        with pytest.raises(ValueError):
            LD.check_edges(bad)
    assert LD.check_edges([0.0, 1.0, np.inf])[-1] == np.inf


def test_restatement_against_the_reference_calc_ld():
    fx = T.fixture()
    gts, ref = fx['genotypes'], fx['r2']
    L = gts.shape[1]
    got = LD.brute_bins(T.bits_of(gts), np.arange(L, dtype=np.float64), fx['edges'])
    i, j = np.triu_indices(L, 1)
    mine, theirs = got['r2'][i, j], ref[i, j]
    c1 = gts.sum(axis=(0, 2))
    mono = (c1 == 0) | (c1 == 2 * gts.shape[0])
    assert mono.sum() == 2 and (got['c1'] == c1).all() and (got['kept'] == ~mono).all()
    # the reference's NaN pairs are exactly the pairs with a monomorphic locus - and ours
    assert (np.isnan(theirs) == (mono[i] | mono[j])).all()
    assert (np.isnan(mine) == np.isnan(theirs)).all()
    ok = np.isfinite(theirs)
    rel = np.abs(mine[ok] - theirs[ok]) / np.maximum(np.abs(theirs[ok]), 1e-300)
    # (a pair in linkage equilibrium to the last bit: the reference's D carries its rounding)
    zero = theirs[ok] < 1e-28
    assert (np.abs(mine[ok][zero]) < 1e-28).all()
    print('r2: worst relative difference %.3g over %d pairs' % (rel[~zero].max(), (~zero).sum()))
    assert rel[~zero].max() <= 1e-12
    assert (ref.T[i, j][ok] == theirs[ok]).all()
    # the binned means computed from the reference's matrix
    assert (got['pairs'] == fx['pairs']).all()
    mean = got['sum_r2'] / got['pairs']
    assert np.abs(mean - fx['mean_r2']).max() <= 1e-12 * fx['mean_r2'].max()
    # complete LD between loci 11 and 12
    assert got['r2'][11, 12] == 1.0


def test_restatement_bins_edges_min_minor_and_the_weight():
    rng = np.random.RandomState(5)
    bits = (rng.rand(60, 12) < 0.4).astype(np.uint8)
    bits[:, 4] = 0
    bits[:, 7] = 0
    bits[3, 7] = 1                                                # a singleton
    pos = np.array([0, 0, 1, 2, 3, 3.5, 4, 6, 6, 8, 50, 51], dtype=np.float64)
    a = LD.brute_bins(bits, pos, [0.0, 1.0, 2.0, 60.0], 1, True)
    assert a['kept'].sum() == 11 and a['pairs'].sum() == 55
    assert a['sum_w'][0] == np.inf and np.isfinite(a['sum_w'][1:]).all()   # loci 0, 1: d = 0
    b = LD.brute_bins(bits, pos, [0.0, 1.0, 2.0, 60.0], 2, True)
    assert b['kept'].sum() == 10 and b['pairs'].sum() == 45
    # a pair on an edge belongs to the bin above; pairs outside every bin are not counted
    c = LD.brute_bins(bits, pos, [1.0, 2.0], 1, False)
    i, j = np.triu_indices(12, 1)
    ok = a['kept'][i] & a['kept'][j]
    d = (pos[j] - pos[i])[ok]
    assert c['pairs'][0] == ((d >= 1.0) & (d < 2.0)).sum() and not c['sum_w'].any()
    e = LD.brute_bins(bits, pos, [0.0, np.inf], 1, True)
    assert e['pairs'][0] == 55


def test_ld_ne_edge_cases():
    with pytest.warns(RuntimeWarning, match='no locus pairs'):
        assert np.isnan(LD.ld_ne(0, 0.0, 0.0, 100))
    assert LD.ld_ne(10, 10 * 0.009, 10 / 3.0, 100) == np.inf     # mean r2 < 1 / n
    assert LD.ld_ne(10, 10 * 0.01, 10 / 3.0, 100) == np.inf      # mean r2 == 1 / n
    # Waples' form for unlinked loci: 1 / (3 (r2 - 1 / n))
    assert LD.ld_ne(7, 7 * 0.0125, 7 / 3.0, 400) == pytest.approx(1 / (3 * (0.0125 - 1 / 400)))


def _wf_ne(r, gens, min_c, seed):
    bits = T.wright_fisher(200, 300, r, gens, seed)
    pos = LD.map_positions(np.r_[0.0, np.full(299, r)])
    lo = min(float(LD.c_to_morgans(min_c)), LD.BREAK_MORGANS / 2)
    got = LD.brute_bins(bits, pos, [lo, np.inf], LD.min_minor(0.05, 400), True)
    return LD.ld_ne(int(got['pairs'][0]), got['sum_r2'][0], got['sum_w'][0], 400), got


def test_ld_ne_recovers_n_of_a_wright_fisher_population():
    """monoecious Wright-Fisher, N = 200, 300 loci, everybody sampled, MAF >= 0.05, seeds 0..3;
    the estimate must be within 20 % of N.  Values seen here: unlinked, 25 generations:
    190.4, 218.8, 192.3, 199.7; adjacent c = 0.01, 120 generations, min_c = 0.05: 216.1, 210.7, 179.9, 202.9.
    This tests the estimator, not the kernel."""
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        for seed in range(4):
            ne, got = _wf_ne(0.5, 25, 0.5, seed)
            print('unlinked, seed %d: Ne = %.1f from %d pairs' % (seed, ne, got['pairs'][0]))
            assert got['pairs'][0] > 30000 and abs(ne - 200.0) <= 40.0, (seed, ne)
            ne, got = _wf_ne(0.01, 120, 0.05, seed)
            print('c = 0.01, seed %d: Ne = %.1f from %d pairs' % (seed, ne, got['pairs'][0]))
            assert got['pairs'][0] > 10000 and abs(ne - 200.0) <= 40.0, (seed, ne)


# ------------------------------------------------------------------ the public calls
class _Dev:
    """the device's ld_bins in numpy (brute_bins), on chromosome bits kept in slot order"""

    def __init__(self, gts):
        self.gts = gts
        self.L = gts.shape[1]
        self.W64 = (self.L + 1023) // 1024 * 16
        self.calls = 0

    def ld_bins(self, loci, pos, edges, slots=None, min_minor=1, morgans=False, max_work=0):
        from geonomics_amd import _native as nat
        self.calls += 1
        slots = np.arange(self.gts.shape[0]) if slots is None else slots
        nq = (2 * len(slots) + 63) // 64
        work = ((len(loci) + 63) // 64) * nq
        if max_work <= 0:
            return dict(work=work, c1=None, pairs=None)
        if work > max_work:
            raise nat.GnxError('gnx_ld_bins: %d tile-words of work exceed max_work = %d'
                               % (work, max_work))
        out = LD.brute_bins(T.bits_of(self.gts[slots])[:, loci], pos, edges, min_minor, morgans)
        out['work'] = work
        return out


class _Species(SpeciesAnalyses):
    """a Species stand-in: the real _calc_ld_decay and _calc_ne over the numpy device"""

    def __init__(self, gts, ids, rates):
        import types
        self._dev = _Dev(gts)
        self.ids = np.asarray(ids)
        self.gen_arch = types.SimpleNamespace(recombinations=types.SimpleNamespace(
            _positions=np.arange(gts.shape[1]), _rates=np.asarray(rates, dtype=float)))
        self._genomes_assigned = True

    def _geno_sample(self, individs):
        order = np.argsort(self.ids)
        if individs is None:
            return self.ids[order], order
        ids = np.sort(np.asarray(individs))
        return ids, order[np.searchsorted(self.ids[order], ids)]


def _stand_in():
    bits = T.wright_fisher(60, 90, 0.02, 30, 4)
    gts = bits.reshape(60, 2, 90).transpose(0, 2, 1).copy()
    ids = np.random.RandomState(2).permutation(60) * 3 + 5
    return _Species(gts, ids, np.r_[0.0, np.full(89, 0.02)]), gts, ids


def test_species_methods_over_a_numpy_device():
    spp, gts, ids = _stand_in()
    order = np.argsort(ids)
    bits = T.bits_of(gts[order])
    pos = LD.map_positions(np.r_[0.0, np.full(89, 0.02)])
    mm = LD.min_minor(0.05, 120)
    res = spp._calc_ld_decay(n_bins=6)
    assert spp._dev.calls == 1                                   # one device call
    edges = LD.default_edges('c', 6)
    ref = LD.brute_bins(bits, pos, LD.c_to_morgans(edges), mm, True)
    want = LD.decay_stats(ref['pairs'], ref['sum_r2'], ref['sum_r4'], ref['sum_d'], ref['sum_w'],
                          True)
    assert (res['pairs'] == ref['pairs']).all() and (res['ids'] == ids[order]).all()
    for k in want:
        np.testing.assert_array_equal(res[k], want[k])
    assert res['n_chrom'] == 120 and res['n_loci_kept'] == ref['kept'].sum()
    assert (res['loci'] == np.arange(90)).all() and res['work'] == 2 * 2
    # c at the mean map distance lies inside its bin
    ok = res['pairs'] > 0
    assert ((res['mean_c'][ok] >= edges[:-1][ok]) & (res['mean_c'][ok] <= edges[1:][ok])).all()
    sub = spp._calc_ld_decay(unit='loci', edges=[1, 3, 10], individs=ids[:20],
                             loci=[5, 9, 7, 30, 31, 60], min_maf=0.0)
    assert (sub['loci'] == [5, 7, 9, 30, 31, 60]).all() and sub['n_chrom'] == 40
    assert np.isnan(sub['mean_c']).all() and np.isnan(sub['expected_w']).all()
    ne = spp._calc_ne(min_c=0.1)
    ref = LD.brute_bins(bits, pos, [float(LD.c_to_morgans(0.1)), np.inf], mm, True)
    assert ne['pairs'] == ref['pairs'][0] and ne['min_c'] == 0.1 and ne['n_chrom'] == 120
    assert ne['Ne'] == LD.ld_ne(int(ref['pairs'][0]), ref['sum_r2'][0], ref['sum_w'][0], 120)
    assert ne['r2_drift'] == ne['mean_r2'] - 1 / 120
    # unlinked pairs only: none on this one chromosome
    with pytest.warns(RuntimeWarning, match='no locus pairs'):
        assert np.isnan(spp._calc_ne(min_c=0.5)['Ne'])


def test_species_methods_refuse_what_they_cannot_do():
    import types
    spp, gts, ids = _stand_in()
    with pytest.raises(ValueError, match="method: 'ld'"):
        spp._calc_ne(method='temporal')
    with pytest.raises(ValueError, match='min_c'):
        spp._calc_ne(min_c=0.6)
    with pytest.raises(ValueError, match='unit'):
        spp._calc_ld_decay(unit='cM')
    with pytest.raises(ValueError, match='edges or max_dist'):
        spp._calc_ld_decay(edges=[0, 0.1], max_dist=0.2)
    for bad in ([0.0, 0.5, 0.6], [0.1, 0.6, 0.7, 0.8], [-0.1, 0.2]):
        with pytest.raises(ValueError, match='edges in c'):
            spp._calc_ld_decay(edges=bad)
    assert spp._calc_ld_decay(edges=[0.0, 0.2, 0.7])['pairs'].shape == (2,)
    with pytest.raises(ValueError, match='min_maf'):
        spp._calc_ld_decay(min_maf=0.7)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='max_work'):
            spp._calc_ld_decay(max_work=bad)
    with pytest.raises(ValueError, match='exceed max_work = 3.*n=.*loci=.*max_dist'):
        spp._calc_ld_decay(max_work=3)
    spp._LD_MAX_WORK = 3
    with pytest.raises(ValueError, match='calc_ne.*exceed max_work = 3'):
        spp._calc_ne()
    del spp._LD_MAX_WORK
    spp._genomes_assigned = False
    for f in (spp._calc_ld_decay, spp._calc_ne):
        with pytest.raises(ValueError, match='burn the model in first'):
            f()
    spp.gen_arch = None
    for f in (spp._calc_ld_decay, spp._calc_ne):
        with pytest.raises(ValueError, match='no genomes'):
            f()
    spp.gen_arch, spp._dev.L = types.SimpleNamespace(), 0
    with pytest.raises(ValueError, match='no genomes'):
        spp._calc_ne()


def test_signatures_the_tiled_refusal_the_statistic_and_the_binding():
    import inspect
    from geonomics_amd import _native
    from geonomics_amd.sim import stats as ST
    from geonomics_amd.sim.model import Model
    from geonomics_amd.structs.species import Species
    from geonomics_amd.structs.tiled import TiledSpecies
    assert list(inspect.signature(Species._calc_ld_decay).parameters) == [
        'self', 'edges', 'n_bins', 'unit', 'max_dist', 'individs', 'loci', 'min_maf', 'max_work']
    assert list(inspect.signature(Species._calc_ne).parameters) == [
        'self', 'method', 'min_c', 'min_maf', 'individs', 'loci']
    assert 'spp' in inspect.signature(Model.calc_ld_decay).parameters
    assert 'spp' in inspect.signature(Model.calc_ne).parameters
    for f in (TiledSpecies._calc_ld_decay, TiledSpecies._calc_ne):
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            f(object())
    sc = ST._StatsCollector
    assert sc.calc_fn_dict['ne'] is ST._calc_ne and 'ne' in sc._needs_genome
    assert sc.file_suffix_dict['ne'] == sc.file_suffix_dict['Nt']
    spp = _stand_in()[0]
    assert ST._calc_ne(spp, min_c=0.1) == spp._calc_ne(min_c=0.1)['Ne']
    for name in ('gnx_ld_bins', 'gnx_ld_budget', 'gnx_ld_info'):
        assert name in _native.EXPORTS
