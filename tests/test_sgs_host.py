"""Fine-scale spatial genetic structure, host side (no GPU): sim/sgs.py's statistics from the
ten per-class sums against the same statistics taken from the pairs themselves (tests/_sgs.py:
the explicit Loiselle matrix, np.polyfit), and Species._calc_spatial_structure /
Model.calc_spatial_structure over a numpy stand-in for the device.  Everything must agree to
BAR = 1e-9 relative (measured: 2.5e-14); permutation p-values are counts of comparisons
and are compared for equality only after asserting that no permuted statistic lies within
GAP = 1e-8 relative of the observed one."""
import inspect
import types
import warnings

import numpy as np
import pytest

import _sgs as O
from geonomics_amd.sim import mmrr as M
from geonomics_amd.sim import sgs as G
from geonomics_amd.structs import species as S
from geonomics_amd.structs.analyses import SpeciesAnalyses

BAR = 1e-9
GAP = 1e-8
EDGES = np.array([0.0, 1.0, 2.0, 3.5, 6.0])


def sample(n=48, L=40, seed=3, side=12.0):
    """dosages with isolation by distance (allele frequencies follow a smooth field in x, y),
    fp32 coordinates, two monomorphic loci"""
    rng = np.random.RandomState(seed)
    x = rng.uniform(0, side, n).astype(np.float32)
    y = rng.uniform(0, side, n).astype(np.float32)
    ph = rng.uniform(0, 2 * np.pi, (2, L))
    p = 0.5 + 0.4 * np.sin(x[:, None] / side * 3 + ph[0]) * np.cos(y[:, None] / side * 3 + ph[1])
    D = rng.binomial(2, p)
    D[:, 0], D[:, 1] = 0, 2
    return x, y, D


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert (np.isnan(got) == np.isnan(want)).all(), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)
    assert (err <= BAR).all(), (what, err.max())
    return float(err.max()) if err.size else 0.0


def from_sums(x, y, D, edges, fit_range=None, perms=None):
    n = D.shape[0]
    s_l = D.sum(axis=0)
    w = G.locus_terms(s_l, n)[0]
    isums, fsums, nz, _ = O.brute_sums(x, y, D, edges, w)
    pI = pS = None
    if perms is not None:
        got = [O.brute_sums(x, y, O.permuted(D, p), edges, w) for p in perms]
        pI, pS = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
    return G.spatial_structure(isums, fsums, s_l, n, fit_range, pI, pS)


@pytest.mark.parametrize('fit_range', [None, (1, 3), (0, 1)])
def test_the_statistics_from_sums_are_those_of_the_pairs(fit_range):
    x, y, D = sample()
    got = from_sums(x, y, D, EDGES, fit_range)
    want = O.explicit_stats(x, y, D, EDGES, fit_range)
    assert (got['pairs'] == want['pairs']).all() and (got['pairs'] > 0).all()
    worst = max(close(got[k], want[k], k)
                for k in ('mean_r', 'mean_lnr', 'F', 'dist2', 'slope', 'F1', 'Sp', 'Nb'))
    print('fit_range %s: worst relative error %.3g' % (fit_range, worst))
    assert got['slope'] < 0 and got['Sp'] > 0 and got['Nb'] > 0      # the sample has IBD


def test_the_permutation_p_values_are_those_of_the_pairs():
    x, y, D = sample()
    n = D.shape[0]
    rows = M.draw_row_shuffles(n, 49, seed=5)
    got = from_sums(x, y, D, EDGES, None, rows)
    obs = O.explicit_stats(x, y, D, EDGES)
    per = [O.explicit_stats(x, y, O.permuted(D, r), EDGES) for r in rows]
    pb = np.array([p['slope'] for p in per])
    pF = np.stack([p['F'] for p in per])
    close(got['perm_slope'], pb, 'perm_slope')
    close(got['perm_F'], pF, 'perm_F')
    assert np.abs(pb - obs['slope']).min() > GAP * abs(obs['slope'])
    centre = pF.mean(axis=0)
    dev_p, dev_o = np.abs(pF - centre), np.abs(obs['F'] - centre)
    assert (np.abs(dev_p - dev_o).min(axis=0) > GAP * dev_o).all()
    assert got['p_slope'] == (1 + (pb <= obs['slope']).sum()) / 50
    assert (got['p_F'] == (1 + (dev_p >= dev_o).sum(axis=0)) / 50).all()
    assert got['nperm'] == 49 and got['p_slope'] <= 0.1              # IBD is detected


def test_an_empty_class_is_nan_and_does_not_touch_the_fit():
    x, y, D = sample()
    edges = np.array([0.0, 1.0, 1.0 + 1e-9, 2.0, 3.5, 6.0])          # class 1 holds no pair
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = from_sums(x, y, D, edges)
    assert got['pairs'][1] == 0
    for k in ('mean_r', 'mean_lnr', 'F', 'dist2'):
        assert np.isnan(got[k][1]) and np.isfinite(np.delete(got[k], 1)).all(), k
    ref = from_sums(x, y, D, EDGES)
    close(got['slope'], ref['slope'], 'slope')
    close(np.delete(got['F'], 1), ref['F'], 'F')


def test_no_polymorphic_locus_gives_nan_and_one_warning():
    x, y, D = sample()
    D[:] = D[0]                                       # everybody the same genotype
    D[:, ::2] = 2
    D[:, 1::2] = 0
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        got = from_sums(x, y, D, EDGES, perms=M.draw_row_shuffles(D.shape[0], 3, seed=1))
    assert len(w) == 1 and 'polymorphic' in str(w[0].message)
    for k in ('F', 'slope', 'F1', 'Sp', 'Nb', 'perm_slope', 'p_slope', 'p_F'):
        assert np.isnan(got[k]).all(), k
    assert np.isfinite(got['mean_r']).all() and (got['dist2'] == 0).all()


def test_kinship_rising_with_distance_gives_nan_nb_and_a_warning():
    # two genotypes on a chessboard of spacing 1: unlike at distance 1, alike at distance sqrt 2
    gx, gy = np.meshgrid(np.arange(6), np.arange(6))
    x, y = gx.ravel().astype(np.float32), gy.ravel().astype(np.float32)
    D = np.where(((gx + gy) % 2).ravel()[:, None] == 1, 2, 0) * np.ones((1, 8), np.int64)
    edges = np.array([0.5, 1.2, 1.6])
    with pytest.warns(UserWarning, match='Sp = .* <= 0'):
        got = from_sums(x, y, D, edges)
    want = O.explicit_stats(x, y, D, edges)
    assert got['slope'] > 0 and got['Sp'] < 0 and np.isnan(got['Nb']) and np.isnan(want['Nb'])
    close(got['slope'], want['slope'], 'slope')
    close(got['Sp'], want['Sp'], 'Sp')


def test_default_edges_and_argument_checks_of_the_host_functions():
    e = G.default_edges(1.0, 6.0, 10)
    assert e.size == 11 and e[0] == 1.0 and e[-1] == 6.0
    np.testing.assert_allclose(np.diff(np.log(e)), np.log(6.0) / 10, rtol=1e-12)
    for lo, hi, k in ((0.0, 6.0, 10), (2.0, 2.0, 3), (1.0, 6.0, 0), (1.0, 6.0, 33),
                      (1.0, np.inf, 4)):
        with pytest.raises(ValueError):
            G.default_edges(lo, hi, k)
    for bad in ([1.0], [1.0, 1.0], [2.0, 1.0], [-1.0, 1.0], [0.0, np.nan], np.arange(34.0)):
        with pytest.raises(ValueError, match='edges'):
            G.check_edges(bad)
    x, y, D = sample()
    s_l = D.sum(axis=0)
    isums, fsums, _, _ = O.brute_sums(x, y, D, EDGES, G.locus_terms(s_l, D.shape[0])[0])
    for fr in ((0, 0), (2, 1), (0, 5), (-1, 2), 3, 'ab'):
        with pytest.raises(ValueError, match='fit_range'):
            G.spatial_structure(isums, fsums, s_l, D.shape[0], fr)
    with pytest.raises(ValueError, match='isums'):
        G.spatial_structure(isums[:, :2], fsums, s_l, D.shape[0])
    with pytest.raises(ValueError, match='at least 2'):
        G.spatial_structure(isums, fsums, s_l, 1)
    with pytest.raises(ValueError, match='perm_isums'):
        G.spatial_structure(isums, fsums, s_l, D.shape[0], None, isums[None, :2], fsums[None])


# ------------------------------------------------------------------ the public calls
class _Dev:
    """the device's sgs_sums and stats_group_counts in numpy, on columns kept in slot order"""

    def __init__(self, x, y, D):
        self.x, self.y, self.D = x, y, D
        self.L = D.shape[1]
        self.W64 = (self.L + 1023) // 1024 * 16
        self.calls = []

    def _loci(self, locus_mask):
        loci = np.arange(self.L)
        if locus_mask is None:
            return loci
        return loci[(locus_mask[loci >> 6] >> (loci & 63).astype(np.uint64)) & np.uint64(1) == 1]

    def stats_group_counts(self, slots, group_start):
        assert list(group_start) == [0, len(slots)]
        c1 = self.D[slots].sum(axis=0)[None, :].astype(np.int32)
        return c1, (self.D[slots] == 1).sum(axis=0)[None, :].astype(np.int32)

    def sgs_sums(self, edges, slots=None, locus_mask=None, locus_weight=None, perm=None,
                 max_work=0):
        self.calls.append(dict(edges=edges, slots=slots, mask=locus_mask, weight=locus_weight,
                               perm=perm, max_work=max_work))
        slots = np.arange(self.D.shape[0]) if slots is None else slots
        loci = self._loci(locus_mask)
        n = len(slots)
        work = n * (n - 1) // 2 * len(np.unique(loci >> 6))
        if max_work <= 0:
            return dict(work=work, isums=None, fsums=None, n_zero=None)
        assert work <= max_work
        D = self.D[slots][:, loci]
        if perm is not None:
            D = D[perm]
        w = None if locus_weight is None else locus_weight[loci]
        isums, fsums, nz, _ = O.brute_sums(self.x[slots], self.y[slots], D, edges, w)
        return dict(work=work, isums=isums, fsums=fsums, n_zero=nz)


class _Species(SpeciesAnalyses):
    """a Species stand-in: the real _calc_spatial_structure over the numpy device"""

    def __init__(self, x, y, D, ids, dim=(12, 12)):
        self._dev = _Dev(x, y, D)
        self.ids = np.asarray(ids)
        self.gen_arch = types.SimpleNamespace(traits={})
        self._genomes_assigned = True
        self._rng = np.random.RandomState(77)
        self._land_ref = types.SimpleNamespace(dim=dim)

    def _geno_sample(self, individs):
        order = np.argsort(self.ids)
        if individs is None:
            return self.ids[order], order
        ids = np.sort(np.asarray(individs))
        return ids, order[np.searchsorted(self.ids[order], ids)]

    def __iter__(self):
        return iter(np.sort(self.ids).tolist())

    def _get_individs(self, ids):
        return {int(i): None for i in ids}


def _model(spp):
    from geonomics_amd.sim.model import Model
    mod = types.SimpleNamespace(comm={0: spp}, _rng=np.random.RandomState(9))
    for name in ('_get_spp_num', '_test_sample', 'calc_spatial_structure'):
        setattr(mod, name, types.MethodType(getattr(Model, name), mod))
    return mod


def _pop(seed=3):
    x, y, D = sample(seed=seed)
    ids = np.random.RandomState(seed).permutation(D.shape[0]) * 3 + 1   # slot order != id order
    return _Species(x, y, D, ids), x, y, D, ids


def test_the_public_call_is_the_host_path_on_the_sample_in_id_order():
    spp, x, y, D, ids = _pop()
    mod = _model(spp)
    o = np.argsort(ids)
    res = mod.calc_spatial_structure(edges=EDGES, nperm=19, seed=4)
    rows = M.draw_row_shuffles(ids.size, 19, seed=4)
    want = from_sums(x[o], y[o], D[o], EDGES, None, rows)
    assert (res['ids'] == ids[o]).all() and res['n'] == ids.size and res['n_zero'] == 0
    for k in want:
        np.testing.assert_array_equal(res[k], want[k], err_msg=k)
    np.testing.assert_array_equal(res['edges'], EDGES)
    assert res['work'] == ids.size * (ids.size - 1) // 2 * 1
    calls = spp._dev.calls
    assert len(calls) == 1 + 1 + 19 and calls[0]['max_work'] == 0
    assert all(c['max_work'] == S.Species._SGS_MAX_WORK for c in calls[1:])
    assert calls[1]['perm'] is None and (calls[2]['perm'] == rows[0]).all()
    assert calls[2]['perm'].dtype == np.int32
    # default edges: n_classes classes equal in ln r from one cell to a quarter of the side
    res = mod.calc_spatial_structure(n_classes=4)
    np.testing.assert_array_equal(res['edges'], G.default_edges(1.0, 3.0, 4))
    assert 'p_slope' not in res
    res = mod.calc_spatial_structure(n_classes=3, max_dist=5.0, fit_range=(1, 3))
    np.testing.assert_array_equal(res['edges'], G.default_edges(1.0, 5.0, 3))
    close(res['slope'], O.explicit_stats(x[o], y[o], D[o], res['edges'], (1, 3))['slope'], 'b')
    # individs, loci and a random sample of n reach the device call
    some = ids[::3][::-1]
    loci = np.array([5, 2, 30, 31])
    res = mod.calc_spatial_structure(edges=EDGES, individs=some, loci=loci)
    so = np.argsort(ids)[::1]
    keep = np.isin(ids[so], some)
    want = O.explicit_stats(x[so][keep], y[so][keep], D[so][keep][:, np.sort(loci)], EDGES)
    for k in ('F', 'slope', 'Sp', 'dist2'):
        close(res[k], want[k], k)
    w = spp._dev.calls[-1]['weight']
    assert w.shape == (D.shape[1],) and (np.nonzero(w)[0] == np.sort(loci)).all()
    res = mod.calc_spatial_structure(edges=EDGES, n=20)
    assert res['n'] == 20 and res['ids'].size == 20 and np.isin(res['ids'], ids).all()


def test_the_species_method_checks_its_arguments():
    spp, x, y, D, ids = _pop()
    f = spp._calc_spatial_structure
    with pytest.raises(ValueError, match='not both'):
        f(edges=EDGES, max_dist=3.0)
    with pytest.raises(ValueError, match='edges'):
        f(edges=[3.0, 1.0])
    with pytest.raises(ValueError, match='n_classes'):
        f(n_classes=40)
    with pytest.raises(ValueError, match='0 < lo < hi'):
        f(max_dist=0.5)
    with pytest.raises(ValueError, match='nperm'):
        f(edges=EDGES, nperm=-1)
    with pytest.raises(ValueError, match='nperm'):
        f(edges=EDGES, nperm=2.5)
    with pytest.raises(ValueError, match='fit_range'):
        f(edges=EDGES, fit_range=(0, 9))
    with pytest.raises(ValueError, match='max_work'):
        f(edges=EDGES, max_work=0)
    with pytest.raises(ValueError, match='at least 2'):
        f(edges=EDGES, individs=ids[:1])
    with pytest.raises(ValueError, match='loci'):
        f(edges=EDGES, loci=[D.shape[1]])
    assert spp._dev.calls == []                      # all of that before the device is asked
    with pytest.raises(ValueError, match=r'pair-words.*exceed max_work = 100.*n=.*loci=.*max_dist'):
        f(edges=EDGES, max_work=100)
    assert len(spp._dev.calls) == 1 and spp._dev.calls[0]['max_work'] == 0
    with pytest.raises(ValueError, match='give individs or n, not both'):
        _model(spp).calc_spatial_structure(individs=ids[:5], n=3)
    spp.gen_arch = None
    with pytest.raises(ValueError, match='no genomes'):
        f(edges=EDGES)
    spp.gen_arch = types.SimpleNamespace(traits={})
    spp._genomes_assigned = False
    with pytest.raises(ValueError, match='burn the model in first'):
        f(edges=EDGES)


def test_the_public_call_has_the_documented_signature():
    from geonomics_amd.sim.model import Model
    sig = inspect.signature(Model.calc_spatial_structure)
    assert list(sig.parameters) == ['self', 'spp', 'edges', 'n_classes', 'max_dist', 'individs',
                                    'n', 'loci', 'nperm', 'seed', 'fit_range', 'max_work']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['spp'], d['n_classes'], d['nperm']) == (0, 10, 0)
    assert all(d[k] is None for k in ('edges', 'max_dist', 'individs', 'n', 'loci', 'seed',
                                      'fit_range', 'max_work'))
    sig = inspect.signature(S.Species._calc_spatial_structure)
    assert list(sig.parameters) == ['self', 'edges', 'n_classes', 'max_dist', 'individs', 'loci',
                                    'nperm', 'seed', 'fit_range', 'max_work']


def test_a_tiled_species_refuses():
    from geonomics_amd.structs.tiled import TiledSpecies
    with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
        TiledSpecies._calc_spatial_structure(object())


def test_the_binding_exports_the_sums():
    from geonomics_amd import _native as nat
    assert 'gnx_sgs_sums' in nat.EXPORTS
    assert callable(nat.Device.sgs_sums)
