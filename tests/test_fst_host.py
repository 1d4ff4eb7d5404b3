"""The host arithmetic of Model.calc_fst, calc_diversity and calc_sfs (geonomics_amd/sim/fst.py)
on counts taken with numpy: against the reference's recorded Fst (tests/golden/g21_fst.npz,
written by tests/golden/make_fst_fixture.py from the reference's own calc_Fsts_mod) and against
direct restatements.  No GPU.

Bound against the reference.  Both sides evaluate Fst = (Ht - Hs) / Ht in the same order from
the same integers, so they should agree to the last bit; the bound allows for a library that
rounds differently: f and het are single divisions of exact integers (1 rounding each), Ht
takes 5 more operations and Hs 2 (est_Hs: 5), each within 2^-53 relatively, the difference
Ht - Hs carries their absolute errors, and the division rounds once more:

    |Fst - Fst_ref| <= 16 * 2^-53 * (1 + Hs / Ht)

and for the nanmean over the m comparable loci of a pair, the mean of those bounds plus, for
the two sums in any order and their divisions, 2 (m + 1) 2^-53 mean(|Fst_ref| + bound).

Measured here: the worst |difference| is 0.0 of that bound for both est_Hs settings (the
arrays are bit-identical), with the identical NaN pattern."""
import csv
import itertools
import os

import numpy as np
import pytest

from geonomics_amd.sim import fst as F

HERE = os.path.dirname(os.path.abspath(__file__))
U53 = 2.0 ** -53
NAN_CAP = 0.15


def fixture():
    d = np.load(os.path.join(HERE, 'golden', 'g21_fst.npz'))
    return {k: d[k] for k in d.files}


def counts_numpy(gts, labels, G=None):
    """(n [G], cnt1 [G][L], cnt_het [G][L]) of genotypes [n][L][2] by label"""
    G = int(labels.max()) + 1 if G is None else G
    gts = gts.astype(np.int64)
    n = np.array([(labels == g).sum() for g in range(G)], dtype=np.int64)
    cnt1 = np.stack([gts[labels == g].sum(axis=(0, 2)) for g in range(G)])
    het = np.stack([(gts[labels == g].sum(axis=2) == 1).sum(axis=0) for g in range(G)])
    return n, cnt1.astype(np.int32), het.astype(np.int32)


def hs_over_ht(cnt1, cnt_het, n, a, b, est_Hs):
    f0, f1 = cnt1[a] / (2 * n[a]), cnt1[b] / (2 * n[b])
    m = (f0 + f1) / 2
    Ht = 2 * m * (1 - m)
    Hs = f0 * (1 - f0) + f1 * (1 - f1) if est_Hs else (cnt_het[a] / n[a] + cnt_het[b] / n[b]) / 2
    with np.errstate(divide='ignore', invalid='ignore'):
        return Hs / Ht


def assert_meets_reference(fx, cnt1, cnt_het, n):
    """fst_hsht on these counts against the fixture: NaN cap, NaN pattern, the module's bound
    -> the worst fraction of the bound"""
    worst = 0.0
    for est, key in ((False, 'fst'), (True, 'fst_est_Hs')):
        for k, (a, b) in enumerate(fx['pairs']):
            ref = fx[key][k]
            assert np.isnan(ref).mean() <= NAN_CAP          # NaNs cannot hide a failure
            got = F.fst_hsht(cnt1, cnt_het, n, int(a), int(b), est_Hs=est)
            np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
            ok = ~np.isnan(ref)
            bound = 16 * U53 * (1 + hs_over_ht(cnt1, cnt_het, n, int(a), int(b), est)[ok])
            err = np.abs(got[ok] - ref[ok])
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (est, a, b, float((err / bound).max()))
            # the nanmean of m entries: the entries' own bounds average, each side's sum of m
            # terms in any order is within m 2^-53 sum |terms| and its division rounds once
            mean_key = 'mean_fst_est_Hs' if est else 'mean_fst'
            m = int(ok.sum())
            mean_bound = bound.mean() + 2 * (m + 1) * U53 * (np.abs(ref[ok]) + bound).mean()
            assert abs(np.nanmean(got) - fx[mean_key][k]) <= mean_bound
    return worst


def test_fst_hsht_reproduces_the_reference():
    fx = fixture()
    n, cnt1, cnt_het = counts_numpy(fx['genotypes'], fx['labels'])
    assert n.tolist() == [61, 37, 59]
    worst = assert_meets_reference(fx, cnt1, cnt_het, n)
    print('fst_hsht against the reference: worst error / bound %.3g' % worst)
    # loci fixed oppositely in groups 0 and 1: Fst = 1; fixed alike everywhere: NaN, or 0
    got = F.fst_hsht(cnt1, cnt_het, n, 0, 1)
    assert (got[8:12] == 1.0).all() and np.isnan(got[:8]).all()
    z = F.fst_hsht(cnt1, cnt_het, n, 0, 1, include_zeros=True)
    assert (z[:8] == 0.0).all() and not np.isnan(z).any()
    # calc_fst keys its dict as calc_Fsts_mod does, and the means are its nanmeans
    res = F.calc_fst([0, 1, 2], n, cnt1, cnt_het, method='HsHt', mean=True)
    assert [*res] == [tuple(p) for p in fx['pairs'].tolist()]
    for k, key in enumerate(res):
        assert res[key] == np.nanmean(F.fst_hsht(cnt1, cnt_het, n, *key))


def test_fst_hsht_empty_group_is_nan():
    fx = fixture()
    n, cnt1, cnt_het = counts_numpy(fx['genotypes'], fx['labels'], G=4)
    assert n[3] == 0
    assert np.isnan(F.fst_hsht(cnt1, cnt_het, n, 0, 3)).all()
    assert np.isnan(F.fst_hsht(cnt1, cnt_het, n, 3, 1, include_zeros=True)).all()
    assert np.isnan(F.calc_fst([0, 1, 2, 3], n, cnt1, cnt_het)[(2, 3)])


def _random_counts(rng, sizes, L):
    labels = np.repeat(np.arange(len(sizes)), sizes)
    gts = (rng.rand(labels.size, L, 2) < rng.uniform(0, 1, L)[None, :, None]).astype(np.uint8)
    gts[:, :3] = 0
    gts[:, 3:5] = 1
    return gts, labels, counts_numpy(gts, labels)


def test_pi_is_the_mean_pairwise_difference():
    rng = np.random.RandomState(1)
    gts, labels, (n, cnt1, cnt_het) = _random_counts(rng, (20, 7, 1), 90)
    d = F.diversity(cnt1, cnt_het, n)
    for g in range(3):
        chrom = gts[labels == g].transpose(0, 2, 1).reshape(-1, 90).astype(np.int64)   # [2n][L]
        m = chrom.shape[0]
        assert m <= 40
        diffs = [np.sum(chrom[i] != chrom[j]) for i, j in itertools.combinations(range(m), 2)]
        # L terms c (2n - c) / C(2n, 2), each rounded once, summed in any order
        tol = 90 * U53 * np.mean(diffs) + 1e-300
        assert abs(d['pi'][g] - np.mean(diffs)) <= 2 * tol
        seg = ((chrom.sum(0) > 0) & (chrom.sum(0) < m)).sum()
        assert d['S'][g] == seg and d['n'][g] == n[g]
        f = chrom.mean(0)
        assert d['Ho'][g] == np.mean(cnt_het[g] / n[g])
        np.testing.assert_allclose(d['He'][g], np.mean(2 * f * (1 - f) * m / (m - 1)), rtol=1e-14)
        np.testing.assert_allclose(d['Fis'][g], 1 - d['Ho'][g] / d['He'][g], rtol=1e-14)


def test_theta_w_and_tajima_constants():
    a1 = sum(1.0 / i for i in range(1, 10))
    a2 = sum(1.0 / i ** 2 for i in range(1, 10))
    c = F.tajima_constants(10)
    assert abs(c[0] - a1) <= 4 * U53 * a1 and abs(c[1] - a2) <= 4 * U53 * a2
    m = 10
    b1, b2 = (m + 1) / (3 * (m - 1)), 2 * (m * m + m + 3) / (9 * m * (m - 1))
    e1 = (b1 - 1 / a1) / a1
    e2 = (b2 - (m + 2) / (a1 * m) + a2 / a1 ** 2) / (a1 ** 2 + a2)
    np.testing.assert_allclose(c[2:], [e1, e2], rtol=1e-13)
    rng = np.random.RandomState(2)
    gts, labels, (n, cnt1, cnt_het) = _random_counts(rng, (5,), 60)
    d = F.diversity(cnt1, cnt_het, n)
    S = d['S'][0]
    assert S > 0
    np.testing.assert_allclose(d['theta_w'][0], S / a1, rtol=1e-14)
    np.testing.assert_allclose(d['tajima_d'][0], (d['pi'][0] - S / a1)
                               / np.sqrt(e1 * S + e2 * S * (S - 1)), rtol=1e-12)


def test_tajima_d_nan_cases():
    # S = 0: every locus fixed
    d = F.diversity(np.array([[0, 10, 0]]), np.array([[0, 0, 0]]), np.array([5]))
    assert d['S'][0] == 0 and np.isnan(d['tajima_d'][0]) and d['pi'][0] == 0.0
    # 2n < 4: one individual
    d = F.diversity(np.array([[1, 2, 0]]), np.array([[1, 0, 0]]), np.array([1]))
    assert d['S'][0] == 1 and np.isnan(d['tajima_d'][0]) and d['pi'][0] == 1.0
    # an empty group: everything NaN, S = 0
    d = F.diversity(np.array([[0, 0]]), np.array([[0, 0]]), np.array([0]))
    assert d['S'][0] == 0 and all(np.isnan(d[k][0]) for k in ('pi', 'theta_w', 'tajima_d', 'Ho'))


def test_sfs():
    rng = np.random.RandomState(3)
    gts, labels, (n, cnt1, cnt_het) = _random_counts(rng, (9, 4, 13), 77)
    s = F.sfs(cnt1, n)
    assert s.shape == (3, 27) and (s.sum(axis=1) == 77).all()
    for g in range(3):
        np.testing.assert_array_equal(s[g], np.bincount(cnt1[g], minlength=27))
        assert s[g, 2 * n[g] + 1:].sum() == 0 and s[g, 0] >= 3 and s[g, 2 * n[g]] >= 2
    sf = F.sfs(cnt1, n, folded=True)
    assert sf.shape == (3, 14) and (sf.sum(axis=1) == 77).all()
    for g in range(3):
        m = 2 * int(n[g])
        by_hand = np.zeros(14, np.int64)
        for c in range(m + 1):
            by_hand[min(c, m - c)] += s[g, c]
        np.testing.assert_array_equal(sf[g], by_hand)


def test_fst_hudson_restated():
    rng = np.random.RandomState(4)
    gts, labels, (n, cnt1, cnt_het) = _random_counts(rng, (11, 6, 17), 50)
    for a, b in itertools.combinations(range(3), 2):
        num, den = F.fst_hudson(cnt1, n, a, b)
        for l in range(50):
            n1, n2 = 2 * int(n[a]), 2 * int(n[b])
            p1, p2 = int(cnt1[a, l]) / n1, int(cnt1[b, l]) / n2
            N = (p1 - p2) ** 2 - p1 * (1 - p1) / (n1 - 1) - p2 * (1 - p2) / (n2 - 1)
            D = p1 * (1 - p2) + p2 * (1 - p1)
            assert num[l] == N and den[l] == D
        res = F.calc_fst([0, 1, 2], n, cnt1, cnt_het, method='hudson')
        assert res[(a, b)] == np.mean(num) / np.mean(den)
        per = F.calc_fst([0, 1, 2], n, cnt1, cnt_het, method='hudson', mean=False)[(a, b)]
        np.testing.assert_array_equal(per[den > 0], (num / np.where(den > 0, den, 1))[den > 0])
        assert np.isnan(per[den == 0]).all() and (den == 0).sum() >= 5
    assert np.isnan(F.fst_hudson(cnt1, np.array([11, 0, 17]), 0, 1)[0]).all()


def test_fst_var_restated():
    rng = np.random.RandomState(5)
    gts, labels, (n, cnt1, cnt_het) = _random_counts(rng, (11, 6, 17), 50)
    f = cnt1 / (2 * n)[:, None]
    v = F.fst_var(cnt1, n)
    for l in range(50):
        m = np.mean(f[:, l])
        exp = 0.0 if m * (1 - m) == 0 else np.var(f[:, l]) / (m * (1 - m))
        assert abs(v[l] - exp) <= 8 * U53 * abs(exp)
    assert (v[:5] == 0.0).all()
    assert F.calc_fst([0, 1, 2], n, cnt1, cnt_het, method='var') == np.mean(v)
    with pytest.raises(ValueError, match='method'):
        F.calc_fst([0, 1, 2], n, cnt1, cnt_het, method='wc')


def test_make_groups():
    ids = np.array([3, 8, 9, 14, 20, 21, 40])
    lab = np.array([1, 0, -1, 1, 3, 0, -5])
    names, order, gs = F.make_groups(ids, lab)
    assert names == [0, 1, 2, 3]                     # group 2 is empty
    assert gs.tolist() == [0, 2, 4, 4, 5] and gs.dtype == np.int64
    assert order.tolist() == [1, 5, 0, 3, 4]         # the negative labels are left out
    names_d, order_d, gs_d = F.make_groups(ids, {1: [14, 3], 0: (21, 8), 2: [], 3: {20}})
    assert names_d == names
    np.testing.assert_array_equal(order_d, order)
    np.testing.assert_array_equal(gs_d, gs)
    names_s, _, gs_s = F.make_groups(ids, {'north': [3, 8], 'a': [9]})
    assert names_s == ['a', 'north'] and gs_s.tolist() == [0, 1, 3]
    with pytest.raises(ValueError, match='not alive'):
        F.make_groups(ids, {0: [3, 4]})
    with pytest.raises(ValueError, match='not alive'):
        F.make_groups(ids, {0: [41]})
    with pytest.raises(ValueError, match='two groups'):
        F.make_groups(ids, {0: [3, 8], 1: [8, 9]})
    with pytest.raises(ValueError, match='labels for'):
        F.make_groups(ids, lab[:-1])
    with pytest.raises(ValueError, match='at least one group'):
        F.make_groups(ids, {})
    with pytest.raises(ValueError, match='at least one group'):
        F.make_groups(ids, np.full(7, -1))
    with pytest.raises(ValueError, match='integer label'):
        F.make_groups(ids, np.zeros(7))


def test_tiled_species_refuses():
    from geonomics_amd.structs.tiled import TiledSpecies
    spp = TiledSpecies.__new__(TiledSpecies)
    for call in (lambda: spp._group_counts(np.zeros(3, int)),
                 lambda: spp._calc_fst(np.zeros(3, int)),
                 lambda: spp._calc_diversity(np.zeros(3, int)),
                 lambda: spp._calc_sfs(np.zeros(3, int))):
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            call()


class _StubSpecies:
    """what the collector's 'fst' statistic asks of a Species: labels and counts"""
    name = 'stub'

    def __init__(self):
        self.fx = fixture()
        self.t = 0
        self.grids = []

    def _labels(self):
        lab = self.fx['labels'].copy()
        if self.t == 1:
            lab[lab == 2] = -1                       # nobody stands in the last rectangle
        return lab

    def _group_by_grid(self, nx, ny):
        self.grids.append((nx, ny))
        return self._labels()

    def _group_counts(self, labels):
        G = int(labels.max()) + 1
        n, c1, ch = counts_numpy(self.fx['genotypes'], labels, G)
        return [*range(G)], n, c1, ch


def test_stats_collector_writes_fst_csv(tmp_path, monkeypatch):
    from geonomics_amd.sim.params import ParametersDict
    from geonomics_amd.sim.stats import _StatsCollector
    monkeypatch.chdir(tmp_path)
    params = ParametersDict({
        'model': {'T': 5, 'stats': {'fst': {'calc': True, 'freq': 2, 'method': 'HsHt',
                                            'grid': (3, 1)}}},
        'comm': {'species': {'stub': {'gen_arch': {}}}}})
    sc = _StatsCollector('m', params)
    assert 'fst' in sc._needs_genome
    spp = _StubSpecies()
    for t in range(5):
        spp.t = t
        sc._calc_stats({0: spp}, t, 0)
    path = tmp_path / 'GNX_mod-m' / 'it-0' / 'spp-stub' / 'mod-m_it-0_spp-stub_FST.csv'
    with open(path) as f:
        rows = [*csv.reader(f)]
    assert rows[0] == ['t', '0-1', '0-2', '1-2']                 # once, from the group names
    assert [r[0] for r in rows[1:]] == ['0', '2', '4']           # freq 2 and the last timestep
    assert spp.grids == [(3, 1)] * 3
    for r in rows[1:]:
        np.testing.assert_array_equal(np.array(r[1:], float), spp.fx['mean_fst'])
    # freq 0: the first and the last timestep; a group nobody stands in gives NaN columns
    params.model.stats.fst.freq = 0
    sc = _StatsCollector('z', params)
    spp = _StubSpecies()
    for t in (0, 1, 4):
        spp.t = 1 if t == 4 else 0
        if t in (0, 4):
            sc._calc_stats({0: spp}, t, 0)
    with open(tmp_path / 'GNX_mod-z' / 'it-0' / 'spp-stub' / 'mod-z_it-0_spp-stub_FST.csv') as f:
        rows = [*csv.reader(f)]
    assert [r[0] for r in rows] == ['t', '0', '4']
    last = np.array(rows[2][1:], float)
    assert last[0] == spp.fx['mean_fst'][0] and np.isnan(last[1:]).all()
    with pytest.raises(ValueError, match="'grid'"):
        from geonomics_amd.sim.stats import _calc_fst
        _calc_fst(spp, grid=(2, 2), lyr=1, edges=[0, 1])
