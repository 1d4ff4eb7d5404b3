"""Model.calc_local_ancestry on the device (csrc/gnx_lai.hip, sim/lai.py,
Species._calc_local_ancestry): gnx_lai_paint against the numpy restatement
geonomics_amd/sim/lai.brute_paint on the cases of tests/_lai.py, under another byte budget,
repeated, forward only, its refusals, the planted mosaic, and on a walked Model.  Needs an MI355X.

Equality.  The forward and backward recurrences are IEEE fp64 additions, multiplications and
divisions in one stated order on both sides (the build sets -ffp-contract=off, and HIP's fp64
division is correctly rounded), so anc_hap, anc_locus, switches and calls are compared bit for
bit: no tolerance.

The log-likelihood of a haplotype is the sum of ln c_j over the L_u used loci, and the c_j are
the same bits on both sides.  In units of u = 2^-53, to first order, with S = sum_j |ln c_j|
(brute_paint's loglik_abs):
  the device's logarithm (the ROCm device library documents 1 ulp for log in double precision) is
  within 1 ulp <= 2 u |ln c_j| of ln c_j, numpy's (the C library's, below 1 ulp) likewise: 4 u S
  between the terms of the two sides;
  the device adds its terms one after the other in ascending j: L_u - 1 roundings, each of a
  partial sum that is at most S in size (every term has the sign of ln c_j < 0): (L_u - 1) u S;
  the restatement's math.fsum rounds once: u S.
    |ll - ll_ref| <= (L_u + 4) 2^-53 S

Measured on an MI355X, worst |ll - ll_ref| / bound over the haplotypes (the tests print it): A
0.047, B 0.045 (K = 1), 0.060 (K = 2), 0.043 (K = 8), C 0.083, D 0.012 (0.015 under the uniform
prior), the walked Model (n = 284, L = 100) 0.072; everything else the same bits (DESIGN.md
section 24)."""
import ctypes as C
import math

import numpy as np
import pytest

import _lai as CASES
from test_gpu_mmrr import _handle
from test_gpu_parity import native
from geonomics_amd.sim import lai as LAI

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
BITWISE = ('anc_hap', 'anc_locus', 'switches', 'calls')


def _population(nat, D, seed):
    """the dosages D on a handle over a flat 8 x 8 landscape"""
    rng = np.random.RandomState(seed)
    n = D.shape[0]
    return _handle(nat, D, rng.uniform(0, 8, n), rng.uniform(0, 8, n),
                   np.arange(n, dtype=np.int64), np.ones((1, 8, 8)))


@pytest.fixture(scope='module')
def devs():
    """handles holding the genomes of cases A and B ('a'), C ('c') and D ('d': every haplotype of
    the planted mosaic as a homozygous individual)"""
    nat = native()
    out = dict(a=_population(nat, CASES.dosages_a(), 1),
               c=_population(nat, CASES.case_c()['D'], 2),
               d=_population(nat, CASES.as_homozygotes(CASES.case_d()['X']), 3))
    yield nat, out
    for dev in out.values():
        dev.close()


def _paint(dev, c, **kw):
    kw.setdefault('want_calls', kw.get('want_post', True))
    return dev.lai_paint(c['F'], c['sw'], c['stay'], c['Q'], c['slots'], c['loci'], c['by'],
                         c['n_groups'], **kw)


def _same_bits(a, b, label):
    for k in BITWISE:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (label, k)


def _loglik_ratio(got, ref, L_u):
    """worst |ll - ll_ref| / bound over the haplotypes; asserts the bound of the docstring"""
    bound = (L_u + 4) * U53 * ref['loglik_abs']
    err = np.abs(got['loglik'] - ref['loglik'])
    assert np.isfinite(got['loglik']).all() and (err <= bound).all(), float((err / bound).max())
    return float((err / bound).max())


def _case(name):
    return {'a': CASES.case_a, 'c': CASES.case_c}[name]() if name in 'ac' else \
        CASES.case_b(int(name[1:]))


@pytest.mark.parametrize('name', ['a', 'b1', 'b2', 'b8', 'c'])
def test_paint_is_the_restatement_bit_for_bit(devs, name):
    c = _case(name)
    dev = devs[1]['c' if name == 'c' else 'a']
    got = _paint(dev, c)
    ref = c['ref']
    _same_bits(got, ref, c['name'])
    worst = _loglik_ratio(got, ref, c['F'].shape[0])
    assert got['batches'] == 1 and got['kernel_ms'] > 0
    print('%s: n = %d, L_u = %d, K = %d: anc_hap, anc_locus, switches, calls bit-equal; loglik '
          'worst error / bound %.3g; kernels %.3f ms'
          % (c['name'], c['Q'].shape[0], c['F'].shape[0], c['F'].shape[1], worst,
             got['kernel_ms']))
    again = _paint(dev, c)
    _same_bits(again, got, c['name'] + ' repeated')
    assert again['loglik'].tobytes() == got['loglik'].tobytes()


def test_the_budget_changes_no_bit(devs):
    """case A: 140 haplotypes of 200 x 3 x 8 + 2 x 200 bytes each under a budget of 64 of them
    are three batches (64, 64 and 12 haplotypes), under one of 128 two, against the default's
    one; case C (80 haplotypes) likewise"""
    for name in 'ac':
        c = _case(name)
        dev = devs[1][name]
        L_u, K = c['F'].shape
        T = 2 * c['Q'].shape[0]
        per = L_u * K * 8 + 2 * L_u
        one = _paint(dev, c)
        assert one['batches'] == 1
        seen = []
        for budget in (64 * per, 128 * per - 1, 128 * per):
            cut = _paint(dev, c, budget=budget)
            assert cut['batches'] == -(-T // (budget // per // 64 * 64))
            seen.append(cut['batches'])
            _same_bits(cut, one, name)
            assert cut['loglik'].tobytes() == one['loglik'].tobytes()
        assert seen == ([3, 3, 2] if name == 'a' else [2, 2, 1])


def test_forward_only_gives_the_same_loglik_and_writes_nothing_else(devs):
    c = CASES.case_c()
    dev = devs[1]['c']
    full = _paint(dev, c)
    fwd = _paint(dev, c, want_post=False)
    assert fwd['loglik'].tobytes() == full['loglik'].tobytes()
    assert all(fwd[k] is None for k in BITWISE) and fwd['batches'] == 1
    # the entry point itself, over buffers it must leave alone
    n, (L_u, K) = c['Q'].shape[0], c['F'].shape
    ll = np.zeros(2 * n)
    ah = np.full((2 * n, K), 7.0)
    al = np.full((3, L_u, K), 7.0)
    sn = np.full(2 * n, 7, np.int32)
    calls = np.full((2 * n, L_u), 7, np.uint8)
    loci = c['loci'].astype(np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = dev.lib.gnx_lai_paint(
        dev.h, C.c_int64(n), p(c['slots'], C.c_int64), C.c_int32(K), C.c_int32(L_u),
        p(loci, C.c_int32), p(c['F'], C.c_double), p(c['sw'], C.c_double),
        p(c['stay'], C.c_double), p(c['Q'], C.c_double), p(c['by'], C.c_int32), C.c_int32(3),
        C.c_int64(0), C.c_int32(0), C.c_int32(0), p(ll, C.c_double), p(ah, C.c_double),
        p(al, C.c_double), p(sn, C.c_int32), p(calls, C.c_uint8), None, None)
    assert rc == 0 and ll.tobytes() == full['loglik'].tobytes()
    assert (ah == 7.0).all() and (al == 7.0).all() and (sn == 7).all() and (calls == 7).all()


def test_refusals(devs):
    nat, d = devs
    dev = d['c']
    c = CASES.case_c()

    def refused(match, **change):
        k = dict(c, **change)
        with pytest.raises(nat.GnxError, match=match):
            dev.lai_paint(k['F'], k['sw'], k['stay'], k['Q'], k['slots'], k['loci'], k['by'],
                          k['n_groups'], budget=k.get('budget'))

    n = 40
    refused(r'1 <= K <= 8 \(got 9\)', F=np.full((61, 9), 0.5), Q=np.full((n, 9), 1 / 9))
    refused(r'1\.\.2\^30 individuals \(n = 0\)', slots=np.zeros(0, np.int64),
            Q=np.zeros((0, 3)), by=None, n_groups=0)
    refused('cannot hold 64 haplotypes', budget=63 * 61 * 3 * 8)
    down = c['loci'].copy()
    down[[4, 5]] = down[[5, 4]]
    refused(r'loci ascending in 0\.\.199 \(entry 5', loci=down)
    twice = c['loci'].copy()
    twice[9] = twice[8]
    refused(r'loci ascending in 0\.\.199 \(entry 9', loci=twice)
    refused(r'loci ascending in 0\.\.199 \(entry 60: 200\)', loci=np.r_[c['loci'][:-1], 200])
    refused(r'loci ascending in 0\.\.199 \(entry 0: -1\)', loci=np.r_[-1, c['loci'][1:]])
    refused(r'L_u = 61 but the genome has 200 loci', loci=None)
    refused(r'labels in -1\.\.2 \(individual 7: 3\)', by=np.where(np.arange(n) == 7, 3, c['by']))
    refused(r'labels in -1\.\.2 \(individual 0: -2\)', by=np.where(np.arange(n) == 0, -2, c['by']))
    refused(r'0 <= n_groups <= 64 \(got 65\)', n_groups=65)
    refused('budget >= 0', budget=-1)
    refused('slot out of range', slots=np.r_[c['slots'][:-1], 131])
    # the handle is as it was: the case still paints to the same bits
    _same_bits(_paint(dev, c), c['ref'], 'after the refusals')


def test_the_planted_mosaic_is_recovered_on_the_device(devs):
    """case D: each haplotype is a homozygous individual, so haplotype t of the mosaic is
    homologue 0 of individual t; the bars are the host test's"""
    from test_lai_host import ACCURACY, Q_ERROR
    d = CASES.case_d()
    dev = devs[1]['d']
    for prior, ref in ((d['Q'], d['ref']), (np.full(d['Q'].shape, 0.5), d['ref_uniform'])):
        got = dev.lai_paint(d['F'], d['sw'], d['stay'], np.repeat(prior, 2, axis=0),
                            want_calls=True)
        res = dict(calls=got['calls'][0::2], anc_hap=got['anc_hap'][0::2])
        assert got['calls'][1::2].tobytes() == res['calls'].tobytes()
        acc, dq = CASES.recovery(res, d['Z'], d['Q'])
        print('%.4f called correctly, mean |Q_local - true| %.4f, kernels %.2f ms'
              % (acc, dq, got['kernel_ms']))
        assert acc >= ACCURACY
        if prior is d['Q']:
            assert dq <= Q_ERROR
        assert res['anc_hap'].tobytes() == ref['anc_hap'].tobytes()
        assert res['calls'].tobytes() == ref['calls'].tobytes()
        worst = _loglik_ratio(dict(loglik=got['loglik'][0::2]), ref, 3000)
        print('loglik worst error / bound %.3g' % worst)


def _linked_model(seed):
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    p = small_params(seed=seed, L=100)
    p['comm']['species']['spp_0']['gen_arch']['r_distr_alpha'] = 0.02     # linked loci
    mod = gnx.make_model(p)
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(4, 'main', verbose=False)
    return mod


def _halves(mod):
    """(panels by x-half, groups by y-half) of the living in ascending-id order"""
    xy = mod.get_coords()
    return (xy[:, 0] >= 15).astype(np.int64), (xy[:, 1] >= 15).astype(np.int64)


def test_model_calc_local_ancestry_is_the_restatement():
    from geonomics_amd.sim import ld as LD
    from geonomics_amd.structs.analyses import _rec_rates
    mod = _linked_model(11)
    spp = mod.comm[0]
    panels, by = _halves(mod)
    assert panels.min() == 0 and panels.max() == 1 and by.min() == 0 and by.max() == 1
    res = mod.calc_local_ancestry(panels=panels, gens='fit', by=by, calls=True)
    G = mod.get_genotypes(biallelic=True)                      # [n][L][2], ids ascending
    n, L = G.shape[:2]
    np.testing.assert_array_equal(res['ids'], np.array([*spp]))
    np.testing.assert_array_equal(res['loci'], np.arange(L))
    ones = np.stack([G[panels == k].sum(axis=(0, 2)) for k in range(2)]).astype(np.float64)
    n_k = np.bincount(panels, minlength=2).astype(np.float64)
    F = np.clip((ones + 0.5) / (2.0 * n_k[:, None] + 1.0), 1e-3, 1.0 - 1e-3)
    pos = LD.map_positions(_rec_rates(spp))
    sw, stay = LAI.switch_probs(pos, res['gens'])
    Q = res['Q_prior']
    assert Q.shape == (n, 2) and np.abs(Q.sum(axis=1) - 1.0).max() < 1e-12
    ref = LAI.brute_paint(G, F.T, sw, stay, Q, by, 2)
    assert res['K'] == 2 and res['calls'].tobytes() == ref['calls'].tobytes()
    assert res['switches'].tobytes() == ref['switches'].tobytes()
    q_local = 0.5 * (ref['anc_hap'][0::2] + ref['anc_hap'][1::2]) / L
    assert res['Q_local'].tobytes() == q_local.tobytes()
    per = 2.0 * np.bincount(by, minlength=2)
    assert res['anc_locus'].tobytes() == (ref['anc_locus'] / per[:, None, None]).tobytes()
    worst = _loglik_ratio(dict(loglik=res['loglik_hap']), ref, L)
    assert res['loglik'] == math.fsum(res['loglik_hap'].tolist())
    # the fitted time: the best of the evaluations, each the forward pass at that time
    tr = res['gens_trace']
    assert tr.shape[1] == 2 and res['gens'] == tr[np.argmax(tr[:, 1]), 0]
    assert 1.0 <= tr[:, 0].min() and tr[:, 0].max() <= 1000.0
    g0 = float(tr[0, 0])
    s0, t0 = LAI.switch_probs(pos, g0)
    ll0 = LAI.brute_paint(G, F.T, s0, t0, Q)
    assert abs(tr[0, 1] - math.fsum(ll0['loglik'].tolist())) <= \
        (L + 4) * U53 * ll0['loglik_abs'].sum() + U53 * abs(tr[0, 1])
    tracts = res['tracts']
    assert len(tracts['tracts']) == 2 * n
    assert sum(t.shape[0] for t in tracts['tracts']) >= 2 * n + int(res['switches'].sum())
    print('n = %d, L = %d: fitted gens %.3f after %d evaluations, loglik worst error / bound '
          '%.3g, map_len %.3f' % (n, L, res['gens'], tr.shape[0], worst, res['map_len']))
    # a given F and a uniform prior over a sample and some loci
    ids = res['ids'][::3]
    loci = np.arange(5, 90, 2)
    sub = mod.calc_local_ancestry(F=F[:, loci], loci=loci, prior='uniform', gens=7.0,
                                  individs=ids)
    s1, t1 = LAI.switch_probs(pos[loci], 7.0)
    ref1 = LAI.brute_paint(G[::3][:, loci], F[:, loci].T, s1, t1, np.full((ids.size, 2), 0.5))
    assert sub['anc_locus'].tobytes() == (ref1['anc_locus'][0] / (2.0 * ids.size)).tobytes()
    assert sub['switches'].tobytes() == ref1['switches'].tobytes()
    assert 'calls' not in sub and 'gens_trace' not in sub and sub['gens'] == 7.0
    with pytest.raises(ValueError, match='exactly one of ancestry, F and panels'):
        mod.calc_local_ancestry()
    with pytest.raises(ValueError, match='not alive'):
        mod.calc_local_ancestry(F=F, individs=[int(res['ids'][-1]) + 1000])


def test_calc_local_ancestry_leaves_the_model_as_it_was():
    """get_genotypes, get_x and the next walk step: byte-identical with and without the call"""
    a, b = _linked_model(12), _linked_model(12)
    panels, by = _halves(a)
    a.calc_local_ancestry(panels=panels, gens='fit', by=by, calls=True)
    for step in range(2):
        np.testing.assert_array_equal(np.array([*a.comm[0]]), np.array([*b.comm[0]]))
        assert a.get_genotypes(biallelic=True).tobytes() == \
            b.get_genotypes(biallelic=True).tobytes()
        assert a.get_x().tobytes() == b.get_x().tobytes()
        assert a.get_e().tobytes() == b.get_e().tobytes()
        a.walk(1, 'main', verbose=False)
        b.walk(1, 'main', verbose=False)
        if step == 0:
            a.calc_local_ancestry(panels=_halves(a)[0], prior='uniform', gens=5.0)
