"""Model.calc_ancestry on the device (csrc/gnx_admix.hip, sim/ancestry.py,
Species._calc_ancestry): gnx_admix_sweep against the numpy restatement
geonomics_amd/sim/ancestry.brute_sweep (every sum a math.fsum, as include/gnx_hip.h specifies),
against gnx_stats_locus_counts at K = 1, on a walked Model, and the whole fit against the same
driver over the restatement.  Needs an MI355X.

Bounds, in units of 2^-53, to first order (the second-order terms are below 1e-12 of these).
The inputs q, f and g = fl(1 - f) are the same numbers on both sides.
Device (csrc/gnx_admix.hip): p and r are chains of K FMAs over positive terms: K roundings each.
t = fl(1 / fl(p r)) adds two, fl(r t) one more, and r cancels exactly: u = d fl(r t) =
(d / p)(1 + (K + 3) units); d and 2 - d are 0, 1 or 2, so their product is exact; v likewise.  A
term u f_k (v g_k, u q_k, v q_k) enters its sum through an FMA, so the product is not rounded:
every term carries K + 3 units, and a sum of m positive terms in any order adds m - 1.
Restatement: p = fsum(fl(q f)): 2 units; u = fl(d / p): 3; fl(u f): 4; the fsum: 5.
Every output is a sum S of m positive terms, so sum |term| = S:

    |S - S_ref| <= (m + K + 8) 2^-53 S_ref,   m = 2 L_u for A (the terms u f and v g),
                                              m = n for B1 and B0.

The log-likelihood has 2 n L_u terms d ln p and (2 - d) ln r.  ln fl(p) = ln p + (relative error
of p), an absolute error: 2 units in the restatement, so 4 per genotype (d + (2 - d) = 2).  The
device takes one logarithm per genotype: 2 ln r, ln fl(p r) or 2 ln p for d = 0, 1, 2, at most
2 K + 1 units absolute.  Each logarithm is within 1 ulp = 2 units of its own value, at most the
genotype's sum |term|; the products by 1 and 2 are exact; the device's sum in any order adds at
most 2 n L_u units of sum |term|, the fsum one:

    |ll - ll_ref| <= 2^-53 (n L_u (2 K + 5) + (2 n L_u + 4) sum |term|).

Two device calls that differ in the order of their sums (another byte budget) differ by at most
twice the device's share: 2 (m + K + 3) units of S, and 2 (n L_u (2 K + 1) + (2 n L_u + 2) |ll|)
units.
A call repeated is bit-equal in every output.  Unused loci: B is exactly 0, and their F entries
change no output bit.

Measured on an MI355X, worst error / bound (A; B1 and B0; loglik): case A over the sixteen
instances 0.007 - 0.027; 0.029 - 0.092; <= 6e-5.  The boundary state 0.015; 0.037; 0, and with u, v
at 2e6 0.022; 0.037; 4e-5.  Mask and slots 0.072; 0.064; 0.  n = 5: 0.008; 0.25; 0.0015, n = 1:
0.005; 0.33; 0 (m = 1: the bound is a dozen units).  40 of 1031 individuals at L = 1500: 0.001;
0.11; 1e-5.  The walked model (n = 295, L = 4000, two blocks per homologue) 0.015 over all; 0.
Six chunks of n = 1031 against one: the same bits (the stretches of 64 rows are the same).  The
whole fit: 50 plain sweeps end 3.3e-16 from the restatement's Q and F, which itself moves by
5.6e-16 under reversed loci (tolerance 1e-13); the default run takes 558 sweeps to a
log-likelihood of -85746.684 and a recovery of 0.9947 (host: 0.9947 after 574)."""
import numpy as np
import pytest

from test_ancestry_host import PLANTED, RECOVERY
from test_gpu_mmrr import _handle
from test_gpu_parity import native
from geonomics_amd.sim import ancestry as AN
from geonomics_amd.structs.analyses import SpeciesAnalyses

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def _mask_words(dev, used):
    """uint64 [W64] bit mask of the bool mask used [L]"""
    loci = np.flatnonzero(used).astype(np.int64)
    m = np.zeros(dev.W64, np.uint64)
    np.bitwise_or.at(m, loci >> 6, np.uint64(1) << (loci & 63).astype(np.uint64))
    return m


def _state(rng, n, L, K):
    """a random interior state: Dirichlet rows, frequencies in [0.05, 0.95]"""
    return rng.dirichlet(np.ones(K), size=n), rng.uniform(0.05, 0.95, (K, L))


def _call(dev, Q, F, slots=None, used=None, budget=None, want_B=True, want_loglik=True):
    got = dev.admix_sweep(_t(Q), _t(F), slots, None if used is None else _mask_words(dev, used),
                          want_loglik, budget, want_B)
    return {k: (v.cpu().numpy() if hasattr(v, 'cpu') else v) for k, v in got.items()}


def _check(dev, D, Q, F, slots=None, used=None, label=''):
    """one sweep against the restatement within the bounds of the module's docstring, finite,
    zero at unused loci and bit-equal when repeated -> (the call's dict, the restatement's)"""
    Ds = D if slots is None else D[slots]
    n, L = Ds.shape
    K = Q.shape[1]
    ref = AN.brute_sweep(Ds, Q, F, used)
    got = _call(dev, Q, F, slots, used)
    info = dev.admix_info()
    L_u = L if used is None else int(np.count_nonzero(used))
    assert info['instance'] == K and info['launches'] >= 4 and info['chunks'] >= 1, label
    worst = {}
    for k, m in (('A', 2 * L_u), ('B1', n), ('B0', n)):
        assert np.isfinite(got[k]).all(), (label, k)
        err = np.abs(got[k] - ref[k])
        bound = (m + K + 8) * U53 * ref[k]
        assert (err <= bound).all(), (label, k, float(err.max()))
        worst[k] = float((err / np.maximum(bound, 1e-300)).max())
    if used is not None:
        assert not got['B1'][:, ~used].any() and not got['B0'][:, ~used].any(), label
    cells = 2.0 * n * L_u
    b_ll = U53 * (0.5 * cells * (2 * K + 5) + (cells + 4) * ref['loglik_abs'])
    assert np.isfinite(got['loglik']) and abs(got['loglik'] - ref['loglik']) <= b_ll, label
    worst['loglik'] = abs(got['loglik'] - ref['loglik']) / b_ll
    # the identity of the header, on the device's own numbers
    np.testing.assert_allclose((Q * got['A']).sum(axis=1), 2.0 * L_u, rtol=1e-12, err_msg=label)
    print('%s: n = %d, L_u = %d, K = %d, %s: worst error / bound A %.3g, B1 %.3g, B0 %.3g, '
          'loglik %.3g' % (label, n, L_u, K, info, worst['A'], worst['B1'], worst['B0'],
                           worst['loglik']))
    again = _call(dev, Q, F, slots, used)
    for k in ('A', 'B1', 'B0'):
        assert again[k].tobytes() == got[k].tobytes(), (label, k)
    assert again['loglik'] == got['loglik'], label
    return got, ref


def _case_a():
    """131 individuals (two full tiles of 64 and three rows), L = 130 (two words and two bits
    inside 16 padded words); loci 5 and 129 are monomorphic (0 and 2)"""
    rng = np.random.RandomState(19)
    n, L = 131, 130
    D = rng.binomial(2, rng.uniform(0.1, 0.9, L), size=(n, L))
    D[:, 5], D[:, 129] = 0, 2
    return D


@pytest.fixture(scope='module')
def case_a():
    nat = native()
    D = _case_a()
    n = D.shape[0]
    rng = np.random.RandomState(1)
    dev = _handle(nat, D, rng.uniform(0, 24, n), rng.uniform(0, 20, n), np.arange(n),
                  np.ones((1, 20, 24)))
    yield nat, dev, D
    dev.close()


@pytest.mark.parametrize('K', [1, 2, 3, 8, 9, 16])
def test_case_a_one_sweep_from_an_interior_state(case_a, K):
    nat, dev, D = case_a
    Q, F = _state(np.random.RandomState(100 + K), 131, 130, K)
    _check(dev, D, Q, F, label='case A, K = %d' % K)
    if K == 1:
        # f = 1/2 and q = 1: u = 2 d and v = 2 (2 - d) exactly, so B1 = 2 count to the bit
        got = _call(dev, np.ones((131, 1)), np.full((1, 130), 0.5))
        cnt1, _ = dev.stats_locus_counts()
        assert np.array_equal(got['B1'][0], 2.0 * cnt1)
        assert np.array_equal(got['B1'][0] / (got['B1'][0] + got['B0'][0]), cnt1 / (2.0 * 131))
        assert (got['A'] == 2.0 * 130).all()


@pytest.mark.parametrize('K', [4, 5, 6, 7, 10, 11, 12, 13, 14, 15])
def test_case_a_the_other_template_instances(case_a, K):
    """K is the template parameter: with the six above every instance has run"""
    nat, dev, D = case_a
    Q, F = _state(np.random.RandomState(100 + K), 131, 130, K)
    _check(dev, D, Q, F, label='case A, K = %d' % K)


def test_a_state_on_the_boundary(case_a):
    """after 200 restatement sweeps of the accelerated fit of case A with K = 3, 46 f sit at eps
    or 1 - eps and 24 q at eps; with the frequencies of the two monomorphic loci exchanged p or r
    is 1e-6 where the data say otherwise, and u and v reach 2e6: nothing overflows"""
    nat, dev, D = case_a
    res = AN.fit(AN.host_sweep(D), 131, 130, 3, init='random', seed=7, tol=0.0, max_sweeps=200)
    Q, F = res['Q'], res['F']
    at_f = int(((F == AN.EPS) | (F == 1 - AN.EPS)).sum())
    at_q = int((Q < 1.001 * AN.EPS).sum())
    print('boundary state: %d of %d f at a bound, %d of %d q at eps' % (at_f, F.size, at_q,
                                                                        Q.size))
    assert at_f >= 10 and at_q >= 10
    assert (F[:, 5] == AN.EPS).all() and (F[:, 129] == 1 - AN.EPS).all()
    _check(dev, D, Q, F, label='boundary state')
    F2 = F.copy()
    F2[:, 5], F2[:, 129] = F[:, 129], F[:, 5]
    got, ref = _check(dev, D, Q, F2, label='boundary state, against the data')
    assert got['B0'][:, 5].sum() > 1.9e6 * 131 and got['B1'][:, 129].sum() > 1.9e6 * 131


def test_masks_and_slots(case_a):
    nat, dev, D = case_a
    rng = np.random.RandomState(5)
    used = np.zeros(130, bool)
    used[:64] = rng.rand(64) < 0.6                 # parts of word 0
    used[[0, 5, 63]] = True                        # its first and last bit, a monomorphic locus
    used[128] = True                               # a part of word 2; word 1 is empty
    assert not used[64:128].any() and not used[129] and 20 < used.sum() < 64
    slots = rng.permutation(131)[:70].astype(np.int64)
    assert (np.diff(slots) < 0).any()
    Q, F = _state(rng, 70, 130, 3)
    got, ref = _check(dev, D, Q, F, slots, used, label='mask and slots')
    # the F of a masked-out locus is never part of a result: any value, the same bits
    F2 = F.copy()
    F2[:, ~used] = rng.choice([AN.EPS, 0.3, 1 - AN.EPS], size=(3, int((~used).sum())))
    other = _call(dev, Q, F2, slots, used)
    for k in ('A', 'B1', 'B0'):
        assert other[k].tobytes() == got[k].tobytes(), k
    assert other['loglik'] == got['loglik']
    # every locus through an all-ones mask is the unmasked call
    full = _call(dev, Q, F, slots, np.ones(130, bool))
    none = _call(dev, Q, F, slots)
    assert all(full[k].tobytes() == none[k].tobytes() for k in ('A', 'B1', 'B0'))
    # without B and without the log-likelihood: the same A
    only = _call(dev, Q, F, slots, used, want_B=False, want_loglik=False)
    assert only['B1'] is None and only['B0'] is None and only['loglik'] is None
    assert only['A'].tobytes() == got['A'].tobytes()


def test_fewer_individuals_than_one_tile():
    nat = native()
    rng = np.random.RandomState(6)
    D = rng.randint(0, 3, size=(5, 130))
    dev = _handle(nat, D, rng.uniform(0, 24, 5), rng.uniform(0, 20, 5), np.arange(5),
                  np.ones((1, 20, 24)))
    try:
        Q, F = _state(rng, 5, 130, 2)
        _check(dev, D, Q, F, label='n = 5')
        _check(dev, D, Q[:1], F, np.array([3], np.int64), label='n = 1')
    finally:
        dev.close()


def test_chunks_over_the_individuals_under_a_byte_budget():
    """n = 1031 (17 tiles), L = 1500 (24 words), K = 3: the default budget takes the sample in
    one chunk; 600 000 bytes of partial sums force chunks of three tiles"""
    nat = native()
    rng = np.random.RandomState(31)
    n, L, K = 1031, 1500, 3
    D = rng.binomial(2, rng.uniform(0.05, 0.95, L), size=(n, L))
    dev = _handle(nat, D, rng.uniform(0, 30, n), rng.uniform(0, 30, n), np.arange(n),
                  np.ones((1, 30, 30)))
    try:
        Q, F = _state(rng, n, L, K)
        whole = _call(dev, Q, F)
        assert dev.admix_info()['chunks'] == 1
        cut = _call(dev, Q, F, budget=600000)
        info = dev.admix_info()
        print('chunked: %s' % (info,))
        assert info['chunks'] >= 3 and info['instance'] == 3
        worst = 0.0
        for k, m in (('A', 2 * L), ('B1', n), ('B0', n)):
            err = np.abs(cut[k] - whole[k])
            bound = 2 * (m + K + 3) * U53 * whole[k]
            assert (err <= bound).all(), k
            worst = max(worst, float((err / bound).max()))
        cells = 2.0 * n * L
        b_ll = 2 * U53 * (0.5 * cells * (2 * K + 1) +
                          (cells + 2) * abs(whole['loglik']) * (1 + 1e-9))
        assert abs(cut['loglik'] - whole['loglik']) <= b_ll
        print('chunked against whole: worst difference / bound %.3g, loglik %.3g'
              % (worst, abs(cut['loglik'] - whole['loglik']) / b_ll))
        np.testing.assert_allclose((Q * cut['A']).sum(axis=1), 2.0 * L, rtol=1e-12)
        for budget, first in ((None, whole), (600000, cut)):
            again = _call(dev, Q, F, budget=budget)
            for k in ('A', 'B1', 'B0'):
                assert again[k].tobytes() == first[k].tobytes(), (budget, k)
            assert again['loglik'] == first['loglik']
        # projection under the budget: A alone (its partial sums are smaller: other chunks)
        only = _call(dev, Q, F, budget=600000, want_B=False)
        assert only['B1'] is None and dev.admix_info()['chunks'] >= 2
        assert (np.abs(only['A'] - whole['A']) <= 2 * (2 * L + K + 3) * U53 * whole['A']).all()
        # a spot check of the big case against the restatement: 40 individuals, all loci
        rows = rng.choice(n, 40, replace=False).astype(np.int64)
        _check(dev, D, Q[rows], F, rows, label='40 of 1031')
    finally:
        dev.close()


def _admix_params(seed):
    from test_gpu_model_api import small_params
    p = small_params(seed=seed, L=4000, T=12)
    # sparse recombination: two crossovers a gamete, two blocks per homologue
    p['comm']['species']['spp_0']['gen_arch']['r_distr_alpha'] = 0.0005
    return p


def _walked(seed, sweep):
    """a Model walked 5 steps, optionally swept once, walked one more step
    -> (ids, genotypes before the last step, ids and genotypes after it, what sweep returned)"""
    import geonomics_amd as gnx
    mod = gnx.make_model(_admix_params(seed))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(5, 'main', verbose=False)
    out = sweep(mod) if sweep else None
    ids, gts = np.array([*mod.comm[0]]), mod.get_genotypes(biallelic=True)
    mod.walk(1, 'main', verbose=False)
    return ids, gts, np.array([*mod.comm[0]]), mod.get_genotypes(biallelic=True), out


def test_a_walked_model_is_read_through_its_block_table_and_left_unchanged():
    """genomes that went through the deferred crossover, in blocks that parents and offspring
    share; the call joins the pending crossover and changes nothing"""
    rng = np.random.RandomState(3)
    seen = {}

    def sweep(mod):
        spp = mod.comm[0]
        before = mod.get_genotypes(biallelic=True)
        ids, slots = spp._geno_sample(None)
        Q, F = _state(rng, ids.size, 4000, 2)
        got = _call(spp._dev, Q, F, slots)
        seen.update(Q=Q, F=F, blocks=spp._dev.blocks_per_hom)
        assert np.array_equal(mod.get_genotypes(biallelic=True), before)
        return got

    ids, gts, ids1, gts1, got = _walked(8, sweep)
    D = gts.sum(axis=2)
    n, L, K = D.shape[0], 4000, 2
    assert n > 100 and 0 < D.mean() < 2 and seen['blocks'] == 2
    ref = AN.brute_sweep(D, seen['Q'], seen['F'])
    worst = 0.0
    for k, m in (('A', 2 * L), ('B1', n), ('B0', n)):
        err, bound = np.abs(got[k] - ref[k]), (m + K + 8) * U53 * ref[k]
        assert (err <= bound).all(), k
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    cells = 2.0 * n * L
    b_ll = U53 * (0.5 * cells * (2 * K + 5) + (cells + 4) * ref['loglik_abs'])
    assert abs(got['loglik'] - ref['loglik']) <= b_ll
    print('walked model: n = %d, %d blocks per homologue: worst error / bound %.3g, loglik %.3g'
          % (n, seen['blocks'], worst, abs(got['loglik'] - ref['loglik']) / b_ll))
    # the twin that made no call: the same population before and after the next step
    t_ids, t_gts, t_ids1, t_gts1, _ = _walked(8, None)
    assert np.array_equal(t_ids, ids) and np.array_equal(t_gts, gts)
    assert np.array_equal(t_ids1, ids1) and np.array_equal(t_gts1, gts1)


class _Arch:
    neut_loci = np.arange(0, PLANTED['L'], 3)


class _Spp(SpeciesAnalyses):
    """a Species' analysis methods over a Device that holds an uploaded sample"""
    gen_arch = _Arch()

    def __init__(self, dev):
        self._dev = dev
        self._genomes_assigned = True
        self._rng = np.random.RandomState(0)

    def __len__(self):
        return int(self._dev.N)


class _Mod:
    def __init__(self, spp):
        self.comm = [spp]
        self._rng = spp._rng

    def _get_spp_num(self, spp):
        return spp


def _model_over(dev):
    from geonomics_amd.sim.model import Model
    from geonomics_amd.structs.species import Species
    _Spp._field = Species._field
    for name in ('calc_ancestry', '_test_sample'):
        setattr(_Mod, name, getattr(Model, name))
    return _Mod(_Spp(dev))


def test_the_whole_fit_on_the_planted_case():
    """Model.calc_ancestry on the planted host case: 50 plain sweeps from given arrays against the
    same driver over brute_sweep, then the accelerated default run"""
    nat = native()
    D, Qt, Ft = AN.planted_case(**PLANTED)
    n, L, K = D.shape[0], D.shape[1], PLANTED['K']
    rng = np.random.RandomState(2)
    ids = np.sort(rng.choice(10 ** 5, n, replace=False))
    order = rng.permutation(n)                                 # slots are not in id order
    dev = _handle(nat, D[order], rng.uniform(0, 24, n), rng.uniform(0, 20, n), ids[order],
                  np.ones((1, 20, 24)))
    try:
        mod = _model_over(dev)
        init = AN.init_random(n, L, K, seed=11)
        kw = dict(init=init, accelerate=False, tol=0.0, max_sweeps=50)
        got = mod.calc_ancestry(K, **kw)
        ref = AN.fit(AN.host_sweep(D, exact=True), n, L, K, **kw)
        # the restatement's own sensitivity to the order of its sums: the loci reversed
        fwd = AN.fit(AN.host_sweep(D), n, L, K, **kw)
        rev = AN.fit(AN.host_sweep(D[:, ::-1]), n, L, K, init=(init[0], init[1][:, ::-1]),
                     accelerate=False, tol=0.0, max_sweeps=50)
        own = max(np.abs(fwd['Q'] - rev['Q']).max(), np.abs(fwd['F'] - rev['F'][:, ::-1]).max())
        tol = max(16.0 * own, 1e-13)
        dq, df = np.abs(got['Q'] - ref['Q']).max(), np.abs(got['F'] - ref['F']).max()
        print('50 plain sweeps: the restatement moves by %.3g under reversed loci (tolerance '
              '%.3g); device against restatement: Q %.3g, F %.3g, loglik %.17g against %.17g'
              % (own, tol, dq, df, got['loglik'][-1], ref['loglik'][-1]))
        assert got['n_sweeps'] == ref['n_sweeps'] == 50 and not got['converged']
        assert np.array_equal(got['individs'], ids) and np.array_equal(got['loci'], np.arange(L))
        assert dq <= tol and df <= tol
        np.testing.assert_allclose(got['loglik'], ref['loglik'], rtol=1e-12)
        assert got['n_params'] == ref['n_params'] and got['aic'] == pytest.approx(ref['aic'])
        # ---- the accelerated default run (init='pca' from the device's exact PCs)
        res = mod.calc_ancestry(K)
        corr, match = AN.match_components(res['Q'], Qt)
        print('default run: %d sweeps, converged %s, loglik %.3f, recovery %.4f (host: %.4f)'
              % (res['n_sweeps'], res['converged'], res['loglik'][-1], corr, RECOVERY))
        assert res['converged']
        assert (np.diff(res['loglik']) >= -1e-9 * np.abs(res['loglik'][:-1])).all()
        assert res['loglik'][-1] >= got['loglik'][-1]
        assert abs(corr - RECOVERY) <= 0.005
        assert (np.diff(res['Q'].mean(axis=0)) <= 0).all()
        # ---- projection of everybody onto the fitted frequencies, and a sample of the loci
        proj = mod.calc_ancestry(K, fixed_F=res['F'], init='random', seed=4)
        assert proj['converged'] and np.abs(proj['Q'] - res['Q']).max() < 0.02
        assert np.array_equal(proj['F'], res['F']) and proj['n_params'] == n * (K - 1)
        sub = mod.calc_ancestry(2, individs=ids[::2], loci='neutral', init='random', seed=1,
                                max_sweeps=30)
        assert sub['Q'].shape == (n // 2, 2) and sub['F'].shape == (2, L // 3)
        assert np.array_equal(sub['loci'], np.arange(0, L, 3))
        assert np.array_equal(sub['individs'], ids[::2])
        for bad in (0, 17):
            with pytest.raises(ValueError, match='K'):
                mod.calc_ancestry(bad)
        with pytest.raises(ValueError, match='loci'):
            mod.calc_ancestry(2, loci='selected')
    finally:
        dev.close()


def test_refusals_come_before_any_launch(case_a):
    nat, dev, D = case_a
    import torch
    Q, F = _state(np.random.RandomState(0), 131, 130, 3)
    before = _call(dev, Q, F)
    assert dev.admix_info()['launches'] > 0

    def refused(match, Q, F, *a, **kw):
        with pytest.raises(nat.GnxError, match=match):
            dev.admix_sweep(Q, F, *a, **kw)
        info = dev.admix_info()
        assert info['launches'] == 0 and info['chunks'] == 0 and info['instance'] == 0

    z = lambda *s: torch.full(s, 0.5, dtype=torch.float64, device='cuda')
    refused('1 <= K <= 16', z(131, 0), z(0, 130))
    refused('1 <= K <= 16', z(131, 17), z(17, 130))
    refused('locus mask is empty', _t(Q), _t(F), None, np.zeros(dev.W64, np.uint64))
    pad = np.zeros(dev.W64, np.uint64)
    pad[2] = np.uint64(0xfffffffffffffffc)                    # only bits past L = 130
    pad[3:] = np.uint64(0xffffffffffffffff)
    refused('locus mask is empty', _t(Q), _t(F), None, pad)
    refused('slot out of range', _t(Q[:2]), _t(F), np.array([0, dev.N]))
    refused('slot out of range', _t(Q[:2]), _t(F), np.array([-1, 3]))
    refused('at least one individual', z(0, 3), _t(F), np.zeros(0, np.int64))
    refused('budget >= 0', _t(Q), _t(F), None, None, True, -1)
    with pytest.raises(ValueError, match='rows'):
        dev.admix_sweep(_t(Q[:100]), _t(F))
    with pytest.raises(ValueError, match='F'):
        dev.admix_sweep(_t(Q), _t(F[:, :100]))
    with pytest.raises(ValueError, match='device'):
        dev.admix_sweep(torch.as_tensor(Q), _t(F))
    after = _call(dev, Q, F)
    assert all(after[k].tobytes() == before[k].tobytes() for k in ('A', 'B1', 'B0'))
    empty = nat.Device(16, 16, 1, L=96, cap_inds=256, cap_rows=256, seed=1)
    empty.upload_rasters(np.ones((1, 16, 16), np.float32))
    empty.set_species_params(nat.default_species_params())
    empty.upload_population(np.ones(10), np.ones(10), np.zeros(10), np.zeros(10), np.arange(10))
    with pytest.raises(nat.GnxError, match='genomes not assigned'):
        empty.admix_sweep(z(10, 2), z(2, 96))
    assert empty.admix_info()['launches'] == 0
    empty.close()
    tile = _handle(nat, D[:10], np.ones(10), np.ones(10), np.arange(10), np.ones((1, 20, 24)))
    tile.admix_sweep(z(10, 2), z(2, 130))
    assert tile.admix_info()['launches'] > 0                  # (so that the 0 below says something)
    rec = np.zeros(1, nat.IND_REC)
    rec['x'], rec['y'], rec['id'] = 1.0, 1.0, 10 ** 6
    tile.tile_import_ghosts(rec)
    with pytest.raises(nat.GnxError, match='ghost records'):
        tile.admix_sweep(z(10, 2), z(2, 130), np.arange(10, dtype=np.int64))
    assert tile.admix_info()['launches'] == 0
    tile.close()
