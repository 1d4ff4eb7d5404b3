"""geonomics_amd/sim/lai.py on the host: the numpy restatement of gnx_lai_paint (brute_paint)
against the sum over all K^L ancestry paths, its invariants and limits, the recovery of a planted
mosaic, the fit of the admixture time, the tracts of the hard calls, and every request check of
Species._calc_local_ancestry on a stand-in whose handle has no calls.  No GPU, no library.

Bounds.  enumerate_paths multiplies L factors per path and adds K^L paths in another order than
the recurrence: gamma within 1e-13 and the log-likelihood within 1e-12 at L = 7 (measured:
1.4e-15 and 8.9e-16).  A row of gamma is K quotients p_k / s of one s = fl(sum p_k): each within
2^-53 of p_k / s, and s and the test's own sum of the row are rounded K - 1 times each; the bar
is 4 2^-53 at every K (measured: at most 3 units at K = 3, 4 at K = 8).  anc_hap adds L_u such rows
left to right per component: relative to their sum L_u that is (L_u - 1) 2^-53 from the adds and
2^-51 from the rows, so |sum_k anc_hap_k - L_u| <= L_u 2^-52 relative to L_u, that is
L_u^2 2^-52 absolute.  (Read as an absolute bound, L_u 2^-52 = 4.4e-14 at L_u = 200 is below
what 3 x 200 roundings of partial sums near 100, half an ulp of 7e-15 each, leave behind:
measured 3.2 L_u 2^-52 = 1.4e-13 on case A, five ulps of 200.)

Recovery on case D (60 individuals, L = 3000, K = 2, 1 Morgan, 10 generations; this generator's
draws from RandomState(3)), measured: 0.9913 of the haplotype-loci called correctly and a mean
|Q_local - true| of 0.0039 under the true priors, 0.9914 and 0.0042 under a uniform prior.  The
profile of the total log-likelihood over gens = 2.5, 5, 10, 20, 40 peaks at 10, 65 log units
above 5 and 98 above 20."""
import inspect
import math
import types

import numpy as np
import pytest

import _lai as CASES
from geonomics_amd.sim import lai as LAI
from geonomics_amd.structs.analyses import SpeciesAnalyses

U53 = 2.0 ** -53
ACCURACY = 0.98          # the bars for case D (measured: the module docstring)
Q_ERROR = 0.01


# ---------------------------------------------------------------- the recurrence
@pytest.mark.parametrize('K', [1, 2, 3])
def test_brute_paint_is_the_sum_over_all_paths(K):
    rng = np.random.RandomState(K)
    n, L = 3, 7
    X = rng.randint(0, 2, (n, L, 2)).astype(np.uint8)
    F = rng.uniform(0.05, 0.95, (L, K))
    Q = rng.dirichlet(np.ones(K), n)
    sw = rng.uniform(0.05, 0.95, L)
    sw[[0, 3]] = 1.0                                            # a break in the middle
    stay = 1.0 - sw
    ref = LAI.brute_paint(X, F, sw, stay, Q, want_gamma=True)
    worst_g = worst_l = 0.0
    for t in range(2 * n):
        g, ll = LAI.enumerate_paths(X[t >> 1, :, t & 1], F, sw, stay, Q[t >> 1])
        worst_g = max(worst_g, float(np.abs(g - ref['gamma'][t]).max()))
        worst_l = max(worst_l, abs(ll - ref['loglik'][t]))
    print('K = %d: gamma %.3g, loglik %.3g from the enumeration' % (K, worst_g, worst_l))
    assert worst_g <= 1e-13 and worst_l <= 1e-12


@pytest.mark.parametrize('case', ['a', 'b1', 'b2', 'b8', 'c'])
def test_invariants_of_the_posteriors(case):
    c = {'a': CASES.case_a, 'c': CASES.case_c}.get(case) or \
        (lambda: CASES.case_b(int(case[1:])))
    c = c()
    ref = c['ref']
    L_u, K = c['F'].shape
    rows = np.abs(ref['gamma'].sum(axis=2) - 1.0).max()
    total = np.abs(ref['anc_hap'].sum(axis=1) - L_u).max()
    print('%s: rows of gamma %.3g units of 2^-53; anc_hap %.3g of L_u^2 2^-52 (%.3g of '
          'L_u 2^-52)' % (c['name'], rows / U53, total / (L_u * L_u * 2 * U53),
                          total / (L_u * 2 * U53)))
    assert rows <= 4 * U53
    assert total <= L_u * (L_u * 2 * U53)
    assert (ref['gamma'] > 0).all() and np.isfinite(ref['loglik']).all()
    assert ref['calls'].max() < K and ref['switches'].max() <= L_u - 1
    np.testing.assert_array_equal(ref['calls'], ref['gamma'].argmax(axis=2))
    # anc_locus adds every painted haplotype once
    lab = np.zeros(c['Q'].shape[0], int) if c['by'] is None else c['by']
    per = 2 * np.bincount(lab[lab >= 0], minlength=max(c['n_groups'], 1))
    np.testing.assert_allclose(ref['anc_locus'].sum(axis=2),
                               np.repeat(per[:, None], L_u, axis=1), rtol=1e-13)


def test_one_ancestry_is_the_bernoulli_product():
    c = CASES.case_b(1)
    ref = c['ref']
    assert (ref['gamma'] == 1.0).all() and (ref['anc_hap'] == 200.0).all()
    assert not ref['calls'].any() and not ref['switches'].any()
    bits = c['X_used'].transpose(0, 2, 1).reshape(140, 200) != 0
    E = np.where(bits, c['F'][:, 0], 1.0 - c['F'][:, 0])
    want = np.array([math.fsum(r) for r in np.log(E).tolist()])
    np.testing.assert_allclose(ref['loglik'], want, rtol=1e-15)


def test_a_very_long_time_gives_the_locus_by_locus_posterior():
    c = CASES.case_a()
    L_u, K = c['F'].shape
    sw, stay = LAI.switch_probs(np.arange(L_u, dtype=np.float64), 1e6)
    assert (sw == 1.0).all() and (stay == 0.0).all()
    got = LAI.brute_paint(c['X_used'], c['F'], sw, stay, c['Q'], want_gamma=True)
    bits = c['X_used'].transpose(0, 2, 1).reshape(140, L_u) != 0
    E = np.where(bits[:, :, None], c['F'][None], 1.0 - c['F'][None])
    post = np.repeat(c['Q'], 2, axis=0)[:, None, :] * E
    post /= post.sum(axis=2, keepdims=True)
    np.testing.assert_allclose(got['gamma'], post, rtol=1e-14)


def test_switch_probs_and_clip_freqs():
    pos = np.array([0.0, 0.01, 0.01, 40.01, 40.02])
    sw, stay = LAI.switch_probs(pos, 10.0)
    np.testing.assert_array_equal(sw, np.r_[1.0, -np.expm1(-10.0 * np.diff(pos))])
    np.testing.assert_array_equal(stay, 1.0 - sw)
    assert sw[0] == 1.0 and stay[0] == 0.0 and sw[2] == 0.0 and sw[3] == 1.0
    for bad in (0.0, -1.0, np.nan, np.inf, True, 'fit'):
        with pytest.raises(ValueError, match='gens'):
            LAI.switch_probs(pos, bad)
    with pytest.raises(ValueError, match='non-decreasing'):
        LAI.switch_probs(pos[::-1], 10.0)
    F = LAI.clip_freqs([[0.0, 0.5, 1.0]], 1e-3)
    np.testing.assert_array_equal(F, [[1e-3, 0.5, 1.0 - 1e-3]])
    for bad in (0.0, 0.5, True):
        with pytest.raises(ValueError, match='eps'):
            LAI.clip_freqs(F, bad)
    with pytest.raises(ValueError, match='finite'):
        LAI.clip_freqs([[np.nan]])
    np.testing.assert_array_equal(LAI.panel_freqs([[0, 3, 6]], [3]),
                                  [[0.5 / 7, 3.5 / 7, 6.5 / 7]])


# ---------------------------------------------------------------- the planted mosaic
def test_recovery_of_the_planted_mosaic():
    d = CASES.case_d()
    acc, dq = CASES.recovery(d['ref'], d['Z'], d['Q'])
    acc_u, dq_u = CASES.recovery(d['ref_uniform'], d['Z'], d['Q'])
    print('true priors: %.4f called correctly, mean |Q_local - true| %.4f; uniform prior: '
          '%.4f, %.4f' % (acc, dq, acc_u, dq_u))
    assert acc >= ACCURACY and dq <= Q_ERROR
    assert acc_u >= ACCURACY


def test_fit_gens_finds_the_planted_time():
    d = CASES.case_d()

    def loglik(g):
        sw, stay = LAI.switch_probs(d['pos'], g)
        return math.fsum(LAI.brute_paint(d['X'], d['F'], sw, stay, d['Q'])['loglik'].tolist())

    gens, trace = LAI.fit_gens(loglik)
    print('fitted gens %.3f after %d evaluations' % (gens, len(trace)))
    assert 5.0 <= gens <= 20.0
    assert all(1.0 <= g <= 1000.0 for g, _ in trace)
    assert max(v for _, v in trace) == dict(trace)[gens]
    # the search itself, on a function whose peak is known
    g, tr = LAI.fit_gens(lambda x: -(math.log(x) - math.log(37.0)) ** 2)
    assert abs(math.log(g / 37.0)) <= 0.01 and len(tr) <= 20
    for bad in (dict(lo=0.0), dict(lo=5.0, hi=5.0), dict(tol=0.0)):
        with pytest.raises(ValueError, match='fit_gens'):
            LAI.fit_gens(loglik, **bad)


def test_calls_to_tracts_on_a_hand_written_string():
    calls = np.array([[0, 0, 1, 1, 1, 0, 0, 0],
                      [2, 2, 2, 2, 2, 2, 2, 2]], np.uint8)
    pos = np.array([0.0, 0.1, 0.2, 0.3, 0.4, 40.4, 40.5, 40.7])
    brk = np.array([1, 0, 0, 0, 0, 1, 0, 0], bool)
    got = LAI.calls_to_tracts(calls, pos, brk, edges=[0.0, 0.15, 1.0])
    np.testing.assert_array_equal(got['tracts'][0], [[0, 1, 0], [2, 4, 1], [5, 7, 0]])
    np.testing.assert_allclose(got['lengths'][0], [0.1, 0.2, 0.3], atol=1e-12)
    # the break cuts the run of equal calls in two
    np.testing.assert_array_equal(got['tracts'][1], [[0, 4, 2], [5, 7, 2]])
    np.testing.assert_array_equal(got['hist']['counts'], [[1, 1], [0, 1], [0, 2]])
    np.testing.assert_allclose(got['hist']['sum_len'], [[0.1, 0.3], [0.0, 0.2], [0.0, 0.7]],
                               atol=1e-12)
    whole = LAI.calls_to_tracts(calls, pos)
    np.testing.assert_array_equal(whole['tracts'][1], [[0, 7, 2]])
    assert whole['hist']['counts'].shape == (3, LAI.TRACT_EDGES.size - 1)
    with pytest.raises(ValueError, match='do not fit'):
        LAI.calls_to_tracts(calls, pos[:-1])


# ---------------------------------------------------------------- the request checks
class _Species(SpeciesAnalyses):
    """four individuals with 8 loci on a handle that has no calls at all: a check that came
    after a device call would fail with AttributeError"""

    def __init__(self, L=8, assigned=True):
        self._dev = types.SimpleNamespace(L=L, W64=16)
        self.gen_arch = None
        if L:
            rec = types.SimpleNamespace(_positions=np.arange(L),
                                        _rates=np.r_[0.0, np.full(L - 1, 0.01)])
            self.gen_arch = types.SimpleNamespace(recombinations=rec,
                                                  neut_loci=np.array([0, 2, 5]))
        if assigned:
            self._genomes_assigned = True

    def __len__(self):
        return 4

    def _geno_sample(self, individs):
        return np.arange(4, dtype=np.int64), np.arange(4, dtype=np.int64)


def _refusal(**kw):
    with pytest.raises(ValueError) as err:
        _Species()._calc_local_ancestry(**kw)
    return str(err.value)


WHO = 'calc_local_ancestry: '
F2 = np.full((2, 8), 0.3)


def test_the_call_refuses_a_species_without_assigned_genomes():
    with pytest.raises(ValueError) as err:
        _Species(L=0)._calc_local_ancestry(F=F2)
    assert str(err.value) == WHO + 'the Species has no genomes (no gen_arch)'
    with pytest.raises(ValueError) as err:
        _Species(assigned=False)._calc_local_ancestry(F=F2)
    assert str(err.value) == WHO + 'genomes are assigned at the end of the burn-in; burn the ' \
        'model in first'


def test_exactly_one_source_gives_the_frequencies():
    msg = WHO + 'exactly one of ancestry, F and panels gives the frequencies (got %s)'
    assert _refusal() == msg % 'none'
    assert _refusal(F=F2, panels=np.array([0, 0, 1, 1])) == msg % 'F, panels'
    assert _refusal(ancestry=dict(F=F2, loci=np.arange(8)), F=F2) == msg % 'ancestry, F'
    assert _refusal(ancestry=dict(F=F2, loci=np.arange(8)), loci=[1]) == \
        WHO + 'ancestry brings its own loci; give no loci'
    assert _refusal(ancestry=dict(Q=1)) == \
        WHO + 'ancestry: the dict calc_ancestry returned (F and loci)'


def test_loci_frequencies_and_panels_are_checked():
    assert _refusal(F=F2, loci='selected') == \
        WHO + "loci: a list of loci, None or 'neutral' (got 'selected')"
    assert _refusal(F=F2[:, :3], loci=[2, 1, 5]) == \
        WHO + 'loci: ascending and distinct (they are the columns of F)'
    assert _refusal(F=F2[:, :2], loci=[2, 8]) == 'loci: a non-empty list of loci in 0..7'
    assert _refusal(F=F2[:, :5]) == \
        WHO + 'F: finite frequencies [K][the 8 loci used] (got (2, 5))'
    assert _refusal(F=F2, loci='neutral') == \
        WHO + 'F: finite frequencies [K][the 3 loci used] (got (2, 8))'
    assert _refusal(F=np.where(np.arange(8) == 3, np.nan, F2)).startswith(
        WHO + 'F: finite frequencies')
    assert _refusal(F=np.full((9, 8), 0.5)) == \
        'K: a number of ancestral populations in 1..8 (got 9)'
    for bad in (0.0, 0.5, True):
        assert _refusal(F=F2, eps=bad) == WHO + 'eps: a number in (0, 0.5) (got %r)' % (bad,)
    msg = WHO + 'panels: one integer label per living individual, in ascending-id order'
    assert _refusal(panels=np.array([0, 1, 1])) == msg
    assert _refusal(panels=np.array([0.0, 1.0, 1.0, 0.0])) == msg
    assert _refusal(panels=np.array([0, -2, 1, 1])) == \
        WHO + 'panels: labels in -1..K-1 (-1: in no panel)'
    assert _refusal(panels=np.array([-1, -1, -1, -1])) == \
        WHO + 'panels: labels in -1..K-1 (-1: in no panel)'
    assert _refusal(panels=np.array([0, 2, 2, -1])) == \
        WHO + 'panels: every panel 0..2 holds at least one individual'
    assert _refusal(panels=np.array([0, 8, 1, 1])) == \
        'K: a number of ancestral populations in 1..8 (got 9)'


def test_gens_prior_by_and_budget_are_checked():
    for bad in (0, -3.0, np.nan, np.inf, True, 'auto'):
        assert _refusal(F=F2, gens=bad) == \
            "gens: a positive finite number of generations, or 'fit' (got %r)" % (bad,)
    assert _refusal(F=F2, prior='flat') == \
        "prior: 'fit', 'uniform' or an array (n, K) (got 'flat')"
    assert _refusal(F=F2, prior=np.full((3, 2), 0.5)) == \
        'prior: an array of shape (3, 2), not (n, K) = (4, 2)'
    for bad in (np.full((4, 2), 0.4), np.tile([1.5, -0.5], (4, 1)), np.full((4, 2), np.nan)):
        assert _refusal(F=F2, prior=bad) == 'prior: rows of probabilities that sum to 1'
    ok = np.full((4, 2), 0.5)
    msg = 'by: one integer label per analysed individual (4 of them)'
    assert _refusal(F=F2, prior=ok, by=[0, 1, 1]) == msg
    assert _refusal(F=F2, prior=ok, by=[0.0, 1.0, 1.0, 0.0]) == msg
    for bad in ([0, 64, 1, 1], [0, -2, 1, 1], [-1, -1, -1, -1]):
        assert _refusal(F=F2, prior=ok, by=bad) == \
            'by: labels in -1..63 (-1: left out), at least one of them >= 0'
    for bad in (0, 1.5, True, -4):
        assert _refusal(F=F2, prior=ok, budget=bad) == \
            WHO + 'budget: a positive number of bytes (got %r)' % (bad,)
    # with every check passed the call goes on to the device: the stand-in has none
    with pytest.raises(AttributeError):
        _Species()._calc_local_ancestry(F=F2, prior=ok)


def test_public_surface():
    from geonomics_amd import _native
    from geonomics_amd.sim.model import Model
    from geonomics_amd.structs.species import Species
    from geonomics_amd.structs.tiled import _NOT_TILED, TiledSpecies
    assert list(inspect.signature(Model.calc_local_ancestry).parameters) == [
        'self', 'spp', 'ancestry', 'F', 'loci', 'panels', 'prior', 'gens', 'individs', 'n',
        'by', 'eps', 'calls', 'budget']
    sig = inspect.signature(Model.calc_local_ancestry).parameters
    assert sig['prior'].default == 'fit' and sig['gens'].default == 10.0
    assert sig['eps'].default == 1e-3 and sig['calls'].default is False
    assert callable(Species._calc_local_ancestry) and '_calc_local_ancestry' in _NOT_TILED
    with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
        TiledSpecies._calc_local_ancestry(object())
    assert 'gnx_lai_paint' in _native.EXPORTS
    assert list(inspect.signature(_native.Device.lai_paint).parameters) == [
        'self', 'F', 'sw', 'stay', 'Q', 'slots', 'loci', 'by', 'n_groups', 'budget', 'want_post',
        'want_calls']
    assert LAI.MAX_K == 8 and LAI.MAX_GROUPS == 64
