"""geonomics_amd/sim/ancestry.py on the host: the numpy restatement of gnx_admix_sweep
(brute_sweep) against a 3 x 4 example worked by hand and in rational arithmetic, the closed form
at K = 1, the identity sum_k q_ik A_ik = 2 L_u, the EM's monotone log-likelihood, the recovery of
a planted structure by the accelerated fit, projection onto held frequencies, and the driver's
ordering, bookkeeping and refusals.  No GPU.

Recorded on the planted case (planted_case(200, 450, 3, 0.2, seed=1); init='pca' from the exact
PCs, signs by their loadings): the accelerated fit converges at tol = 1e-4 after 574 sweeps to a
log-likelihood of -85746.682 with a mean per-component correlation with the true Q of 0.9947 after
label matching (with the PCs' signs taken from the scores: 266 sweeps, 0.9947; seeds 2, 3, 22 of
the case then give 0.9941, 0.9930, 0.9937 after 254, 346, 310 sweeps).  Plain EM from a random
start needs 1151 sweeps for the same log-likelihood, the accelerated fit from that start 493.
The test asserts RECOVERY - 0.01."""
import inspect
from fractions import Fraction

import numpy as np
import pytest

from geonomics_amd.sim import ancestry as AN
from geonomics_amd.sim import pca as PCA

RECOVERY = 0.9947          # see the module docstring; tests/test_gpu_ancestry.py compares with it
PLANTED = dict(n=200, L=450, K=3, fst=0.2, seed=1)


def exact_pcs(D, k):
    """the first k genetic PCs from the exact Gram matrix, as Species._calc_genetic_PCA"""
    Dd = np.asarray(D, np.int64)
    return PCA.pca_from_gram(Dd @ Dd.T, k, rmatmul=lambda U: Dd.T @ U)[0]


def planted():
    return AN.planted_case(**PLANTED)


def column_corr(Qa, Qb):
    return float(np.mean([np.corrcoef(Qa[:, k], Qb[:, k])[0, 1] for k in range(Qa.shape[1])]))


# ---------------------------------------------------------------- the restatement
def _rational_sweep(D, Q, F, used):
    """the header's sums in rational arithmetic (inputs dyadic: exact)"""
    n, L = len(D), len(D[0])
    K = len(Q[0])
    A = [[Fraction(0)] * K for _ in range(n)]
    B1 = [[Fraction(0)] * L for _ in range(K)]
    B0 = [[Fraction(0)] * L for _ in range(K)]
    for i in range(n):
        for l in used:
            p = sum(Q[i][k] * F[k][l] for k in range(K))
            r = sum(Q[i][k] * (1 - F[k][l]) for k in range(K))
            u, v = Fraction(D[i][l]) / p, Fraction(2 - D[i][l]) / r
            for k in range(K):
                A[i][k] += u * F[k][l] + v * (1 - F[k][l])
                B1[k][l] += u * Q[i][k]
                B0[k][l] += v * Q[i][k]
    return A, B1, B0


def test_brute_sweep_matches_a_3_by_4_example_worked_by_hand():
    h, q, t = Fraction(1, 2), Fraction(1, 4), Fraction(3, 4)
    D = [[0, 1, 2, 1], [2, 0, 1, 1], [1, 2, 0, 2]]
    Q = [[h, h], [q, t], [t, q]]
    F = [[h, q, t, h], [h, t, q, q]]
    f64 = lambda M: np.array([[float(x) for x in row] for row in M])
    got = AN.brute_sweep(np.array(D), f64(Q), f64(F))
    # individual 0 by hand: p = (1/2, 1/2, 1/2, 3/8), r = (1/2, 1/2, 1/2, 5/8),
    # u = (0, 2, 4, 8/3), v = (4, 2, 0, 8/5)
    #   A[0][0] = 2 + 2 + 3 + (4/3 + 4/5) = 137/15,  A[0][1] = 2 + 2 + 1 + (2/3 + 6/5) = 103/15
    #   log-likelihood of its row: ln(1/2) (0 + 2 + 1 + 1 + 2 + 0) + ln(3/8) + ln(5/8)
    assert got['A'][0, 0] == pytest.approx(137 / 15, rel=4e-16)
    assert got['A'][0, 1] == pytest.approx(103 / 15, rel=4e-16)
    # locus 3 by hand: p = (3/8, 5/16, 7/16), u = d / p = (8/3, 16/5, 32/7),
    #   B1[0][3] = 8/3 1/2 + 16/5 1/4 + 32/7 3/4 = 4/3 + 4/5 + 24/7 = 584/105
    assert got['B1'][0, 3] == pytest.approx(584 / 105, rel=4e-16)
    A, B1, B0 = _rational_sweep(D, Q, F, range(4))
    np.testing.assert_allclose(got['A'], f64(A), rtol=1e-15, atol=0)
    np.testing.assert_allclose(got['B1'], f64(B1), rtol=1e-15, atol=0)
    np.testing.assert_allclose(got['B0'], f64(B0), rtol=1e-15, atol=0)
    ll = sum(d * np.log(float(sum(Q[i][k] * F[k][l] for k in range(2)))) +
             (2 - d) * np.log(float(sum(Q[i][k] * (1 - F[k][l]) for k in range(2))))
             for i, row in enumerate(D) for l, d in enumerate(row))
    assert got['loglik'] == pytest.approx(ll, rel=1e-14)
    # a mask: loci 0 and 3 only; the B of unused loci is exactly 0 and their F is never read
    Fm = f64(F)
    Fm[:, 1:3] = np.nan
    part = AN.brute_sweep(np.array(D), f64(Q), Fm, [3, 0])
    A2, B12, _ = _rational_sweep(D, Q, F, (0, 3))
    np.testing.assert_allclose(part['A'], f64(A2), rtol=1e-15, atol=0)
    assert not part['B1'][:, 1:3].any() and not part['B0'][:, 1:3].any()
    np.testing.assert_allclose(part['B1'][:, [0, 3]], f64(B12)[:, [0, 3]], rtol=1e-15, atol=0)
    same = AN.brute_sweep(np.array(D), f64(Q), Fm, np.array([True, False, False, True]))
    assert all(np.array_equal(same[k], part[k]) for k in ('A', 'B1', 'B0'))
    # the fast sums agree with the exact ones
    fast = AN.brute_sweep(np.array(D), f64(Q), f64(F), exact=False)
    for k in ('A', 'B1', 'B0'):
        np.testing.assert_allclose(fast[k], got[k], rtol=1e-14, atol=0)


def test_one_population_has_the_closed_form():
    rng = np.random.RandomState(4)
    n, L = 37, 50
    D = rng.binomial(2, rng.uniform(0.05, 0.95, L), size=(n, L))
    D[:, 7], D[:, 11] = 0, 2
    Q, F = np.ones((n, 1)), np.full((1, L), 0.5)
    got = AN.brute_sweep(D, Q, F)
    assert (got['A'] == 2.0 * L).all()
    Qn, Fn = AN.em_update(Q, F, got['A'], got['B1'], got['B0'], L)
    assert (Qn == 1.0).all()
    count = D.sum(axis=0)
    assert np.array_equal(Fn[0], np.clip(count / (2.0 * n), AN.EPS, 1.0 - AN.EPS))
    assert Fn[0, 7] == AN.EPS and Fn[0, 11] == 1.0 - AN.EPS
    # and that is where the fit stays
    res = AN.fit(AN.host_sweep(D, exact=True), n, L, 1, init='random', seed=0, accelerate=False)
    assert res['converged'] and np.allclose(res['F'][0], Fn[0], rtol=1e-12, atol=0)
    assert (res['Q'] == 1.0).all() and res['n_params'] == L


def test_the_numerators_of_q_sum_to_two_per_locus():
    """sum_k q_ik A_ik = sum_l (u p + v r) = sum_l (d + 2 - d) = 2 L_u for any valid input"""
    rng = np.random.RandomState(9)
    for n, L, K in ((31, 47, 2), (20, 33, 5), (9, 21, 16)):
        D = rng.randint(0, 3, size=(n, L))
        Q = rng.dirichlet(np.ones(K), size=n) * rng.uniform(0.5, 2.0, (n, 1))   # rows positive
        F = rng.uniform(AN.EPS, 1 - AN.EPS, (K, L))
        F[:, :5] = rng.choice([AN.EPS, 1 - AN.EPS], size=(K, 5))
        used = rng.rand(L) < 0.7
        got = AN.brute_sweep(D, Q, F, used)
        np.testing.assert_allclose((Q * got['A']).sum(axis=1), 2.0 * used.sum(), rtol=1e-13)
        # the frequency numerators obey theirs: sum_k f B1 + g B0 = sum_i (u p + v r) = 2 n
        tot = (F * got['B1'] + (1.0 - F) * got['B0']).sum(axis=0)
        np.testing.assert_allclose(tot[used], 2.0 * n, rtol=1e-13)
        assert not tot[~used].any()


def test_plain_em_never_lowers_the_log_likelihood():
    rng = np.random.RandomState(12)
    n, L, K = 40, 60, 3
    D = rng.binomial(2, rng.uniform(0.05, 0.95, L), size=(n, L))
    res = AN.fit(AN.host_sweep(D, exact=True), n, L, K, init='random', seed=5, accelerate=False,
                 tol=0.0, max_sweeps=120)
    ll = res['loglik']
    assert ll.size == 120 == res['n_sweeps'] and not res['converged']
    assert (np.diff(ll) >= -1e-12 * np.abs(ll[:-1])).all()
    assert ll[-1] > ll[0] + 10.0


@pytest.fixture(scope='module')
def planted_fit():
    D, Qt, Ft = planted()
    res = AN.fit(AN.host_sweep(D), D.shape[0], D.shape[1], PLANTED['K'], init='pca',
                 pcs=exact_pcs(D, PLANTED['K'] - 1))
    return D, Qt, Ft, res


def test_the_accelerated_fit_recovers_a_planted_structure(planted_fit):
    D, Qt, Ft, res = planted_fit
    corr, match = AN.match_components(res['Q'], Qt)
    print('planted case: %d sweeps, converged %s, loglik %.3f, recovery %.4f'
          % (res['n_sweeps'], res['converged'], res['loglik'][-1], corr))
    assert res['converged'] and res['n_sweeps'] < 1151
    assert (np.diff(res['loglik']) >= -1e-9).all()
    assert corr >= max(RECOVERY - 0.01, 0.95)
    # the frequencies too, under the same matching
    assert column_corr(res['F'][match].T, Ft.T) > 0.9
    # at least as likely as what a long plain EM run reaches from the same start
    plain = AN.fit(AN.host_sweep(D), D.shape[0], D.shape[1], 3, init='pca',
                   pcs=exact_pcs(D, 2), accelerate=False, max_sweeps=res['n_sweeps'])
    assert res['loglik'][-1] >= plain['loglik'][-1] - 1e-6


def test_projection_on_held_frequencies_recovers_held_out_individuals():
    D, Qt, Ft = AN.planted_case(260, 450, 3, 0.2, seed=5)
    joint = AN.fit(AN.host_sweep(D), 260, 450, 3, init='pca', pcs=exact_pcs(D, 2))
    _, match = AN.match_components(joint['Q'], Qt)
    held = np.random.RandomState(0).choice(260, 60, replace=False)
    proj = AN.fit(AN.host_sweep(D[held]), 60, 450, 3, init='random', seed=1, fixed_F=Ft)
    c_joint = column_corr(joint['Q'][:, match][held], Qt[held])
    c_proj = column_corr(proj['Q'], Qt[held])              # (fixed_F keeps its order)
    print('held-out individuals: joint fit %.4f, projection on the true F %.4f'
          % (c_joint, c_proj))
    assert proj['converged'] and c_proj >= c_joint
    assert np.array_equal(proj['F'], np.clip(Ft, AN.EPS, 1 - AN.EPS))
    assert proj['n_params'] == 60 * 2
    assert (np.diff(proj['loglik']) >= -1e-9).all()


def test_order_of_components_bookkeeping_and_refusals(planted_fit):
    D, Qt, Ft, res = planted_fit
    n, L, K = D.shape[0], D.shape[1], 3
    m = res['Q'].mean(axis=0)
    assert (np.diff(m) <= 0).all()
    assert res['Q'].shape == (n, K) and res['F'].shape == (K, L)
    np.testing.assert_allclose(res['Q'].sum(axis=1), 1.0, rtol=1e-12)
    assert res['Q'].min() >= AN.EPS * 0.99 and AN.EPS <= res['F'].min() \
        and res['F'].max() <= 1 - AN.EPS
    # the labels of the start do not matter: the same fit from a relabelled start
    Q0, F0 = AN.init_random(n, L, K, seed=8)
    a = AN.fit(AN.host_sweep(D), n, L, K, init=(Q0, F0), max_sweeps=40, accelerate=False)
    b = AN.fit(AN.host_sweep(D), n, L, K, init=(Q0[:, [2, 0, 1]], F0[[2, 0, 1]]), max_sweeps=40,
               accelerate=False)
    np.testing.assert_allclose(a['Q'], b['Q'], rtol=0, atol=1e-10)
    np.testing.assert_allclose(a['F'], b['F'], rtol=0, atol=1e-10)
    assert a['n_sweeps'] == 40 and a['loglik'].size == 40 and not a['converged']
    ll = res['loglik'][-1]
    assert res['n_params'] == n * (K - 1) + K * L
    assert res['aic'] == 2.0 * res['n_params'] - 2.0 * ll
    assert res['bic'] == res['n_params'] * np.log(n * L) - 2.0 * ll
    sw = AN.host_sweep(D)
    for bad in (0, 17, 2.5, True):
        with pytest.raises(ValueError, match='K'):
            AN.fit(sw, n, L, bad)
    for init in ((Q0[:-1], F0), (Q0, F0[:, :-1]), (Q0, F0.T), (Q0, np.where(F0 > 0.5, 1.0, F0)),
                 (Q0, -F0), (np.where(Q0 > 0.5, 0.0, Q0), F0), (Q0 * np.nan, F0), 'kmeans',
                 (Q0,)):
        with pytest.raises(ValueError, match='init'):
            AN.fit(sw, n, L, K, init=init)
    with pytest.raises(ValueError, match='pcs'):
        AN.fit(sw, n, L, K, init='pca')
    with pytest.raises(ValueError, match='fixed_F'):
        AN.fit(sw, n, L, K, fixed_F=F0[:2])
    with pytest.raises(ValueError, match='max_sweeps'):
        AN.fit(sw, n, L, K, max_sweeps=0)


def test_em_update_is_one_code_for_numpy_and_torch():
    import torch
    rng = np.random.RandomState(2)
    n, L, K = 17, 23, 4
    D = rng.randint(0, 3, size=(n, L))
    Q, F = AN.init_random(n, L, K, seed=3)
    got = AN.brute_sweep(D, Q, F)
    want = AN.em_update(Q, F, got['A'], got['B1'], got['B0'], L)
    tt = [torch.as_tensor(a) for a in (Q, F, got['A'], got['B1'], got['B0'])]
    back = AN.em_update(*tt, L)
    assert all(isinstance(t, torch.Tensor) for t in back)
    for w, b in zip(want, back):
        np.testing.assert_allclose(b.numpy(), w, rtol=1e-15, atol=0)
    held = AN.em_update(tt[0], tt[1], tt[2], None, None, L, update_F=False)
    assert held[1] is tt[1]


def test_public_surface():
    from geonomics_amd import _native
    from geonomics_amd.sim.model import Model
    from geonomics_amd.structs.species import Species
    from geonomics_amd.structs.tiled import TiledSpecies
    assert list(inspect.signature(Model.calc_ancestry).parameters) == [
        'self', 'K', 'spp', 'individs', 'n', 'loci', 'init', 'seed', 'accelerate', 'tol',
        'max_sweeps', 'fixed_F']
    sig = inspect.signature(Model.calc_ancestry).parameters
    assert sig['init'].default == 'pca' and sig['accelerate'].default is True
    assert sig['tol'].default == 1e-4 and sig['max_sweeps'].default == 2000
    assert 'fixed_F' in Model.calc_ancestry.__doc__ and 'sample' in Model.calc_ancestry.__doc__
    assert 'K' in inspect.signature(Species._calc_ancestry).parameters
    with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
        TiledSpecies._calc_ancestry(object())
    for name in ('gnx_admix_sweep', 'gnx_admix_info'):
        assert name in _native.EXPORTS
    assert list(inspect.signature(_native.Device.admix_sweep).parameters)[:7] == [
        'self', 'Q', 'F', 'slots', 'locus_mask', 'want_loglik', 'budget']
