"""The host side of Model.prune_ld, clump, calc_ld_scores and run_ldsc (geonomics_amd/sim/ldwin.py,
the argument checks of Species._prune_ld / _clump / _calc_ld_scores / _run_ldsc, the prototypes
of include/gnx_ldwin.h).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import _ld as T
import _ldwin as W
from geonomics_amd.sim import ld as LD
from geonomics_amd.sim import ldwin as LW


@pytest.fixture(scope='module')
def case_a():
    D, pos = W.case_a()
    return T.bits_of(W.gts_of(D)), pos


def test_the_restatements_r2_is_brute_bins_r2_bit_for_bit(case_a):
    bits, pos = case_a
    one = LD.brute_bins(bits, pos, np.array([0.0, np.inf]), 2, True)
    for window in (0.0, 0.3, np.inf):
        ref = LW.brute_window(bits, pos, window, 2, 0.0)
        np.testing.assert_array_equal(ref['c1'], one['c1'])
        np.testing.assert_array_equal(ref['kept'], one['kept'])
        assert ref['r2'].tobytes() == one['r2'].tobytes()
        # with r2_min = 0 the edges are the in-window pairs, their r2 that of the matrix
        assert ref['er2'].tobytes() == one['r2'][ref['ei'], ref['ej']].tobytes()
    assert ref['ei'].size == 127 * 126 // 2                      # inf: every kept pair


def test_partners_are_symmetric_and_an_edge_is_a_near_pair_above_the_threshold(case_a):
    bits, pos = case_a
    assert pos[39] == pos[40] == pos[41] and pos[90] - pos[89] >= LD.BREAK_MORGANS - 1e-9
    L = pos.size
    for window, r2_min in ((0.0, 0.0), (0.05, 0.01), (1.0, 0.02), (np.inf, 0.05)):
        ref = LW.brute_window(bits, pos, window, 2, r2_min)
        kept, r2 = ref['kept'], ref['r2']
        d = pos[None, :] - pos[:, None]
        near = np.triu(np.ones((L, L), bool), 1) & kept[:, None] & kept[None, :] & (d <= window)
        assert (ref['in_window'] == near).all()
        sym = near | near.T
        np.testing.assert_array_equal(ref['partners'], sym.sum(axis=1))
        assert not ref['partners'][~kept].any() and not ref['score'][~kept].any()
        with np.errstate(invalid='ignore'):
            want = near & (r2 >= r2_min)
        got = np.zeros((L, L), bool)
        got[ref['ei'], ref['ej']] = True
        assert (got == want).all() and ref['ei'].size == want.sum()
        key = ref['ei'].astype(np.int64) * L + ref['ej']
        assert (np.diff(key) > 0).all() and (ref['ei'] < ref['ej']).all()
        both = np.where(sym, np.where(np.isnan(r2), r2.T, r2), 0.0)
        np.testing.assert_allclose(ref['score'], both.sum(axis=1), rtol=1e-13, atol=0)
    # window 0: only the tied positions; a finite window never crosses the break
    tied = LW.brute_window(bits, pos, 0.0, 2, 0.0)
    assert sorted(zip(tied['ei'].tolist(), tied['ej'].tolist())) == [(39, 40), (39, 41), (40, 41)]
    short = LW.brute_window(bits, pos, 1.0, 2, 0.0)
    assert not ((short['ei'] < 90) & (short['ej'] >= 90)).any()


def _random_graph(rng, n, m):
    i, j = np.triu_indices(n, 1)
    pick = rng.choice(i.size, m, replace=False)
    return i[pick], j[pick]


def test_greedy_independent_keeps_a_maximal_independent_set_whatever_the_edge_order():
    rng = np.random.RandomState(5)
    for n, m in ((1, 0), (2, 1), (40, 60), (200, 900)):
        ei, ej = _random_graph(rng, n, m)
        rank = rng.permutation(n)
        keep, claimed = LW.greedy_independent(n, ei, ej, rank)
        adj = np.zeros((n, n), bool)
        adj[ei, ej] = adj[ej, ei] = True
        W.check_independent(keep, claimed, rank, adj)
        for _ in range(3):
            p = rng.permutation(m)
            flip = rng.rand(m) < 0.5                        # (and either end first)
            a, b = np.where(flip, ej[p], ei[p]), np.where(flip, ei[p], ej[p])
            k2, c2 = LW.greedy_independent(n, a, b, rank)
            assert (k2 == keep).all() and (c2 == claimed).all()
    keep, claimed = LW.greedy_independent(3, [], [], [2, 0, 1])
    assert keep.all() and (claimed == -1).all()


def test_two_identical_columns_at_r2_one_leave_one():
    rng = np.random.RandomState(7)
    bits = (rng.rand(80, 6) < 0.4).astype(np.uint8)
    bits[:, 4] = bits[:, 1]
    ref = LW.brute_window(bits, np.arange(6.0), np.inf, 1, 1.0)
    assert list(zip(ref['ei'].tolist(), ref['ej'].tolist())) == [(1, 4)] and ref['er2'][0] == 1.0
    rank = LW.maf_rank(ref['c1'], 80)
    keep, claimed = LW.greedy_independent(6, ref['ei'], ref['ej'], rank)
    assert keep.sum() == 5 and keep[1] and not keep[4] and claimed[4] == 1   # the tie: by index
    # the ranks: the commonest minor allele first; p ascending
    minor = np.minimum(ref['c1'], 80 - ref['c1'])
    order = np.argsort(rank)
    assert (np.diff(minor[order]) <= 0).all() and rank[1] < rank[4]
    assert LW.p_rank([0.3, 0.01, 0.3, 0.0]).tolist() == [2, 1, 3, 0]


def test_clumps_drop_the_index_loci_above_p1_with_their_members():
    p = np.array([1e-6, 1e-3, 5e-3, 1e-5, 8e-3, 2e-3])
    ei, ej = np.array([0, 1, 3]), np.array([2, 4, 5])
    keep, claimed = LW.greedy_independent(6, ei, ej, LW.p_rank(p))
    assert keep.tolist() == [True, True, False, True, False, False]
    idx, mem = LW.clumps(p, keep, claimed, 1e-4)
    assert idx.tolist() == [0, 3] and [m.tolist() for m in mem] == [[2], [5]]    # 1 is above p1


def test_ld_scores_and_weights():
    S, m = np.array([0.0, 2.5, 1.0]), np.array([0, 10, 4])
    kept = np.array([True, True, False])
    plain = LW.ld_scores(m, S, kept, 100, adjust=False)
    assert plain[:2].tolist() == [1.0, 3.5] and np.isnan(plain[2])
    adj = LW.ld_scores(m, S, kept, 100, adjust=True)
    assert adj[0] == 1.0 and adj[1] == 1.0 + 2.5 - (10 - 2.5) / 98.0
    # the sum of r2 - (1 - r2) / (N - 2) over the partners, term by term
    r2 = np.array([0.5, 0.25, 0.125])
    np.testing.assert_allclose(LW.ld_scores([3], [r2.sum()], [True], 50)[0],
                               1.0 + (r2 - (1 - r2) / 48.0).sum(), rtol=1e-15)
    assert LW.score_weights(np.array([0.4, 4.0, np.nan])).tolist() == [1.0, 0.25, 0.0]
    with pytest.raises(ValueError, match='more than 2 chromosomes'):
        LW.ld_scores(m, S, kept, 2)


def test_ldsc_recovers_a_planted_noise_free_line():
    rng = np.random.RandomState(11)
    for a, b, m, blocks in ((1.0, 0.02, 500, 200), (1.3, 0.5, 57, 200), (0.9, 3e-4, 1000, 10)):
        ls = 1.0 + rng.gamma(2.0, 20.0, m)
        res = LW.ldsc(a + b * ls, ls, 400, 2000, blocks)
        assert abs(res['intercept'] - a) <= 1e-10 * a and abs(res['slope'] - b) <= 1e-10 * b
        assert abs(res['h2'] - b * 2000 / 400) <= 1e-10 * b * 5
        assert res['n_blocks'] == min(blocks, m) and res['n_loci'] == m
        assert res['intercept_se'] <= 1e-8 and res['slope_se'] <= 1e-8    # nothing to jackknife
        want = (a - 1.0) / ((a + b * ls).mean() - 1.0)
        assert abs(res['ratio'] - want) <= 1e-9 * max(abs(want), 1e-3)
    # noise: the truth within a few standard errors
    ls = 1.0 + rng.gamma(2.0, 20.0, 4000)
    mean = 1.1 + 0.05 * ls
    res = LW.ldsc(mean * rng.chisquare(1, 4000), ls, 400, 4000, 50)
    assert abs(res['intercept'] - 1.1) < 5 * res['intercept_se'] < 2.0
    assert abs(res['slope'] - 0.05) < 5 * res['slope_se'] < 0.05


def test_argument_checks_raise_value_errors():
    with pytest.raises(ValueError, match='unit'):
        LW.check_window(5, 'cM')
    for bad in (-1, float('nan'), True, 'wide', None):
        with pytest.raises(ValueError, match='window: a distance >= 0'):
            LW.check_window(bad, 'loci')
    assert LW.check_window(50, 'loci') == 50.0 and LW.check_window(np.inf, 'morgans') == np.inf
    assert LW.check_window(0.5, 'c') == np.inf
    assert LW.check_window(0.1, 'c') == float(LD.c_to_morgans(0.1))
    for bad in (-0.1, 1.5, True):
        with pytest.raises(ValueError, match='r2: a threshold in 0..1'):
            LW.check_r2(bad)
    with pytest.raises(ValueError, match='differ in length'):
        LW.greedy_independent(3, [0, 1], [1], [0, 1, 2])
    with pytest.raises(ValueError, match='3 distinct values'):
        LW.greedy_independent(3, [0], [1], [0, 1, 1])
    for ei, ej in (([0], [3]), ([-1], [1]), ([2], [2])):
        with pytest.raises(ValueError, match='two different loci in 0..2'):
            LW.greedy_independent(3, ei, ej, [0, 1, 2])
    ls = np.arange(1.0, 11.0)
    with pytest.raises(ValueError, match='at least 3 loci'):
        LW.ldsc([1.0, 2.0], [1.0, 2.0], 10, 10)
    with pytest.raises(ValueError, match='at least 3 loci'):
        LW.ldsc(np.r_[ls[:-1], np.nan], ls, 10, 10)
    with pytest.raises(ValueError, match='all equal'):
        LW.ldsc(ls, np.ones(10), 10, 10)
    for bad in (1, 2.5, True):
        with pytest.raises(ValueError, match='n_blocks'):
            LW.ldsc(ls, ls, 10, 10, bad)


class _Dev:
    L = 40


class _Spp:
    """enough of a Species for the checks that come before the device is asked"""
    from geonomics_amd.structs.analyses import SpeciesAnalyses as A
    _prune_ld, _clump, _calc_ld_scores, _run_ldsc = \
        A._prune_ld, A._clump, A._calc_ld_scores, A._run_ldsc
    _ld_request, _ldw_call, _geno_loci = A._ld_request, A._ldw_call, A._geno_loci
    _LD_MAX_WORK, _LDW_MAX_EDGES = A._LD_MAX_WORK, A._LDW_MAX_EDGES
    gen_arch = object()
    _dev = _Dev()
    _genomes_assigned = True

    def __init__(self):
        self.__dict__['_genomes_assigned'] = True

    def _geno_sample(self, individs):
        return np.arange(10, dtype=np.int64), np.arange(10, dtype=np.int64)


def test_the_species_methods_check_their_arguments_before_the_device_is_asked():
    spp = _Spp()
    with pytest.raises(ValueError, match='prune_ld: r2: a threshold'):
        spp._prune_ld(r2=1.2)
    with pytest.raises(ValueError, match="prune_ld: unit: 'c', 'morgans' or 'loci'"):
        spp._prune_ld(unit='kb')
    with pytest.raises(ValueError, match='prune_ld: window: a distance >= 0'):
        spp._prune_ld(window=-3)
    with pytest.raises(ValueError, match='prune_ld: max_work: a positive number of tile-words'):
        spp._prune_ld(max_work=0)
    for bad in (0, 2 ** 26 + 1, 1.5, True):
        with pytest.raises(ValueError, match='prune_ld: max_edges: a positive integer'):
            spp._prune_ld(max_edges=bad)
    with pytest.raises(ValueError, match='min_maf'):
        spp._calc_ld_scores(min_maf=0.7)
    with pytest.raises(ValueError, match='calc_ld_scores: window'):
        spp._calc_ld_scores(window=float('nan'))
    res = dict(p=np.full((40, 2), 0.5), loci=np.arange(40), tested=np.ones(40, bool))
    with pytest.raises(ValueError, match="clump: result: the dict of an association scan"):
        spp._clump(dict(loci=np.arange(3)))
    with pytest.raises(ValueError, match='clump: r: a column of p in 0..1'):
        spp._clump(res, r=2)
    with pytest.raises(ValueError, match='clump: 0 <= p1 <= p2 <= 1'):
        spp._clump(res, p1=0.1, p2=0.01)
    with pytest.raises(ValueError, match='clump: result: p and loci differ'):
        spp._clump(dict(p=np.ones(3), loci=np.arange(4)))
    # nothing at or below p2: no device call, no clump
    none = spp._clump(dict(res, trait_loci=np.array([3])))
    assert none['n_clumps'] == 0 and none['members'] == [] and none['trait_loci_hit'].size == 0
    sc = dict(ld_score=np.arange(1.0, 41.0), loci=np.arange(40), n_chrom=20)
    with pytest.raises(ValueError, match="run_ldsc: result"):
        spp._run_ldsc(dict(loci=np.arange(40)), sc)
    with pytest.raises(ValueError, match="run_ldsc: scores: the dict of calc_ld_scores"):
        spp._run_ldsc(dict(res, t=np.ones((40, 2))), dict(loci=np.arange(40)))
    with pytest.raises(ValueError, match='run_ldsc: r: a column of t'):
        spp._run_ldsc(dict(res, t=np.ones((40, 2))), sc, r=5)
    # the planted line through the Species method: t^2 = 1 + 0.1 l on the tested loci
    t = np.sqrt(1.0 + 0.1 * sc['ld_score'])
    tested = np.ones(40, bool)
    tested[[3, 9]] = False
    got = spp._run_ldsc(dict(loci=np.arange(40), t=np.column_stack([t, -t]), tested=tested,
                             ids=np.arange(10)), sc, r=1, n_blocks=500)
    assert abs(got['intercept'] - 1.0) <= 1e-10 and abs(got['slope'] - 0.1) <= 1e-11
    assert got['n_loci'] == 38 == got['n_blocks'] and abs(got['h2'] - 0.1 * 40 / 10) <= 1e-9


def test_the_header_of_its_own_is_read_like_the_others_and_the_tiled_species_refuses():
    from geonomics_amd import _native as nat
    from geonomics_amd.structs.tiled import _NOT_TILED, TiledSpecies
    i64, i32, dbl = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    assert nat.PROTOTYPES_LDWIN == {
        'gnx_ld_window': (C.c_int, [C.c_void_p, C.c_int64, i64, C.c_int32, i32, dbl, C.c_double,
                                    C.c_int32, C.c_double, C.c_int64, C.c_int64, i64, i64, i64,
                                    dbl, i64, i32, i32, dbl]),
        'gnx_ld_window_info': (C.c_int, [C.c_void_p, dbl, i64, i64])}
    assert not set(nat.PROTOTYPES_LDWIN) & set(nat.PROTOTYPES)
    for name in ('_prune_ld', '_clump', '_calc_ld_scores', '_run_ldsc'):
        assert name in _NOT_TILED
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            getattr(TiledSpecies, name)(object())
