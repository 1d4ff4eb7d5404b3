"""The host side of the kinship calls (geonomics_amd/sim/kin.py, TreeTables.parents_of,
Species._calc_relatedness / _calc_kin_pairs, Model.calc_relatedness / find_kin): the numpy
restatement on a case worked by hand, the integer keep rule, the labels on a synthetic pedigree,
the pedigree's parents, and the request checks with their texts.  No GPU, no library.

The synthetic pedigree (tests/_kin.py): 40 founders, p ~ U(0.1, 0.9), L = 16384, free
recombination.  KING-robust kinship is a ratio of sums over the loci, so its spread falls as
1 / sqrt(L): over twenty seeds of such pedigrees the unrelated pairs lay in -0.036..0.029, the
second-degree pairs in 0.108..0.143 and the first-degree pairs in 0.237..0.261, each inside its
class (cutoffs 0.0884, 0.177, 0.354), and the smallest full-sib ibs0 was 288 (a full-sib pair
shares no allele IBD at a quarter of the loci, so its ibs0 is in the hundreds here; a
parent-offspring pair's is 0).  At L = 4096 the second-degree minimum was 0.091 against the
0.0884 cutoff, which is why L is 16384.  Half-avuncular pairs (expected 1/16) straddle the
2^-4.5 cutoff: nothing is asserted about them."""
import inspect
import types

import numpy as np
import pytest

import _kin as KT
from test_analyses_host import NO_GENOMES, UNASSIGNED, _Species, _refusal
from geonomics_amd import _native as nat
from geonomics_amd.sim import kin as K
from geonomics_amd.structs.analyses import SpeciesAnalyses
from geonomics_amd.structs.pedigree import TreeTables

# three individuals at four loci, worked by hand:
#        locus 0   1      2      3       het        P (hom 1)   O (carries 1)
#   a    (0,1)  (1,1)  (0,0)  (1,0)     {0, 3}     {1}         {0, 1, 3}
#   b    (1,0)  (0,0)  (1,1)  (1,1)     {0}        {2, 3}      {0, 2, 3}
#   c    (1,1)  (1,1)  (0,1)  (0,0)     {2}        {0, 1}      {0, 1, 2}
HAND = np.array([[[0, 1], [1, 1], [0, 0], [1, 0]],
                 [[1, 0], [0, 0], [1, 1], [1, 1]],
                 [[1, 1], [1, 1], [0, 1], [0, 0]]], np.uint8)


def test_counts_on_a_case_worked_by_hand():
    c = K.counts_numpy(HAND)
    assert c['nhet'].tolist() == [2, 1, 1]
    # hh: a and b are both heterozygous at locus 0 only; the diagonal is nhet
    assert c['hh'].tolist() == [[2, 1, 0], [1, 1, 0], [0, 0, 1]]
    # ibs0: a-b P_a \ O_b = {1}, P_b \ O_a = {2}; a-c none; b-c P_b \ O_c = {3}, P_c \ O_b = {1}
    assert c['ibs0'].tolist() == [[0, 2, 0], [2, 0, 2], [0, 2, 0]]
    kin = K.king(c['hh'], c['ibs0'], c['nhet'][:, None], c['nhet'][None, :])
    assert kin.tolist() == [[0.5, -1.0, 0.0], [-1.0, 0.5, -2.0], [0.0, -2.0, 0.5]]
    # loci 0 and 1 only: c has no heterozygous locus left
    c2 = K.counts_numpy(HAND, [0, 1])
    assert c2['nhet'].tolist() == [1, 1, 0]
    assert c2['hh'].tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 0]]
    assert c2['ibs0'].tolist() == [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
    k2 = K.king(c2['hh'], c2['ibs0'], c2['nhet'][:, None], c2['nhet'][None, :])
    assert k2[0, 1] == -0.5 and np.isnan(k2[2, 2]) and k2[0, 2] == 0.0
    with pytest.raises(ValueError, match=r'\[n\]\[L\]\[2\]'):
        K.counts_numpy(HAND[:, :, 0])


def test_a_self_pair_has_kinship_one_half_and_is_a_duplicate():
    rng = np.random.RandomState(1)
    G = (rng.random_sample((5, 300, 2)) < 0.4).astype(np.uint8)
    kin, ibs0, rel = KT.labels(np.concatenate([G, G[:2]]))
    assert (np.diag(kin) == 0.5).all() and (np.diag(ibs0) == 0).all()
    assert kin[0, 5] == 0.5 and kin[1, 6] == 0.5 and ibs0[0, 5] == 0
    assert rel[0, 5] == 'dup' and rel[3, 3] == 'dup' and K.relationship(0.5, 0) == 'dup'


def test_the_keep_rule_is_the_float_comparison_away_from_the_boundary_and_exact_on_it():
    rng = np.random.RandomState(2)
    m = 20000
    nh_a, nh_b = rng.randint(0, 3000, m), rng.randint(0, 3000, m)
    hh = rng.randint(0, 1 + np.minimum(nh_a, nh_b))
    ibs0 = rng.randint(0, 400, m)
    for mk in (2 ** -3.5, 2 ** -2.5, 0.0, -1.0, 0.5, 0.1):
        T = K.threshold(mk)
        assert T == int(np.ceil(mk * 2 ** 20)) and -2 ** 20 <= T <= 2 ** 19
        kept = K.keep_rule(hh, ibs0, nh_a, nh_b, T)
        kin = K.king(hh, ibs0, nh_a, nh_b)
        assert not kept[np.isnan(kin)].any() and np.isnan(kin).sum() == (nh_a + nh_b == 0).sum()
        # T / 2^20 is within 2^-20 of min_kinship: away from that the two rules agree
        away = ~np.isnan(kin) & (np.abs(kin - mk) > 2.0 ** -19)
        assert away.sum() > m // 2
        np.testing.assert_array_equal(kept[away], kin[away] >= mk)
    # on the boundary the integers decide: 1 / 8 is kept at min_kinship = 1 / 8 ...
    assert K.threshold(0.125) == 131072
    assert K.keep_rule(1, 0, 3, 5, 131072) and not K.keep_rule(1, 0, 4, 5, 131072)
    assert K.keep_rule(5, 2, 3, 5, 131072)
    # ... and 2^-3.5 is irrational, so T / 2^20 lies just above it: a ratio between the two is
    # kept by the float comparison and dropped by the rule the device applies
    T = K.threshold(2 ** -3.5)
    assert T == 92682
    num, den = 88388348, 10 ** 9
    assert 2 ** -3.5 <= num / den < T / 2 ** 20
    assert not K.keep_rule(num, 0, den, 0, T) and K.keep_rule(num + 100, 0, den, 0, T)
    # never without a heterozygous locus, whatever the threshold
    assert not K.keep_rule(0, 0, 0, 0, -2 ** 20)
    for bad in (0.6, -1.01, np.nan, np.inf):
        with pytest.raises(ValueError, match='min_kinship'):
            K.threshold(bad)


def test_relationship_cutoffs():
    c = K.CUTOFFS
    assert c == (2 ** -1.5, 2 ** -2.5, 2 ** -3.5, 2 ** -4.5)
    k = np.array([0.5, c[0] + 1e-9, c[0], 0.25, 0.25, c[1], c[1] - 1e-9, c[2], c[2] - 1e-9,
                  c[3], c[3] - 1e-9, -0.2, np.nan])
    z = np.array([0, 0, 0, 0, 7, 3, 0, 0, 0, 0, 0, 0, 0])
    assert K.relationship(k, z).tolist() == ['dup', 'dup', 'PO', 'PO', 'FS', 'FS', '2nd', '2nd',
                                             '3rd', '3rd', 'un', 'un', 'un']
    assert K.relationship(0.25, 7, po_max_ibs0=7) == 'PO'
    assert K.relationship(0.25, 8, po_max_ibs0=7) == 'FS'


@pytest.fixture(scope='module')
def pedigree():
    return KT.synthetic_pedigree(0)


def test_labels_on_a_synthetic_pedigree(pedigree):
    G, parents, rel = pedigree
    assert G.shape == (72, 16384, 2)
    assert len(rel['PO']) == 64 and len(rel['FS']) == 8 and len(rel['second']) == 40
    kin, ibs0, lab = KT.labels(G)

    def of(kind, M):
        a, b = np.array(sorted(rel[kind])).T
        return M[a, b]

    span = {k: (of(k, kin).min(), of(k, kin).max()) for k in rel}
    print('kinship: ' + ', '.join('%s %.3f..%.3f' % (k, lo, hi) for k, (lo, hi) in span.items())
          + '; full-sib ibs0 >= %d' % of('FS', ibs0).min())
    assert (of('PO', lab) == 'PO').all() and (of('PO', ibs0) == 0).all()
    assert (of('FS', lab) == 'FS').all() and of('FS', ibs0).min() > 100
    assert (of('second', lab) == '2nd').all()
    assert (of('unrelated', kin) < 2 ** -3.5).all()
    assert np.isin(of('unrelated', lab), ['un', '3rd']).all()
    # the pedigree's own account of the relations, from the parents alone
    truth = K.pedigree_relations(parents)
    assert {tuple(p) for p in truth['PO'].tolist()} == rel['PO']
    assert {tuple(p) for p in truth['FS'].tolist()} == rel['FS']
    half_sibs = {(a, b) for a, b in rel['second'] if parents[a, 0] >= 0 and parents[b, 0] >= 0
                 and parents[a, 0] == parents[b, 0] and parents[a, 1] != parents[b, 1]}
    assert len(half_sibs) == 16 and {tuple(p) for p in truth['HS'].tolist()} == half_sibs


def test_pair_truth_and_pedigree_relations_by_id():
    ids = np.array([10, 11, 12, 13, 14, 15, 16])
    #            founders     12 = 10 x 11   13 = 10 x 11   14 = 10 x 15   16 = 12 x 13
    par = np.array([[-1, -1], [-1, -1], [10, 11], [11, 10], [10, 15], [-1, -1], [12, 13]])
    t = K.pedigree_relations(par, ids)
    assert t['PO'].tolist() == [[0, 2], [0, 3], [0, 4], [1, 2], [1, 3], [2, 6], [3, 6], [4, 5]]
    assert t['FS'].tolist() == [[2, 3]]                       # whichever parent gave which
    assert t['HS'].tolist() == [[2, 4], [3, 4]]
    # two founders share their missing parents: not sibs
    assert K.pair_truth([10], [11], [[-1, -1]], [[-1, -1]]).tolist() == ['']
    with pytest.raises(ValueError, match='ids'):
        K.pedigree_relations(par, ids[:3])


def _table():
    tt = TreeTables(4, [0, 0], np.zeros(0, np.int64))
    tt.add_founders(np.array([3, 5, 9]), np.zeros((3, 2)))
    tt.add_births(1, np.array([12, 11]), np.array([[3, 5], [9, 3]]), np.zeros((2, 2), np.int64),
                  np.array([[0, 1], [1, 0]]), np.zeros((2, 2)))
    tt.add_births(2, np.array([20]), np.array([[12, 5]]), np.zeros((1, 2), np.int64),
                  np.zeros((1, 2), np.int64), np.zeros((1, 2)))
    return tt


def test_parents_of_on_a_hand_built_table():
    tt = _table()
    got = tt.parents_of([3, 11, 12, 20, 99, 4, 0])
    assert got.dtype == np.int64
    assert got.tolist() == [[-1, -1], [9, 3], [3, 5], [12, 5], [-1, -1], [-1, -1], [-1, -1]]
    assert tt.parents_of([]).shape == (0, 2)
    assert TreeTables(4, [0, 0], np.zeros(0, np.int64)).parents_of([1]).tolist() == [[-1, -1]]
    # simplified for the living {20}: 9 and 11 leave the table, the ancestors of 20 keep theirs
    tt.simplify(np.array([np.searchsorted(tt.ids, 20)]))
    assert tt.ids.tolist() == [3, 5, 12, 20]
    assert tt.parents_of([11, 12, 20, 9]).tolist() == [[-1, -1], [3, 5], [12, 5], [-1, -1]]


# ------------------------------------------------------------------ the Species' calls
class _Over(SpeciesAnalyses):
    """a Species stand-in: the real _calc_relatedness and _calc_kin_pairs over the numpy device"""

    def __init__(self, G, ids, xy, tt=None):
        self._dev = KT.NumpyDevice(G, xy[:, 0], xy[:, 1])
        self.ids, self.xy = np.asarray(ids), xy
        self.gen_arch = types.SimpleNamespace()
        self._genomes_assigned = True
        self._tt = tt

    def _geno_sample(self, individs):
        order = np.argsort(self.ids)
        if individs is None:
            return self.ids[order], order
        ids = np.sort(np.asarray(individs))
        return ids, order[np.searchsorted(self.ids[order], ids)]

    def _field(self, f):
        return self.xy[:, 0 if f == nat.F_X else 1]


def test_species_methods_over_a_numpy_device():
    rng = np.random.RandomState(5)
    G, parents, rel = KT.synthetic_pedigree(3, L=2048, n_founders=8, n_fam=2)
    n = G.shape[0]
    ids = rng.permutation(n) * 3 + 7
    xy = rng.uniform(0, 10, (n, 2)).astype(np.float32)
    spp = _Over(G, ids, xy)
    order = np.argsort(ids)
    kin, ibs0, lab = KT.labels(G[order])
    res = spp._calc_relatedness()
    assert (res['ids'] == ids[order]).all()
    np.testing.assert_array_equal(res['kinship'], kin)
    np.testing.assert_array_equal(res['ibs0'], ibs0)
    assert (np.diag(res['hh']) == res['nhet']).all()
    sub = spp._calc_relatedness(individs=ids[:5], loci=np.arange(100, 900))
    o5 = np.argsort(ids[:5])
    np.testing.assert_array_equal(sub['kinship'], KT.labels(G[:5][o5], np.arange(100, 900))[0])
    # the pair list: the filtered upper triangle, in order, with distances and labels
    got = spp._calc_kin_pairs(min_kinship=0.1)
    a, b = np.triu_indices(n, 1)
    keep = K.keep_rule(res['hh'][a, b], res['ibs0'][a, b], res['nhet'][a], res['nhet'][b],
                       K.threshold(0.1))
    assert 0 < keep.sum() < a.size
    np.testing.assert_array_equal(got['ids_a'], ids[order][a[keep]])
    np.testing.assert_array_equal(got['ids_b'], ids[order][b[keep]])
    np.testing.assert_array_equal(got['kinship'], kin[a, b][keep])
    np.testing.assert_array_equal(got['relationship'], lab[a, b][keep])
    np.testing.assert_array_equal(got['dist'], KT.pair_radius(*xy[order].T)[a, b][keep])
    assert got['n_candidates'] == a.size and 'true_relationship' not in got
    near = spp._calc_kin_pairs(max_dist=4.0, min_kinship=-1.0, po_max_ibs0=10 ** 6)
    assert near['n_candidates'] == (KT.pair_radius(*xy.T)[a, b] < 4.0).sum()
    assert (near['dist'] < 4.0).all() and 'FS' not in near['relationship']
    # the library's refusals become ValueErrors with advice
    msg = _refusal(spp._calc_kin_pairs, min_kinship=0.1, max_pairs=3)
    assert msg.startswith('find_kin: n_found = %d kept pairs exceed max_pairs = 3: ' % keep.sum())
    assert 'higher min_kinship' in msg and 'smaller max_dist' in msg and 'larger max_pairs' in msg
    msg = _refusal(spp._calc_kin_pairs, max_work=9)
    assert 'exceed max_work = 9' in msg and 'n=...' in msg and 'max_dist' in msg


def test_the_truth_of_a_recorded_pedigree_stands_beside_the_labels():
    tt = _table()
    ids = np.array([20, 5, 12, 3, 11])
    G = (np.random.RandomState(8).random_sample((5, 640, 2)) < 0.5).astype(np.uint8)
    spp = _Over(G, ids, np.zeros((5, 2), np.float32), tt)
    got = spp._calc_kin_pairs(min_kinship=-1.0)
    pairs = list(zip(got['ids_a'].tolist(), got['ids_b'].tolist(),
                     got['true_relationship'].tolist()))
    # 11 = 9 x 3 and 12 = 3 x 5 share 3; 20 = 12 x 5
    assert pairs == [(3, 5, ''), (3, 11, 'PO'), (3, 12, 'PO'), (3, 20, ''), (5, 11, ''),
                     (5, 12, 'PO'), (5, 20, 'PO'), (11, 12, 'HS'), (11, 20, ''), (12, 20, 'PO')]
    p_ids, par = spp._get_pedigree_parents()
    assert p_ids.tolist() == [3, 5, 11, 12, 20]
    assert par.tolist() == [[-1, -1], [-1, -1], [9, 3], [3, 5], [12, 5]]
    assert spp._get_pedigree_parents([12])[1].tolist() == [[3, 5]]
    spp._tt = None
    assert 'no pedigree was recorded' in _refusal(spp._get_pedigree_parents)


@pytest.mark.parametrize('who,method', [('calc_relatedness', '_calc_relatedness'),
                                        ('find_kin', '_calc_kin_pairs')])
def test_both_calls_refuse_a_species_without_assigned_genomes(who, method):
    assert _refusal(getattr(_Species(L=0), method)) == '%s: %s' % (who, NO_GENOMES)
    assert _refusal(getattr(_Species(assigned=False), method)) == '%s: %s' % (who, UNASSIGNED)


def test_request_checks_come_before_any_device_call_and_name_the_argument():
    f = _Species()._calc_kin_pairs                 # (its handle has no calls at all)
    for bad in (0.6, -1.5, np.nan, np.inf, 'close', None):
        assert _refusal(f, min_kinship=bad) == \
            'find_kin: min_kinship: a finite number in [-1, 0.5] (got %r)' % (bad,)
    for bad in (0, -2.0, np.inf, np.nan, True):
        assert _refusal(f, max_dist=bad) == \
            'find_kin: max_dist: None or a positive finite distance (got %r)' % (bad,)
    for bad in (0, -1, 1.5, True, 2 ** 26 + 1):
        assert _refusal(f, max_pairs=bad) == \
            'find_kin: max_pairs: a positive integer, at most 2^26 (got %r)' % (bad,)
    for bad in (0, True, 1.5):
        assert _refusal(f, max_work=bad) == \
            'find_kin: max_work: a positive number of pair-words (got %r)' % (bad,)
    # in that order, and all of them before the handle is touched
    assert 'min_kinship' in _refusal(f, min_kinship=2, max_dist=-1, max_pairs=0, max_work=0)
    assert 'max_dist' in _refusal(f, max_dist=-1, max_pairs=0, max_work=0)
    assert 'max_pairs' in _refusal(f, max_pairs=0, max_work=0)
    with pytest.raises(AttributeError, match='kin_pairs'):
        f()
    with pytest.raises(AttributeError, match='kin_matrix'):
        _Species()._calc_relatedness()


def test_more_than_8192_individuals_are_refused_as_get_genetic_distances_refuses_them():
    spp = _Species()
    spp._geno_sample = lambda individs: (np.arange(8193), np.arange(8193))
    assert _refusal(spp._calc_relatedness).startswith(
        'relatedness of at most 8192 individuals per call (got 8193)')
    assert _refusal(spp._calc_genetic_distances) == \
        'genetic distances of at most 8192 individuals per call (got 8193)'


def test_the_model_calls_take_a_sample_and_the_tiled_species_refuses():
    from geonomics_amd.sim.model import Model
    from geonomics_amd.structs.species import Species
    from geonomics_amd.structs.tiled import TiledSpecies
    for name in ('calc_relatedness', 'find_kin'):
        sig = inspect.signature(getattr(Model, name))
        assert {'spp', 'individs', 'n', 'loci'} <= set(sig.parameters)
    sig = inspect.signature(Model.find_kin)
    spp_sig = inspect.signature(Species._calc_kin_pairs)
    for k in ('max_dist', 'min_kinship', 'max_pairs', 'max_work', 'po_max_ibs0'):
        assert sig.parameters[k].default == spp_sig.parameters[k].default
    assert spp_sig.parameters['min_kinship'].default == 2 ** -3.5
    assert spp_sig.parameters['max_pairs'].default == 1 << 22
    assert set(inspect.signature(Model.get_pedigree_parents).parameters) == \
        {'self', 'spp', 'individs'}
    for f in (TiledSpecies._calc_relatedness, TiledSpecies._calc_kin_pairs):
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            f(object())
