"""Model.calc_relatedness and Model.find_kin on the device (csrc/gnx_kin.hip, sim/kin.py,
Species._calc_relatedness / _calc_kin_pairs): gnx_kin_matrix and gnx_kin_pairs against the numpy
restatement (sim/kin.counts_numpy, tests/_kin.brute_pairs: every pair brute-forced as
include/gnx_hip.h specifies), and the public calls against the recorded pedigree.  Needs an
MI355X.

Bounds: none.  Everything the device returns is an integer per individual or per pair, r is
bit-equal on both sides (the fp32 coordinates widen exactly; the differences, the products, their
sum and the IEEE sqrt round identically, without contraction on either side), and the keep rule
is the same integer comparison: matrices and lists are EQUAL, lists in the same order, and a
call repeated is byte-equal."""
import numpy as np
import pytest

import _kin as KT
from test_gpu_parity import native
from test_gpu_sgs import _case_a, _mask
from geonomics_amd.sim import kin as K

pytestmark = pytest.mark.gpu

BIG = 1 << 50
ALL = -(1 << 20)                 # the threshold that keeps every pair with kinship >= -1


def _phased(rng, D):
    """genotypes [n][L][2] with dosages D: a heterozygote's 1 on either homologue"""
    flip = rng.randint(0, 2, D.shape).astype(bool)
    return np.stack([(D == 2) | ((D == 1) & flip), (D == 2) | ((D == 1) & ~flip)],
                    axis=2).astype(np.uint8)


def _handle(nat, G, x, y, shape, ids=None, seed=20):
    """a population with genotypes G [n][L][2] at (x, y) on a handle over a flat landscape of
    `shape` = (H, W)"""
    import gnx_oracle as O
    n, L = G.shape[:2]
    dev = nat.Device(shape[1], shape[0], 1, L=L, n_traits=0, cap_inds=n + 64, cap_rows=n + 64,
                     seed=seed)
    dev.upload_rasters(np.ones((1,) + tuple(shape), np.float32))
    dev.set_species_params(nat.default_species_params())
    dev.upload_population(np.asarray(x, np.float32), np.asarray(y, np.float32), np.zeros(n),
                          np.zeros(n), np.arange(n) if ids is None else ids)
    dev.upload_genomes(O.pack_genomes(G))
    return dev


def _same_list(got, want, label=''):
    for k in ('pa', 'pb', 'hh', 'ibs0', 'nhet'):
        np.testing.assert_array_equal(got[k], want[k], err_msg='%s: %s' % (label, k))
    assert got['n_found'] == want['n_found'] == got['pa'].size, label
    assert got['n_candidates'] == want['n_candidates'], label
    assert (got['pa'] < got['pb']).all(), label


def _check(dev, G, x, y, T, max_dist=None, slots=None, loci=None, label=''):
    """one gnx_kin_pairs call against the brute-force list, and byte-equal when repeated"""
    Gs = G if slots is None else G[slots]
    xs, ys = (x, y) if slots is None else (x[slots], y[slots])
    mask = None if loci is None else _mask(dev, loci)
    got = dev.kin_pairs(T, max_dist, slots, mask, 1 << 22, BIG)
    want = KT.brute_pairs(Gs, xs, ys, T, max_dist, loci)
    _same_list(got, want, label)
    n = Gs.shape[0]
    nw = np.unique((np.arange(G.shape[1]) if loci is None else loci) >> 6).size
    assert want['n_candidates'] * nw <= got['work'] <= n * (n - 1) // 2 * nw, label
    again = dev.kin_pairs(T, max_dist, slots, mask, 1 << 22, BIG)
    for k in ('pa', 'pb', 'hh', 'ibs0', 'nhet'):
        assert again[k].tobytes() == got[k].tobytes(), (label, k)
    print('%s: n = %d, %d candidates, %d kept, work %d, %s'
          % (label, n, got['n_candidates'], got['n_found'], got['work'], dev.kin_info()))
    return got, want


def _check_matrix(dev, G, slots=None, loci=None, label=''):
    got = dev.kin_matrix(slots, None if loci is None else _mask(dev, loci))
    want = K.counts_numpy(G if slots is None else G[slots], loci)
    for k in ('nhet', 'hh', 'ibs0'):
        assert got[k].dtype == np.int32
        np.testing.assert_array_equal(got[k], want[k], err_msg='%s: %s' % (label, k))
    return got


@pytest.fixture(scope='module')
def case_a():
    """test_gpu_sgs.py's case A: n = 131 (two full tiles of 64 rows and 3 rows), L = 130 (three
    words, the last of 2 bits) on a 24 x 20 landscape; the pair (0, 0) - (3, 4) at r = 5 exactly
    and individuals 64 and 130 at one position"""
    nat = native()
    D, x, y = _case_a()
    G = _phased(np.random.RandomState(17), D)
    dev = _handle(nat, G, x, y, (20, 24))
    yield nat, dev, G, x, y
    dev.close()


def test_case_a_matrix_equals_the_restatement(case_a):
    nat, dev, G, x, y = case_a
    got = _check_matrix(dev, G, label='case A')
    assert (np.diag(got['hh']) == got['nhet']).all() and not np.diag(got['ibs0']).any()
    assert (got['hh'] == got['hh'].T).all() and (got['ibs0'] == got['ibs0'].T).all()
    loci = np.sort(np.random.RandomState(3).choice(130, 40, replace=False))
    loci[-1] = 129                                     # the last word's last valid bit
    _check_matrix(dev, G, loci=loci, label='case A, 40 loci')
    _check_matrix(dev, G, loci=np.arange(64, 100), label='case A, one word')
    info = dev.kin_info()
    assert info['launches'] == 3 and info['tasks'] == 6 and info['kernel_ms'] > 0


def test_case_a_pair_lists_against_brute_force(case_a):
    nat, dev, G, x, y = case_a
    a, b = np.triu_indices(131, 1)
    r = KT.pair_radius(x, y)[a, b]
    # every pair closer than 8, in order: cells of side 8 (3 x 3, the last row and column partial)
    got, want = _check(dev, G, x, y, ALL, 8.0, label='case A, r < 8')
    assert got['n_found'] == got['n_candidates'] == (r < 8).sum() > 1000
    np.testing.assert_array_equal(got['pa'], a[r < 8])
    np.testing.assert_array_equal(got['pb'], b[r < 8])
    # r < 5 leaves out the pair at exactly 5 and keeps the pair at 0
    assert r[(a == 0) & (b == 1)] == 5.0 and r[(a == 64) & (b == 130)] == 0.0
    got, _ = _check(dev, G, x, y, ALL, 5.0, label='case A, r < 5')
    pairs = set(zip(got['pa'].tolist(), got['pb'].tolist()))
    assert (0, 1) not in pairs and (64, 130) in pairs
    # a middling threshold: the kept set is keep_rule's
    for mk in (0.0, 0.03):
        got, want = _check(dev, G, x, y, K.threshold(mk), 8.0, label='case A, kinship >= %g' % mk)
        assert 0 < got['n_found'] < got['n_candidates']
    loci = np.sort(np.random.RandomState(3).choice(130, 40, replace=False))
    _check(dev, G, x, y, K.threshold(0.0), 8.0, loci=loci, label='case A, 40 loci')
    # tiny cells: the grid stays at 2^22 cells and finds the co-located pair alone
    got, _ = _check(dev, G, x, y, ALL, 1e-4, label='case A, r < 1e-4')
    assert got['pa'].tolist() == [64] and got['pb'].tolist() == [130]


def test_case_a_without_max_dist_is_the_upper_triangle_of_the_matrix(case_a):
    nat, dev, G, x, y = case_a
    M = dev.kin_matrix()
    a, b = np.triu_indices(131, 1)
    for T in (ALL, K.threshold(0.02)):
        got, _ = _check(dev, G, x, y, T, None, label='case A, every pair')
        keep = K.keep_rule(M['hh'][a, b], M['ibs0'][a, b], M['nhet'][a], M['nhet'][b], T)
        np.testing.assert_array_equal(got['pa'], a[keep])
        np.testing.assert_array_equal(got['pb'], b[keep])
        np.testing.assert_array_equal(got['hh'], M['hh'][a, b][keep])
        np.testing.assert_array_equal(got['ibs0'], M['ibs0'][a, b][keep])
        assert got['n_candidates'] == a.size and got['work'] == a.size * 3
    # an infinite max_dist is no max_dist
    inf = dev.kin_pairs(T, np.inf, None, None, 1 << 22, BIG)
    assert inf['n_candidates'] == a.size and inf['pa'].tobytes() == got['pa'].tobytes() \
        and inf['pb'].tobytes() == got['pb'].tobytes()


@pytest.mark.parametrize('L', [1, 64])
def test_edge_sizes_and_a_permuted_subset_of_slots(L):
    nat = native()
    rng = np.random.RandomState(23 + L)
    n = 70
    x = rng.uniform(0, 12, n).astype(np.float32)
    y = rng.uniform(0, 12, n).astype(np.float32)
    G = (rng.random_sample((n, L, 2)) < 0.5).astype(np.uint8)
    dev = _handle(nat, G, x, y, (12, 12))
    try:
        for m in (1, 2, 64, 65):
            slots = rng.permutation(n)[:m].astype(np.int64)
            _check_matrix(dev, G, slots, label='n = %d' % m)
            for md in (None, 5.0):
                got, _ = _check(dev, G, x, y, ALL, md, slots, label='L = %d, n = %d' % (L, m))
            if m == 1:
                assert got['n_found'] == 0 and got['work'] == 0
        _check(dev, G, x, y, K.threshold(0.1), 6.0, label='L = %d, all' % L)
    finally:
        dev.close()


def test_two_homozygous_individuals_are_never_kept_and_have_no_kinship():
    nat = native()
    rng = np.random.RandomState(29)
    n, L = 6, 100
    G = (rng.random_sample((n, L, 2)) < 0.5).astype(np.uint8)
    G[2, :, 1] = G[2, :, 0]
    G[4, :, 1] = G[4, :, 0]
    x = y = np.full(n, 3.0, np.float32)
    dev = _handle(nat, G, x, y, (8, 8))
    try:
        M = _check_matrix(dev, G, label='homozygous')
        assert M['nhet'][2] == 0 and M['nhet'][4] == 0 and M['hh'][2, 4] == 0
        kin = K.king(M['hh'], M['ibs0'], M['nhet'][:, None], M['nhet'][None, :])
        assert np.isnan(kin[2, 4]) and np.isnan(kin[2, 2]) and np.isnan(kin).sum() == 4
        for md in (None, 2.0):
            got, _ = _check(dev, G, x, y, ALL, md, label='homozygous')
            pairs = set(zip(got['pa'].tolist(), got['pb'].tolist()))
            # (hh - 2 ibs0 = 0 >= T x 0 would hold at any T <= 0: the rule asks for nhet > 0)
            assert (2, 4) not in pairs and (0, 1) in pairs and got['n_candidates'] == 15
    finally:
        dev.close()


@pytest.fixture(scope='module')
def clump():
    """200 individuals inside one cell of side 4 (4 x 4 tiles of the cell with itself, 10 of them
    visited, 4 diagonal; tiles against its neighbours), 150 scattered over the left part of a
    32 x 32 landscape: the right-hand cells are empty"""
    nat = native()
    rng = np.random.RandomState(11)
    n, L = 350, 70
    x = np.concatenate([rng.uniform(8.2, 11.8, 200), rng.uniform(0, 20, 150)]).astype(np.float32)
    y = np.concatenate([rng.uniform(12.2, 15.8, 200), rng.uniform(0, 32, 150)]).astype(np.float32)
    o = rng.permutation(n)
    x, y = x[o], y[o]
    G = _phased(rng, rng.binomial(2, rng.uniform(0.05, 0.95, L), size=(n, L)))
    dev = _handle(nat, G, x, y, (32, 32))
    yield nat, dev, G, x, y
    dev.close()


def test_one_crowded_cell(clump):
    nat, dev, G, x, y = clump
    got, _ = _check(dev, G, x, y, ALL, 4.0, label='clump')
    assert got['n_found'] > 200 * 199 // 4
    _check(dev, G, x, y, K.threshold(0.05), 4.0, label='clump, kinship >= 0.05')


def test_max_pairs_one_below_the_count_is_refused_and_writes_nothing(clump):
    nat, dev, G, x, y = clump
    T = K.threshold(0.05)
    want = KT.brute_pairs(G, x, y, T, 4.0)
    m = want['n_found']
    assert m > 100
    exact = dev.kin_pairs(T, 4.0, None, None, m, BIG)
    _same_list(exact, want, 'max_pairs = the count')
    out = tuple(np.full(m, -7, np.int32) for _ in range(4)) + (np.full(350, -7, np.int32),)
    with pytest.raises(nat.GnxError, match='exceed max_pairs = %d' % (m - 1)) as err:
        dev.kin_pairs(T, 4.0, None, None, m - 1, BIG, out=out)
    assert err.value.n_found == m
    assert all((a == -7).all() for a in out)
    for bad in (0, 2 ** 26 + 1):
        with pytest.raises(nat.GnxError, match='max_pairs'):
            dev.kin_pairs(T, 4.0, None, None, bad, BIG)


def test_refusals_and_the_work_limit_come_before_the_gather(case_a):
    nat, dev, G, x, y = case_a
    before = dev.kin_pairs(K.threshold(0.0), 8.0, None, None, 1 << 22, BIG)
    only = dev.kin_pairs(K.threshold(0.0), 8.0)                # max_work <= 0: the work only
    assert only['work'] == before['work'] > 0 and only['pa'] is None
    assert dev.kin_pairs(0, 8.0, max_work=-5)['work'] == before['work']
    exact = dev.kin_pairs(K.threshold(0.0), 8.0, None, None, 1 << 22, before['work'])
    assert exact['pa'].tobytes() == before['pa'].tobytes()
    with pytest.raises(nat.GnxError, match='exceed max_work = %d' % (before['work'] - 1)):
        dev.kin_pairs(0, 8.0, None, None, 1 << 22, before['work'] - 1)
    # the cell sort's three launches and nothing else: no gather, no pair kernel
    assert dev.kin_info()['launches'] == 3 and dev.kin_info()['tasks'] == 0
    for bad in (-(1 << 20) - 1, (1 << 19) + 1):
        with pytest.raises(nat.GnxError, match='T = '):
            dev.kin_pairs(bad, 8.0, None, None, 1 << 22, BIG)
    with pytest.raises(nat.GnxError, match='NaN'):
        dev.kin_pairs(0, np.nan, None, None, 1 << 22, BIG)
    with pytest.raises(nat.GnxError, match='slot out of range'):
        dev.kin_pairs(0, 8.0, np.array([0, dev.N]), None, 1 << 22, BIG)
    with pytest.raises(nat.GnxError, match='2\\^24'):
        dev.kin_pairs(0, 8.0, np.zeros(0, np.int64), None, 1 << 22, BIG)
    with pytest.raises(nat.GnxError, match='8192'):
        dev.kin_matrix(np.zeros(0, np.int64))
    after = dev.kin_pairs(K.threshold(0.0), 8.0, None, None, 1 << 22, BIG)
    for k in ('pa', 'pb', 'hh', 'ibs0', 'nhet'):
        assert after[k].tobytes() == before[k].tobytes()
    empty = nat.Device(16, 16, 1, L=96, cap_inds=256, cap_rows=256, seed=1)
    empty.upload_rasters(np.ones((1, 16, 16), np.float32))
    empty.set_species_params(nat.default_species_params())
    empty.upload_population(np.ones(10), np.ones(10), np.zeros(10), np.zeros(10), np.arange(10))
    for call in (lambda: empty.kin_pairs(0, 8.0, max_work=BIG), empty.kin_matrix):
        with pytest.raises(nat.GnxError, match='genomes not assigned'):
            call()
    empty.close()


def test_the_synthetic_pedigree_gets_the_hosts_labels():
    nat = native()
    G, parents, rel = KT.synthetic_pedigree(0)
    n = G.shape[0]
    rng = np.random.RandomState(31)
    x = rng.uniform(0, 16, n).astype(np.float32)
    y = rng.uniform(0, 16, n).astype(np.float32)
    dev = _handle(nat, G, x, y, (16, 16))
    try:
        kin, ibs0, lab = KT.labels(G)
        M = _check_matrix(dev, G, label='pedigree')
        dkin = K.king(M['hh'], M['ibs0'], M['nhet'][:, None], M['nhet'][None, :])
        np.testing.assert_array_equal(dkin, kin)
        np.testing.assert_array_equal(K.relationship(dkin, M['ibs0']), lab)
        got, _ = _check(dev, G, x, y, K.threshold(2 ** -3.5), None, label='pedigree')
        named = K.relationship(K.king(got['hh'], got['ibs0'], got['nhet'][got['pa']],
                                      got['nhet'][got['pb']]), got['ibs0'])
        found = dict(zip(zip(got['pa'].tolist(), got['pb'].tolist()), named.tolist()))
        assert set(found) == rel['PO'] | rel['FS'] | rel['second']
        assert all(found[p] == 'PO' for p in rel['PO'])
        assert all(found[p] == 'FS' for p in rel['FS'])
        assert all(found[p] == '2nd' for p in rel['second'])
        assert (got['ibs0'][named == 'PO'] == 0).all() and (named == 'PO').sum() == 64
    finally:
        dev.close()


def test_model_find_kin_against_the_recorded_pedigree():
    """a Model that records its pedigree, mutation off: a parent and its child are never
    opposite homozygotes, find_kin is the filtered matrix, and the truth beside the labels is
    the pedigree's.  (No kinship value of the model population is asserted: nobody has
    measured its background relatedness.)"""
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    p = small_params(seed=9, traits=False, L=200, T=6)
    ga = p['comm']['species']['spp_0']['gen_arch']
    ga.update({'use_tskit': True, 'mu_neut': 0, 'mu_delet': 0})
    mod = gnx.make_model(p)
    with pytest.raises(ValueError, match='no pedigree was recorded'):
        mod.get_pedigree_parents()
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(5, 'main', verbose=False)
    everybody = np.array([*mod.comm[0]])
    sample = np.sort(everybody)[:512] if everybody.size > 512 else np.sort(everybody)
    ids, parents = mod.get_pedigree_parents(individs=sample)
    assert (ids == sample).all() and parents.shape == (ids.size, 2)
    assert (parents >= 0).any() and (parents[parents >= 0] < ids.max()).all()
    rel = mod.calc_relatedness(individs=sample)
    n = ids.size
    assert (rel['ids'] == ids).all() and (np.diag(rel['kinship']) == 0.5).all()
    truth = K.pedigree_relations(parents, ids)
    po = truth['PO']
    assert po.shape[0] > 10
    assert (rel['ibs0'][po[:, 0], po[:, 1]] == 0).all()
    # find_kin on the sample is the filtered matrix, in order
    mk = 2 ** -3.5
    got = mod.find_kin(individs=sample, min_kinship=mk)
    a, b = np.triu_indices(n, 1)
    keep = K.keep_rule(rel['hh'][a, b], rel['ibs0'][a, b], rel['nhet'][a], rel['nhet'][b],
                       K.threshold(mk))
    np.testing.assert_array_equal(got['ids_a'], ids[a[keep]])
    np.testing.assert_array_equal(got['ids_b'], ids[b[keep]])
    np.testing.assert_array_equal(got['kinship'], rel['kinship'][a, b][keep])
    np.testing.assert_array_equal(got['ibs0'], rel['ibs0'][a, b][keep])
    np.testing.assert_array_equal(got['nhet'], rel['nhet'])
    assert got['n_candidates'] == a.size
    # the truth beside the labels is get_pedigree_parents'
    want = K.pair_truth(ids[a[keep]], ids[b[keep]], parents[a[keep]], parents[b[keep]])
    np.testing.assert_array_equal(got['true_relationship'], want)
    listed = set(zip(got['ids_a'].tolist(), got['ids_b'].tolist()))
    print('model: n = %d, %d PO, %d FS, %d HS pairs recorded; %d pairs at kinship >= 2^-3.5, '
          'of which %d recorded relatives'
          % (n, po.shape[0], truth['FS'].shape[0], truth['HS'].shape[0], len(listed),
             (got['true_relationship'] != '').sum()))
    # with a distance: the pairs of the list that are closer, and a sample drawn by n=
    near = mod.find_kin(individs=sample, min_kinship=mk, max_dist=3.0)
    closer = got['dist'] < 3.0
    np.testing.assert_array_equal(near['ids_a'], got['ids_a'][closer])
    np.testing.assert_array_equal(near['ids_b'], got['ids_b'][closer])
    np.testing.assert_array_equal(near['dist'], got['dist'][closer])
    sub = mod.find_kin(n=50, min_kinship=-1.0, max_pairs=50 * 49 // 2)
    assert sub['ids'].size == 50 and sub['ids_a'].size <= 50 * 49 // 2
    with pytest.raises(ValueError, match='n_found = .* exceed max_pairs = 1:'):
        mod.find_kin(individs=sample, min_kinship=-1.0, max_pairs=1)
    with pytest.raises(ValueError, match='exceed max_work = 10:'):
        mod.find_kin(individs=sample, max_work=10)
