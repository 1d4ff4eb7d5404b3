"""Model.calc_spatial_structure on the device (csrc/gnx_sgs.hip, sim/sgs.py,
Species._calc_spatial_structure): gnx_sgs_sums against the numpy restatement of tests/_sgs.py
(every pair brute-forced as include/gnx_hip.h specifies), against the repository's own exact
Gram matrix where the two overlap, and the public call against the explicit per-pair
statistics on the downloaded genotypes and coordinates.  Needs an MI355X.

Bounds.  isums and n_zero are integers: equal, and bit-equal when the call is repeated (so are
the fp64 sums: the library takes them in a fixed order).  An fsums entry is a sum of the
m = pairs terms of its class; the two sides' terms differ as follows, in units of 2^-53 relative
to the term.  r: the fp32 coordinates widen exactly, and the differences, the products, their
sum and the IEEE sqrt round identically on both sides (no contraction on either) - r is
bit-equal: 0.  ln r: the device's log and numpy's are each within 1 ulp = 2 units of the true
value, so within 4 of each other: 4.  ln^2 r: twice that, and the product rounds once on each
side: 10.  dot ln r, (self_a + self_b) ln r, (w_a + w_b) ln r: the integer factors are exact
and w_a is bit-equal (weight[l] d is exact, the loci are added in ascending order on both
sides, one rounding each; w_a + w_b rounds identically), so 4 for the logarithm and one
rounding of the product on each side: 6.  w_a + w_b: 0.  The oracle's sum is the correctly
rounded sum of its terms (math.fsum): half an ulp of the sum, at most 1 unit of sum |term|; the
device's sum in any order adds m units (the any-order bound test_gpu_mmrr.py uses):

    |S - S_ref| <= (m + c) 2^-53 sum |term|,   c = 1, 5, 11, 7, 7, 1, 7  for the seven sums.

Measured on an MI355X: the worst error is 2.2e-2 of its bound (n = 77, classes of 39 to 496
pairs), 1.1e-2 on case A, 9.9e-4 on the clump and 3e-5 with 79799 pairs in one class; the
end-to-end statistics of the model test are within 4.4e-12.  End-to-end statistics must be within 1e-9 relative of the explicit per-pair
statistics; p-values are compared for equality only after asserting on the host that no
permuted statistic of the oracle lies within 1e-8 relative of the observed one."""
import numpy as np
import pytest

import _sgs as O
from test_gpu_mmrr import _handle
from test_gpu_parity import native
from test_sgs_host import BAR, GAP, close
from geonomics_amd.sim import mmrr as M
from geonomics_amd.sim import sgs as G

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
C_TERM = np.array([1, 5, 11, 7, 7, 1, 7], np.float64)
BIG = 1 << 50
EDGES_A = np.array([0.0, 1.5, 3.0, 5.0, 8.0])


def _mask(dev, loci):
    m = np.zeros(dev.W64, np.uint64)
    np.bitwise_or.at(m, loci >> 6, np.uint64(1) << (loci & 63).astype(np.uint64))
    return m


def _check(dev, D, x, y, edges, slots=None, loci=None, perm=None, label=''):
    """one call against the oracle within the bounds of the module's docstring, and bit-equal
    when repeated; -> (the call's dict, the oracle's isums, fsums, n_zero)"""
    Dn = D if slots is None else D[slots]
    xs, ys = (x, y) if slots is None else (x[slots], y[slots])
    Dn = Dn if loci is None else Dn[:, loci]
    n = Dn.shape[0]
    w_full = np.zeros(D.shape[1])
    pbar = G.locus_terms(Dn.sum(axis=0), n)[0]
    w_full[np.arange(D.shape[1]) if loci is None else loci] = pbar
    mask = None if loci is None else _mask(dev, loci)
    got = dev.sgs_sums(edges, slots, mask, w_full, perm, BIG)
    Dp = Dn if perm is None else O.permuted(Dn, perm)
    isums, fsums, nz, absums = O.brute_sums(xs, ys, Dp, edges, pbar)
    np.testing.assert_array_equal(got['isums'], isums, err_msg=label)
    assert got['n_zero'] == nz, label
    bound = (isums[:, :1] + C_TERM[None, :]) * U53 * absums
    err = np.abs(got['fsums'] - fsums)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print('%s: n = %d, pairs %s, n_zero %d, work %d: worst error / bound %.3g'
          % (label, n, isums[:, 0].tolist(), nz, got['work'], worst))
    assert (err <= bound).all(), (label, err, bound)
    nw = np.unique((np.arange(D.shape[1]) if loci is None else loci) >> 6).size
    assert (isums[:, 0].sum() + nz) * nw <= got['work'] <= n * (n - 1) // 2 * nw, label
    again = dev.sgs_sums(edges, slots, mask, w_full, perm, BIG)
    np.testing.assert_array_equal(again['isums'], got['isums'])
    assert again['fsums'].tobytes() == got['fsums'].tobytes()
    assert again['n_zero'] == got['n_zero'] and again['work'] == got['work']
    return got, isums, fsums, nz


def _case_a():
    """n = 131 (two full tiles of 64 rows and 3 rows), L = 130 (three words, the last of 2
    bits), on a 24 x 20 landscape: with EDGES_A the cells have side 8 (3 x 3 of them, the last
    row and column partial); two monomorphic loci, one duplicated position, and one pair at
    (0, 0) - (3, 4), whose r is exactly 5"""
    rng = np.random.RandomState(7)
    n, L = 131, 130
    x = rng.uniform(0, 24, n).astype(np.float32)
    y = rng.uniform(0, 20, n).astype(np.float32)
    x[0], y[0], x[1], y[1] = 0.0, 0.0, 3.0, 4.0
    x[130], y[130] = x[64], y[64]
    D = rng.binomial(2, rng.uniform(0.1, 0.9, L), size=(n, L))
    D[:, 5], D[:, 129] = 0, 2
    return D, x, y


@pytest.fixture(scope='module')
def case_a():
    nat = native()
    D, x, y = _case_a()
    dev = _handle(nat, D, x, y, np.arange(131), np.ones((1, 20, 24)))
    yield nat, dev, D, x, y
    dev.close()


def test_case_a_every_class_two_tiles_and_a_partial_word(case_a):
    nat, dev, D, x, y = case_a
    got, isums, fsums, nz = _check(dev, D, x, y, EDGES_A, label='case A')
    assert nz == 1 and (isums[:, 0] > 100).all()                # every class is filled
    a, b, r, k = O.pair_geometry(x, y, EDGES_A)
    assert r[(a == 0) & (b == 1)] == 5.0 and k[(a == 0) & (b == 1)] == 3
    # through the host arithmetic: the explicit per-pair statistics
    res = G.spatial_structure(got['isums'], got['fsums'], D.sum(axis=0), 131)
    want = O.explicit_stats(x, y, D, EDGES_A)
    for key in ('mean_r', 'mean_lnr', 'F', 'dist2', 'slope', 'F1', 'Sp'):
        close(res[key], want[key], key)


def test_a_clump_in_one_cell_scattered_others_and_empty_cells():
    """200 individuals inside one cell of side 4 (4 x 4 tiles of the cell with itself, 10 of
    them kept, 4 diagonal; several tiles against each neighbour), 150 scattered over the left
    part of a 32 x 32 landscape: the right-hand cells are empty"""
    nat = native()
    rng = np.random.RandomState(11)
    n, L = 350, 70
    x = np.concatenate([rng.uniform(8.2, 11.8, 200), rng.uniform(0, 20, 150)]).astype(np.float32)
    y = np.concatenate([rng.uniform(12.2, 15.8, 200), rng.uniform(0, 32, 150)]).astype(np.float32)
    o = rng.permutation(n)
    x, y = x[o], y[o]
    D = rng.binomial(2, rng.uniform(0.05, 0.95, L), size=(n, L))
    dev = _handle(nat, D, x, y, np.arange(n), np.ones((1, 32, 32)))
    try:
        _, isums, _, _ = _check(dev, D, x, y, np.array([0.25, 1.0, 2.0, 4.0]), label='clump')
        assert (isums[:, 0] > 1000).all()
    finally:
        dev.close()


def test_one_class_covering_every_pair_is_the_gram_matrix():
    nat = native()
    rng = np.random.RandomState(13)
    n, L = 400, 96
    x = rng.uniform(0, 10, n).astype(np.float32)
    y = rng.uniform(0, 10, n).astype(np.float32)
    x[7], y[7] = x[300], y[300]
    D = rng.binomial(2, rng.uniform(0.1, 0.9, L), size=(n, L))
    dev = _handle(nat, D, x, y, np.arange(n), np.ones((1, 10, 10)))
    try:
        got, isums, _, nz = _check(dev, D, x, y, np.array([0.0, 20.0]), label='one class')
        assert nz == 1 and isums[0, 0] + nz == n * (n - 1) // 2
        assert got['work'] == n * (n - 1) // 2 * 2
        Gm = dev.geno_gram()
        a, b, r, _ = O.pair_geometry(x, y, [0.0, 20.0])
        keep = r > 0
        g = np.diag(Gm)
        want = (g[a] + g[b] - 2 * Gm[a, b])[keep].sum()
        assert got['isums'][0, 2] - 2 * got['isums'][0, 1] == want
    finally:
        dev.close()


def test_edges_far_below_the_cell_spacing_cap_the_number_of_cells(case_a):
    nat, dev, D, x, y = case_a
    # 24 x 20 at a side of 1e-4 would be 4.8e10 cells: the grid stays at 2^22 and still finds
    # the duplicated position (n_zero) and nothing else but what the oracle finds
    got, isums, _, nz = _check(dev, D, x, y, np.array([0.0, 1e-4]), label='tiny edges')
    assert nz == 1 and isums[0, 0] == 0 and got['work'] < 131 * 130 // 2 * 3


def test_one_and_two_individuals_slots_masks_and_perm(case_a):
    nat, dev, D, x, y = case_a
    got = dev.sgs_sums(EDGES_A, np.array([5]), None, None, None, BIG)
    assert got['work'] == 0 and got['n_zero'] == 0 and not got['isums'].any() \
        and not got['fsums'].any()
    _check(dev, D, x, y, EDGES_A, np.array([1, 0]), label='n = 2')           # r = 5 exactly
    _check(dev, D, x, y, EDGES_A, np.array([64, 130]), label='n = 2, r = 0')
    rng = np.random.RandomState(3)
    slots = rng.choice(131, 77, replace=False).astype(np.int64)
    loci = np.sort(rng.choice(130, 40, replace=False))
    loci[-1] = 129                                     # the last word's last valid bit
    _check(dev, D, x, y, EDGES_A, slots, loci, label='slots and mask')
    one_word = np.arange(64, 100)
    got, *_ = _check(dev, D, x, y, EDGES_A, None, one_word, label='one word')
    assert got['work'] <= 131 * 130 // 2
    perm = rng.permutation(131).astype(np.int32)
    _check(dev, D, x, y, EDGES_A, perm=perm, label='perm')
    _check(dev, D, x, y, EDGES_A, slots, loci, rng.permutation(77).astype(np.int32),
           label='perm of a subset')
    # no weights: the two w sums are 0 and the rest is unchanged
    a = dev.sgs_sums(EDGES_A, None, None, None, None, BIG)
    b = dev.sgs_sums(EDGES_A, None, None, np.zeros(130), None, BIG)
    assert not a['fsums'][:, 5:].any() and a['fsums'].tobytes() == b['fsums'].tobytes()


def test_refusals_come_before_any_launch_and_leave_the_handle_as_it_was(case_a):
    nat, dev, D, x, y = case_a
    w = np.full(130, 0.25)
    before = dev.sgs_sums(EDGES_A, None, None, w, None, BIG)
    only = dev.sgs_sums(EDGES_A)                                  # max_work <= 0: the work only
    assert only['work'] == before['work'] > 0 and only['isums'] is None
    assert dev.sgs_sums(EDGES_A, max_work=-5)['work'] == before['work']
    exact = dev.sgs_sums(EDGES_A, None, None, w, None, before['work'])
    assert exact['fsums'].tobytes() == before['fsums'].tobytes()
    with pytest.raises(nat.GnxError, match='exceed max_work = %d' % (before['work'] - 1)):
        dev.sgs_sums(EDGES_A, None, None, w, None, before['work'] - 1)
    for bad in ([0.0, 2.0, 2.0], [1.0, 0.5], [-1.0, 2.0], [0.0, np.inf], [0.0, np.nan, 3.0]):
        with pytest.raises(nat.GnxError, match='edges'):
            dev.sgs_sums(np.array(bad), None, None, w, None, BIG)
    with pytest.raises(nat.GnxError, match='distance classes'):
        dev.sgs_sums(np.array([1.0]), None, None, w, None, BIG)
    with pytest.raises(nat.GnxError, match='distance classes'):
        dev.sgs_sums(np.arange(34.0), None, None, w, None, BIG)
    for bad in (131, -1, 2 ** 31 - 1):
        p = np.arange(131, dtype=np.int32)
        p[77] = bad
        with pytest.raises(nat.GnxError, match=r'perm\[77\]'):
            dev.sgs_sums(EDGES_A, None, None, w, p, BIG)
    with pytest.raises(nat.GnxError, match='slot out of range'):
        dev.sgs_sums(EDGES_A, np.array([0, dev.N]), None, w, None, BIG)
    with pytest.raises(nat.GnxError, match='2\\^24'):
        dev.sgs_sums(EDGES_A, np.zeros(0, np.int64), None, w, None, BIG)
    with pytest.raises(ValueError, match='perm'):
        dev.sgs_sums(EDGES_A, None, None, w, np.arange(130, dtype=np.int32), BIG)
    with pytest.raises(ValueError, match='locus_weight'):
        dev.sgs_sums(EDGES_A, None, None, np.zeros(131), None, BIG)
    after = dev.sgs_sums(EDGES_A, None, None, w, None, BIG)
    np.testing.assert_array_equal(after['isums'], before['isums'])
    assert after['fsums'].tobytes() == before['fsums'].tobytes()
    empty = nat.Device(16, 16, 1, L=96, cap_inds=256, cap_rows=256, seed=1)
    empty.upload_rasters(np.ones((1, 16, 16), np.float32))
    empty.set_species_params(nat.default_species_params())
    empty.upload_population(np.ones(10), np.ones(10), np.zeros(10), np.zeros(10), np.arange(10))
    with pytest.raises(nat.GnxError, match='genomes not assigned'):
        empty.sgs_sums(EDGES_A, max_work=BIG)
    empty.close()
    tile = _handle(nat, D[:10], np.ones(10), np.ones(10), np.arange(10), np.ones((1, 20, 24)))
    rec = np.zeros(1, nat.IND_REC)
    rec['x'], rec['y'], rec['id'] = 1.0, 1.0, 10 ** 6
    tile.tile_import_ghosts(rec)
    with pytest.raises(nat.GnxError, match='ghost records'):
        tile.sgs_sums(EDGES_A, np.arange(10, dtype=np.int64), max_work=BIG)
    tile.close()


# ------------------------------------------------------------------ the public call
def _walked_model(seed):
    """a few main steps with mutation on: genome blocks are shared between parents and
    offspring, and the population is not compacted when the analysis is asked for"""
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    p = small_params(seed=seed, L=100)
    p['comm']['species']['spp_0']['gen_arch']['mu_neut'] = 2e-4   # (the expected mutations must fit the neutral loci)
    mod = gnx.make_model(p)
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(4, 'main', verbose=False)
    return mod


def _state(mod):
    return (np.array([*mod.comm[0]]).tobytes(), mod.get_genotypes(biallelic=True).tobytes(),
            mod.get_x().tobytes(), mod.get_y().tobytes())


def test_model_calc_spatial_structure_after_real_steps_changes_nothing():
    a, b = _walked_model(6), _walked_model(6)
    edges = np.array([0.5, 1.5, 3.0, 5.0, 7.5])
    seed = 2
    res = a.calc_spatial_structure(edges=edges, nperm=19, seed=seed)
    assert _state(a) == _state(b)
    # the oracle on what the accessors download, in ascending-id order
    D = np.rint(a.get_genotypes() * 2).astype(np.int64)
    xy = a.get_coords()
    x, y = xy[:, 0].astype(np.float32), xy[:, 1].astype(np.float32)
    assert (x.astype(xy.dtype) == xy[:, 0]).all()
    n = D.shape[0]
    assert res['n'] == n and (res['ids'] == np.array([*a.comm[0]])).all()
    want = O.explicit_stats(x, y, D, edges)
    assert (res['pairs'] == want['pairs']).all() and (res['pairs'] > 0).all()
    assert res['n_zero'] == (O.pair_geometry(x, y, edges)[3] == -2).sum()
    worst = max(close(res[k], want[k], k)
                for k in ('mean_r', 'mean_lnr', 'F', 'dist2', 'slope', 'F1', 'Sp', 'Nb'))
    print('model: n = %d, pairs %s: worst relative error %.3g' % (n, res['pairs'].tolist(), worst))
    rows = M.draw_row_shuffles(n, 19, seed=seed)
    per = [O.explicit_stats(x, y, O.permuted(D, r), edges) for r in rows]
    pb, pF = np.array([p['slope'] for p in per]), np.stack([p['F'] for p in per])
    close(res['perm_slope'], pb, 'perm_slope')
    close(res['perm_F'], pF, 'perm_F')
    centre = pF.mean(axis=0)
    dev_p, dev_o = np.abs(pF - centre), np.abs(want['F'] - centre)
    assert np.abs(pb - want['slope']).min() > GAP * abs(want['slope'])
    assert (np.abs(dev_p - dev_o).min(axis=0) > GAP * dev_o).all()
    assert res['p_slope'] == (1 + (pb <= want['slope']).sum()) / 20
    assert (res['p_F'] == (1 + (dev_p >= dev_o).sum(axis=0)) / 20).all()
    # a request above max_work is refused with advice
    with pytest.raises(ValueError, match='exceed max_work = 10.*n=.*loci=.*max_dist'):
        a.calc_spatial_structure(edges=edges, max_work=10)
    # ... none of which consumed a draw of the device or changed a genome: the twin, which
    # was never analysed, walks on identically
    for step in range(2):
        a.walk(1, 'main', verbose=False)
        b.walk(1, 'main', verbose=False)
        assert _state(a) == _state(b)
    sub = a.calc_spatial_structure(n=50, loci=np.arange(10, 90), n_classes=3, max_dist=6.0)
    assert sub['n'] == 50 and sub['pairs'].shape == (3,) and sub['work'] <= 50 * 49 // 2 * 2
