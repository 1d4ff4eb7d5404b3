"""Simplification of the recorded pedigree on the device (csrc/gnx_simplify.hip:
gnx_pedigree_reach / gnx_lineage_forget; Species._sort_and_simplify_table_collection and the
tskit_simp_interval of Model._do_timestep) against the host recurrence
(TreeTables.ancestral_masks, which tests/test_simplify_host.py checks against the marking of
every lineage chain and by hand).  Everything compared is integers or bits: equality is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _pack(masks, W64):
    """bool [n][L] -> uint64 [n][W64] in the layout of the recombination paths"""
    n, L = masks.shape
    bits = np.zeros((n, W64 * 64), np.uint8)
    bits[:, :L] = masks
    return np.packbits(bits, axis=1, bitorder='little').view('<u8').astype(np.uint64)


def _assert_reach_equals_host(dev, tt, rows, budget=0):
    """node_loci and the masks of every node equal the host's, bit for bit -> launches"""
    tab, bt = tt.node_table()
    want = tt.ancestral_masks(rows)
    dev.lineage_budget(budget)
    loci, masks = dev.pedigree_reach(tab, bt, rows, masks_of=np.arange(2 * bt.size))
    info = dev.lineage_info()
    dev.lineage_budget(0)
    assert loci.dtype == np.int32 and masks.dtype == np.uint64
    assert masks.shape == (2 * bt.size, dev.W64)
    np.testing.assert_array_equal(loci, want.sum(axis=1))
    np.testing.assert_array_equal(masks, _pack(want, dev.W64))      # (bits >= L are zero)
    np.testing.assert_array_equal(dev.pedigree_reach(tab, bt, rows), loci)
    return info['launches']


@pytest.mark.parametrize('tag', ['sparse', 'homog', 'free'])
def test_reach_equals_host_masks(tag):
    from test_gpu_lineage import _device_for
    from test_lineage_host import make_pedigree
    dev, L, bp_off, bp_loci = _device_for(tag)
    tt, t_curr, last = make_pedigree(bp_off, bp_loci, L, n_founders=10, n_gen=36, per_gen=8,
                                     seed=3)
    rows = np.searchsorted(tt.ids, last)
    n_rows, n_cohorts = tt.ids.size, 37
    one = _assert_reach_equals_host(dev, tt, rows)
    assert one == n_cohorts + 1                    # a launch per cohort, one for the masks
    # a budget of half the masks' bytes: the words go in two column blocks or more
    assert dev.W64 >= 4
    many = _assert_reach_equals_host(dev, tt, rows, budget=2 * n_rows * dev.W64 * 8 // 2)
    assert many >= 2 * n_cohorts
    # the smallest block there is (two words), and a subset of the nodes in an order of its own
    tab, bt = tt.node_table()
    dev.lineage_budget(1)
    req = np.random.RandomState(3).permutation(2 * n_rows)[:50]
    loci, masks = dev.pedigree_reach(tab, bt, rows[::-1].copy(), masks_of=req)
    assert dev.lineage_info()['launches'] >= (dev.W64 // 2) * n_cohorts
    want = tt.ancestral_masks(rows)
    np.testing.assert_array_equal(loci, want.sum(axis=1))
    np.testing.assert_array_equal(masks, _pack(want[req], dev.W64))
    dev.close()


def test_reach_with_two_word_groups():
    """L = 1100: 32 words per homologue (two groups of 16), the last 60 bits of word 17 and the
    words 18..31 beyond L"""
    import gnx_oracle as O
    from test_gpu_parity import make_dev
    from test_lineage_host import make_pedigree
    L, n_paths = 1100, 64
    rng = np.random.RandomState(21)
    cross = (rng.random_sample((n_paths, L)) < 3.0 / L).astype(np.uint8)
    cross[:, 0] = 0
    bp_off = np.concatenate([[0], np.cumsum(cross.sum(axis=1))]).astype(np.int64)
    bp_loci = np.nonzero(cross)[1].astype(np.int64)
    dev = make_dev(40, 40, L=L, cap=2048, seed=4, mating_radius=3.0, K_factor=1.0)
    assert dev.W64 == 32
    dev.set_recomb_paths(O.pack_bits(O.recomb_paths(cross)))
    dev.init_population(100)
    dev.assign_genomes(O.starting_mutation_counts(dev.N, np.full(L, 0.5)))
    tt, t_curr, last = make_pedigree(bp_off, bp_loci, L, 12, 40, 6, seed=3, window=3)
    rows = np.searchsorted(tt.ids, last)
    # the host masks are themselves what the lineages say (as tests/test_simplify_host.py)
    from test_simplify_host import brute_masks
    np.testing.assert_array_equal(tt.ancestral_masks(rows), brute_masks(tt, rows, t_curr))
    assert _assert_reach_equals_host(dev, tt, rows) == 42
    assert _assert_reach_equals_host(dev, tt, rows, budget=2 * tt.ids.size * 12 * 8) >= 3 * 41
    dev.close()


def _small_device():
    """the three paths of test_lineage_host.small_pedigree on a device with L = 8"""
    import gnx_oracle as O
    from test_gpu_parity import make_dev
    paths = np.zeros((3, 8), np.uint8)
    paths[1, 4] = 1
    paths[2, [2, 6]] = 1
    dev = make_dev(16, 16, L=8, cap=1024, seed=1)
    dev.set_recomb_paths(O.pack_bits(O.recomb_paths(paths)))
    dev.init_population(50)
    dev.assign_genomes(O.starting_mutation_counts(dev.N, np.full(8, 0.5)))
    return dev


def test_edge_cases_and_refusals_on_the_device():
    from geonomics_amd.structs.pedigree import TreeTables
    from geonomics_amd.structs.tiled import TiledSpecies
    from test_gpu_parity import native
    from test_lineage_host import small_pedigree
    nat = native()
    dev = _small_device()
    tt = small_pedigree()
    tab, bt = tt.node_table()
    # by hand (tests/test_simplify_host.py: test_small_pedigree_by_hand)
    want = {22: 8, 23: 8, 19: 8, 17: 8, 12: 8, 14: 4, 15: 4, 8: 8, 9: 8, 0: 8, 2: 4, 3: 4}
    loci, masks = dev.pedigree_reach(tab, bt, [11], masks_of=[14, 15, 1])
    assert loci.tolist() == [want.get(v, 0) for v in range(24)]
    assert masks[:, 0].tolist() == [0x0f, 0xf0, 0] and not masks[:, 1:].any()
    # everybody sampled; one founder sampled
    assert (dev.pedigree_reach(tab, bt, np.arange(12)) == 8).all()
    assert dev.pedigree_reach(tab, bt, [2]).tolist() == [0] * 4 + [8, 8] + [0] * 18
    # founders only
    ft = TreeTables(8, [0, 0, 1, 3], [4, 2, 6])
    ft.add_founders(np.arange(4), np.zeros((4, 2)))
    assert dev.pedigree_reach(*ft.node_table(), [3, 1]).tolist() == [0, 0, 8, 8, 0, 0, 8, 8]
    assert dev.lineage_info()['launches'] == 1
    # a step without births (tests/test_simplify_host.py: test_a_step_without_births)
    gt = TreeTables(8, [0, 0, 1, 3], [4, 2, 6])
    gt.add_founders(np.arange(3), np.zeros((3, 2)))
    gt.add_births(0, [3, 4], [(0, 1), (1, 1)], [(1, 0), (2, 0)], [(0, 0), (1, 0)],
                  np.zeros((2, 2)))
    gt.add_births(2, [5], [(3, 3)], [(0, 1)], [(0, 1)], np.zeros((1, 2)))
    assert dev.pedigree_reach(*gt.node_table(), [5]).tolist() == \
        [4, 4, 4, 0, 0, 0, 8, 4, 0, 0, 8, 8]
    assert dev.lineage_info()['launches'] == 3
    _assert_reach_equals_host(dev, gt, [5])
    # refusals: nothing is launched
    ok = dev.pedigree_reach(tab, bt, [11])
    up = bt.copy()
    up[7] = 0                               # 1 1 1 1 0 0 -1 -1 -2 ... -> 1 1 1 1 0 0 -1 0 -2 ...
    par = tab.copy()
    par[18, 0] = 8                                          # row 9's parent of its own cohort
    for args, kw, msg in (((tab, bt, [11, 3, 11]), {}, 'listed twice'),
                          ((tab, bt, [12]), {}, 'sample row'),
                          ((tab, bt, [-1]), {}, 'sample row'),
                          ((tab, bt, []), {}, 'at least one'),
                          ((tab, up, [11]), {}, 'must not ascend'),
                          ((par, bt, [11]), {}, 'parent row'),
                          ((tab, bt, [11]), dict(masks_of=[24]), 'requested node'),
                          ((tab, bt, [11]), dict(masks_of=[0, -1]), 'requested node')):
        with pytest.raises(nat.GnxError, match=msg):
            dev.pedigree_reach(*args, **kw)
        assert dev.lineage_info()['launches'] == 0
    with pytest.raises(ValueError):
        dev.pedigree_reach(tab, bt[:-1], [11])
    np.testing.assert_array_equal(dev.pedigree_reach(tab, bt, [11]), ok)
    dev.close()
    with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
        TiledSpecies._sort_and_simplify_table_collection(object())


def test_forget_makes_the_next_lineage_call_upload():
    from test_lineage_host import small_pedigree
    dev = _small_device()
    tt = small_pedigree()
    tab, bt = tt.node_table()
    dev.lineage_trace(tab, bt, [22], [0], 3)
    assert dev.lineage_info()['uploaded'] is True
    dev.pedigree_reach(tab, bt, [11])
    assert dev.lineage_info()['uploaded'] is False           # the resident copy serves both
    dev.lineage_forget()
    dev.lineage_trace(tab, bt, [22], [0], 3)
    assert dev.lineage_info()['uploaded'] is True            # the very same table again
    # simplify, then births until the row count is what it was
    tt.simplify([11], dev.pedigree_reach(tab, bt, [11]))
    dev.lineage_forget()
    tt.add_births(4, [12, 13, 14, 15], [(11, 11)] * 4, [(0, 1)] * 4, [(0, 1)] * 4,
                  np.zeros((4, 2)))
    tab2, bt2 = tt.node_table()
    assert bt2.size == bt.size
    got = dev.lineage_trace(tab2, bt2, [22, 23], [0, 5], 4, drop_before_sim=False)
    assert dev.lineage_info()['uploaded'] is True
    want = tt.trace([22, 23], [0, 5], 4, drop_before_sim=False)
    for k in ('root', 'first', 'last', 'n_kept'):
        np.testing.assert_array_equal(got[k], want[k])
    dev.close()


def _simp_model(T, interval):
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    p = small_params(seed=8, traits=True, L=56, T=T)
    ga = p['comm']['species']['spp_0']['gen_arch']
    ga['use_tskit'] = True
    ga['mu_neut'] = 1e-4
    ga['tskit_simp_interval'] = interval
    mod = gnx.make_model(p)
    mod.walk(10000, 'burn', verbose=False)
    return mod, mod.comm[0]


def test_model_simplifies_at_its_interval(tmp_path):
    from geonomics_amd.structs import pedigree as P
    T = 40
    full_mod, full = _simp_model(T, None)
    full_mod.walk(T, 'main', verbose=False)
    mod, spp = _simp_model(T, 10)
    founders = spp._tt.n_founders
    rows = [spp._tt.ids.size]
    dropped_at = []
    for t in range(T):
        mod.walk(1, 'main', verbose=False)
        assert mod.t == t
        grown = rows[-1] + spp.n_births[-1]
        rows.append(spp._tt.ids.size)
        assert rows[-1] <= grown
        if rows[-1] < grown:
            dropped_at.append(t)
    assert dropped_at == [9, 19, 29, 39]            # (t + 1) % 10 == 0, and only then
    births = sum(spp.n_births[-T:])
    print('model: %d founders + %d births = %d rows unsimplified, %d simplified; %d living'
          % (founders, births, full._tt.ids.size, rows[-1], len(spp)))
    assert full._tt.ids.size == founders + births and rows[-1] < founders + births
    # the simulation itself is what it was
    ids = np.array([*spp])
    np.testing.assert_array_equal(ids, np.array([*full]))
    assert spp.Nt == full.Nt
    g = spp._get_genotypes()
    np.testing.assert_array_equal(g, full._get_genotypes())
    # and so is everything read from the pedigree for the living
    np.testing.assert_array_equal(spp._tt.genotypes_of(ids), g)
    co = spp._check_coalescence()
    assert spp._dev.lineage_info()['uploaded'] is True       # first call since the last pass
    assert co == full._check_coalescence()
    assert spp._check_coalescence(all_loci=True) == full._check_coalescence(all_loci=True)
    a = spp._calc_lineage_stats(as_arrays=True)
    b = full._calc_lineage_stats(as_arrays=True)
    np.testing.assert_array_equal(a['loci'], b['loci'])
    assert a['nodes'].shape == b['nodes'].shape
    np.testing.assert_array_equal(spp._tt.ids[a['nodes'] >> 1], full._tt.ids[b['nodes'] >> 1])
    for st in P.LINEAGE_STATS:
        np.testing.assert_array_equal(a[st], b[st])         # NaN == NaN here
    assert (~np.isnan(a['time'])).mean() >= 0.5
    mod.write_tskit_table_collection(str(tmp_path / 'simp'))
    with open(str(tmp_path / 'simp.individuals.txt')) as f:
        assert len(f.readlines()) == rows[-1] + 1
    # by hand once more: rows before / after, and a pass right after a pass drops nothing
    n = spp._tt.ids.size
    assert spp._sort_and_simplify_table_collection() == (n, n)
    # no pedigree: the error of write_tskit_table_collection
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    plain = gnx.make_model(small_params(T=3, L=16))
    plain.walk(10000, 'burn', verbose=False)
    plain.walk(3, 'main', verbose=False)
    with pytest.raises(ValueError, match='no pedigree was recorded'):
        plain.comm[0]._sort_and_simplify_table_collection()
