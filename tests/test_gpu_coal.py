"""Pairwise coalescence through the recorded pedigree on the device (csrc/gnx_coal.hip:
gnx_coal_times / gnx_coal_segments; Model.calc_tmrca, Model.calc_ibd) against the numpy
restatement (geonomics_amd/sim/coal.py, which tests/test_coal_host.py checks against the edge
rows and by hand).  Everything the device returns is an integer function of the MRCAs: every
comparison is integer equality.  The pedigrees are those of tests/test_gpu_lineage.py: fixture
G17's path sets `sparse` (L = 300: four full 64-locus tiles and a tail of 44), `homog` (L = 190)
and `free` (L = 64, exactly one tile), 36 overlapping generations.  With the last generation's 16
nodes at all loci 0.77 / 0.71 / 0.74 of the (pair, locus) cells coalesce and T spans 1..36; every
test on these pedigrees asserts that the coalesced share of that request lies in 0.5..0.95, so
that a kernel that returns all -1 or all hits cannot pass on an empty comparison.  (The requests
with ancestors of the sample, with few loci or with an age limit have other shares - they are
printed - and assert that both outcomes occur; the model of the API test, a few hundred founders
14 steps back, coalesces in few cells, and asserts that some do.)"""
import numpy as np
import pytest

from geonomics_amd.sim import coal as CO

pytestmark = pytest.mark.gpu

BIG = 1 << 40
TEDGES = [2, 4, 8, 16, 30, 36]            # T = 1 and T = 36 fall outside: both ends are tested


def _pedigree(tag):
    from test_gpu_lineage import _device_for
    from test_lineage_host import make_pedigree
    dev, L, bp_off, bp_loci = _device_for(tag)
    tt, t_curr, last = make_pedigree(bp_off, bp_loci, L, n_founders=10, n_gen=36, per_gen=8,
                                     seed=3)
    return dev, L, tt, t_curr, last


def _nodes_of(tt, ids):
    rows = np.searchsorted(tt.ids, ids)
    return np.stack([2 * rows, 2 * rows + 1], 1).ravel()


def _share(ref):
    return ref['locus_cnt'].sum() / float(ref['work'])


def _assert_times_equal(got, ref, keys):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(got[k], ref[k], k)
    assert got['work'] == ref['work']


ALL_TIMES = ('pair_sum', 'pair_cnt', 'locus_sum', 'locus_cnt', 'locus_max', 'mrca')


@pytest.mark.parametrize('tag', ['sparse', 'homog', 'free'])
def test_coal_times_equal_the_restatement(tag):
    dev, L, tt, t_curr, last = _pedigree(tag)
    tab, bt = tt.node_table()
    rng = np.random.RandomState(7)
    young = _nodes_of(tt, last)
    # (b): with both nodes of five ancestors of the sample, so that an MRCA is a sample node
    mixed = rng.permutation(np.concatenate([young, _nodes_of(tt, tt.ids[40:45])]))
    requests = ((young, np.arange(L)),                               # (a)
                (mixed, rng.permutation(L)[:37]),                    # (b)
                (young, np.array([L - 1, 0, 5, 5, 3])))              # (c) a repeated locus
    for k, (nodes, loci) in enumerate(requests):
        for max_ago in (None, 20):
            ref = CO.coal_times_np(tab, bt, tt, nodes, loci, t_curr,
                                   -1 if max_ago is None else max_ago, TEDGES)
            got = dev.coal_times(tab, bt, nodes, loci, t_curr, max_ago, TEDGES, ALL_TIMES, BIG)
            _assert_times_equal(got, ref, ALL_TIMES + ('thist',))
            assert dev.lineage_info()['launches'] == 2               # the walk and the mirror
            print('%s request %d, max_ago %s: %.2f of %d cells coalesce, thist %s'
                  % (tag, k, max_ago, _share(ref), ref['work'], ref['thist'].tolist()))
            if max_ago is None:
                # (a) is the request the share was measured on (0.77 / 0.71 / 0.74 for the three
                # path sets); with the five ancestors of (b) it is 0.35 .. 0.40 and at the five
                # loci of (c) 0.44 .. 0.86, measured with the restatement: both outcomes occur
                if k == 0:
                    assert 0.5 <= _share(ref) <= 0.95
                    assert ref['thist'].sum() < ref['locus_cnt'].sum()   # T = 1 or 36 occurs
                else:
                    assert 0 < _share(ref) < 1
                if k == 1:
                    assert np.isin(ref['mrca'], nodes).any()
                unlimited = _share(ref)
            else:
                # the limit takes the older MRCAs away and leaves the younger ones
                assert 0 < _share(ref) < unlimited
    nodes, loci = requests[0]
    ref = CO.coal_times_np(tab, bt, tt, nodes, loci, t_curr, 20, TEDGES)
    # only some outputs: the others are not computed
    got = dev.coal_times(tab, bt, nodes, loci, t_curr, 20, None, ('pair_cnt',), BIG)
    assert sorted(got) == ['pair_cnt', 'work']
    np.testing.assert_array_equal(got['pair_cnt'], ref['pair_cnt'])
    got = dev.coal_times(tab, bt, nodes, loci, t_curr, 20, TEDGES, (), BIG)
    assert sorted(got) == ['thist', 'work']
    np.testing.assert_array_equal(got['thist'], ref['thist'])
    assert dev.lineage_info()['launches'] == 1
    got = dev.coal_times(tab, bt, nodes, loci, t_curr, 20, None, ('locus_max', 'mrca'), BIG)
    assert sorted(got) == ['locus_max', 'mrca', 'work']
    _assert_times_equal(got, ref, ('locus_max', 'mrca'))
    # a byte budget that holds the MRCAs of 7 loci: several launches, the same result
    if L > 64:
        dev.lineage_budget(7 * 4 * CO.n_pairs(nodes.size))
        got = dev.coal_times(tab, bt, nodes, loci, t_curr, 20, TEDGES, ALL_TIMES, BIG)
        assert dev.lineage_info()['launches'] == (L + 6) // 7 + 1
        _assert_times_equal(got, ref, ALL_TIMES + ('thist',))
        dev.lineage_budget(0)
    # the table went up once
    assert dev.lineage_info()['uploaded'] is False
    dev.close()


@pytest.mark.parametrize('tag', ['sparse', 'homog'])
def test_coal_segments_equal_the_restatement(tag):
    dev, L, tt, t_curr, last = _pedigree(tag)
    tab, bt = tt.node_table()
    nodes = _nodes_of(tt, last)
    rng = np.random.RandomState(11)
    maps = (np.arange(L, dtype=np.int64), np.cumsum(rng.randint(0, 5, L)).astype(np.int64))
    brk = (rng.rand(L) < 0.05).astype(np.uint8)
    brk[64] = 0                                      # (segments may run from tile 0 into tile 1)
    edges = [0, 1, 4, 16, 64, 1 << 40]
    all_loci = np.arange(L)
    raw = CO.coal_mrca_np(tab, bt, tt, nodes, all_loci)
    assert 0.5 <= (raw >= 0).mean() <= 0.95
    carried = 0
    for pos in maps:
        for b in (None, brk):
            for min_loci in (1, 5):
                for max_ago in (None, 20):
                    ma = -1 if max_ago is None else max_ago
                    ref = CO.coal_segments_np(tab, bt, tt, nodes, all_loci, pos, b, t_curr, ma,
                                              min_loci, 3 if min_loci == 5 else 0, edges, True)
                    got = dev.coal_segments(tab, bt, nodes, all_loci, pos, t_curr, b, max_ago,
                                            min_loci, 3 if min_loci == 5 else 0, edges, True,
                                            BIG)
                    for k in ('cnt', 'len', 'longest', 'hist', 'cover'):
                        assert got[k].dtype == ref[k].dtype, k
                        np.testing.assert_array_equal(got[k], ref[k], k)
                    assert got['work'] == ref['work'] == 120 * L
                    assert ref['cnt'].sum() > 0 and (np.diagonal(got['cnt']) == 0).all()
                    # the carry from one tile of 64 list positions into the next is exercised
                    m, _ = CO.coal_mask(raw, bt, t_curr, ma)
                    _, s, e, _, _ = CO.segments_of(m.T, pos, b, min_loci,
                                                   3 if min_loci == 5 else 0)
                    assert ((s <= 63) & (e >= 64)).sum() >= 1
                    carried += int(((s <= 63) & (e >= 64)).sum())
    print('%s: %d qualifying segments span list positions 63 | 64' % (tag, carried))
    # a strided list (every 3rd locus), positions of the listed loci, without hist and cover
    loci = np.arange(0, L, 3)
    for pos, b in ((maps[1][loci], None), (maps[0][loci], brk[loci])):
        ref = CO.coal_segments_np(tab, bt, tt, nodes, loci, pos, b, t_curr, -1, 2, 0)
        got = dev.coal_segments(tab, bt, nodes, loci, pos, t_curr, b, None, 2, 0, None, False, BIG)
        for k in ('cnt', 'len', 'longest'):
            np.testing.assert_array_equal(got[k], ref[k], k)
        assert got['hist'] is None and got['cover'] is None and ref['cnt'].sum() > 0
    assert dev.lineage_info()['launches'] == 1 and dev.lineage_info()['uploaded'] is False
    dev.close()


def test_refusals_leave_the_handle_as_it_was():
    from test_gpu_parity import native
    nat = native()
    dev, L, tt, t_curr, last = _pedigree('sparse')
    tab, bt = tt.node_table()
    nodes = _nodes_of(tt, last)
    loci = np.arange(L)
    pos = np.arange(L, dtype=np.int64)
    want = tt.trace(nodes, loci[:70], t_curr)
    ok = dev.coal_times(tab, bt, nodes, loci, t_curr, None, None, ('pair_cnt',), BIG)['pair_cnt']
    np.testing.assert_array_equal(ok, CO.coal_times_np(tab, bt, tt, nodes, loci, t_curr)['pair_cnt'])
    assert 0.5 <= ok.sum() / 2.0 / (120 * L) <= 0.95

    def times(n=nodes, l=loci, **kw):
        a = dict(max_time_ago=None, time_edges=None, want=('pair_cnt',), max_work=BIG)
        a.update(kw)
        return dev.coal_times(tab, bt, n, l, t_curr, **a)

    def segs(n=nodes, l=loci, p=pos, **kw):
        a = dict(max_work=BIG)
        a.update(kw)
        return dev.coal_segments(tab, bt, n, l, p, t_curr, **a)

    dup = nodes.copy()
    dup[5] = dup[2]
    for call, msg in (
            (lambda: times(n=dup), 'listed twice'), (lambda: segs(n=dup), 'listed twice'),
            (lambda: times(n=nodes[:1]), r'2\.\.4096 sample nodes'),
            (lambda: segs(n=nodes[:1]), r'2\.\.4096 sample nodes'),
            (lambda: times(n=np.r_[nodes[:3], 2 * bt.size]), 'sample node'),
            (lambda: times(l=[0, L]), 'locus'), (lambda: segs(l=[0, L], p=[0, 1]), 'locus'),
            (lambda: segs(l=[5, 4, 9], p=[0, 1, 2]), 'strictly ascending'),
            (lambda: segs(l=[4, 4, 9], p=[0, 1, 2]), 'strictly ascending'),
            (lambda: segs(l=[3, 4, 9], p=[0, 2, 1]), 'non-decreasing'),
            (lambda: segs(min_len=-1), 'min_len'),
            (lambda: segs(edges=[0, 5, 5]), 'edges'), (lambda: segs(edges=[3]), 'edges'),
            (lambda: times(time_edges=[4, 2]), 'time edges'),
            (lambda: times(max_work=120 * L - 1), 'exceed max_work'),
            (lambda: segs(max_work=120 * L - 1), 'exceed max_work')):
        with pytest.raises(nat.GnxError, match=msg):
            call()
    with pytest.raises(ValueError, match='max_time_ago'):
        times(max_time_ago=-1)
    with pytest.raises(ValueError, match='pos'):
        segs(p=pos[:-1])
    with pytest.raises(ValueError, match='unknown output'):
        times(want=('tmrca',))
    # max_work <= 0: only the work is written
    assert times(max_work=0) == dict(work=120 * L)
    assert segs(max_work=0) == dict(work=120 * L, cnt=None, len=None, longest=None, hist=None,
                                    cover=None)
    assert times(max_work=120 * L)['work'] == 120 * L          # exactly the limit is taken
    # after all these the handle answers as before, the resident table included
    got = dev.lineage_trace(tab, bt, nodes, loci[:70], t_curr)
    for k in ('root', 'first', 'last', 'n_kept'):
        np.testing.assert_array_equal(got[k], want[k], k)
    assert dev.lineage_info()['uploaded'] is False
    np.testing.assert_array_equal(times()['pair_cnt'], ok)
    dev.close()
    # a handle without paths, as the lineage calls
    from test_gpu_parity import make_dev
    bare = make_dev(16, 16, L=0, cap=1024)
    with pytest.raises(nat.GnxError, match='genomes not assigned'):
        bare.coal_times(tab, bt, nodes, [0], t_curr, max_work=BIG)
    bare.close()


# ------------------------------------------------------------------ the public calls
def _coal_model(steps):
    """the model of the lineage and simplification API tests, with a recombination rate below
    free recombination (segments longer than one locus) and - the default - no mutation"""
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    p = small_params(seed=8, traits=True, L=56, T=steps)
    ga = p['comm']['species']['spp_0']['gen_arch']
    ga['use_tskit'] = True
    ga['tskit_simp_interval'] = 10
    ga['r_distr_alpha'] = 0.02
    assert not ga['mu_neut'] and not ga['mu_delet']
    mod = gnx.make_model(p)
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(steps, 'main', verbose=False)
    return mod, mod.comm[0]


def _by_individual(res, tt):
    """(individual id, homologue) of a calc_tmrca result's nodes"""
    return tt.ids[res['nodes'] >> 1], res['nodes'] & 1


def test_model_calc_tmrca_and_calc_ibd():
    from geonomics_amd.sim import tracts as TR
    from geonomics_amd.structs.tiled import TiledSpecies
    mod, spp = _coal_model(14)                       # simplified after step 9, four steps since
    tt = spp._tt
    ids = np.array([*spp])
    some = ids[::6]
    tab, bt = tt.node_table()
    nodes = _nodes_of(tt, some)
    L = spp.gen_arch.L
    # ---- calc_tmrca
    te = [1, 2, 4, 8, 16]
    res = mod.calc_tmrca(individs=some, time_edges=te, n_classes=4, max_dist=12.0,
                         groups=(np.arange(ids.size) % 3 - (np.arange(ids.size) % 5 == 0)),
                         return_mrca=True)
    assert sorted(res) == sorted(['ids', 'nodes', 'loci', 'tmrca', 'n_coalesced', 'per_locus',
                                  'diversity_branch', 'by_group', 'by_dist', 'coal_times',
                                  'share_coalesced', 'mrca', 'work'])
    ref = CO.coal_times_np(tab, bt, tt, nodes, np.arange(L), spp.t, -1, [0] + te)
    print('model: %d living, %d sampled, %d rows, %d of %d cells coalesce'
          % (ids.size, some.size, bt.size, ref['locus_cnt'].sum(), ref['work']))
    # (a few hundred founders a few steps back: most pairs do not coalesce inside the tables, so
    # the share is small here; the synthetic pedigrees above are where both outcomes are common)
    assert 0 < ref['locus_cnt'].sum() < ref['work']
    np.testing.assert_array_equal(res['ids'], some)
    np.testing.assert_array_equal(res['nodes'], nodes)
    np.testing.assert_array_equal(res['loci'], np.arange(L))
    np.testing.assert_array_equal(res['mrca'], ref['mrca'])
    np.testing.assert_array_equal(res['n_coalesced'], ref['pair_cnt'])
    tm, per, share = CO.tmrca_stats(ref['pair_sum'], ref['pair_cnt'], ref['locus_sum'],
                                    ref['locus_cnt'], ref['locus_max'])
    np.testing.assert_array_equal(res['tmrca'], tm)                     # NaN == NaN here
    assert res['tmrca'].dtype == np.float64 and np.isnan(np.diagonal(res['tmrca'])).all()
    for k in ('mean', 'share_coalesced', 'max'):
        np.testing.assert_array_equal(res['per_locus'][k], per[k])
    assert res['share_coalesced'] == share == _share(ref) and res['work'] == ref['work']
    rate = CO.coal_rate(ref['thist'][1:], te, ref['work'], ref['thist'][0])
    for k in ('edges', 'counts', 'at_risk', 'ne'):
        np.testing.assert_array_equal(res['coal_times'][k], rate[k])
    assert rate['at_risk'][0] == ref['work'] - ref['thist'][0]
    i, j = np.triu_indices(nodes.size, 1)
    assert res['diversity_branch'] == 2.0 * ref['pair_sum'][i, j].sum() / ref['pair_cnt'][i, j].sum()
    label = (np.arange(ids.size) % 3 - (np.arange(ids.size) % 5 == 0))[::6]
    div, grp = CO.branch_diversity(ref['pair_sum'], ref['pair_cnt'],
                                   [np.flatnonzero(np.repeat(label, 2) == g) for g in range(3)])
    assert res['by_group']['names'] == [0, 1, 2] and div == res['diversity_branch']
    np.testing.assert_array_equal(res['by_group']['within'], grp['within'])
    np.testing.assert_array_equal(res['by_group']['between'], grp['between'])
    rows = np.searchsorted(ids, some)
    by = CO.tmrca_by_distance(mod.get_x()[rows], mod.get_y()[rows], ref['pair_sum'],
                              ref['pair_cnt'], L, res['by_dist']['edges'])
    for k in ('pairs', 'mean_tmrca', 'share_coalesced', 'mean_dist'):
        np.testing.assert_array_equal(res['by_dist'][k], by[k])
    assert by['pairs'].sum() > 10
    # a limit, a locus subset, the defaults of the histogram
    sub = mod.calc_tmrca(individs=some, loci=[5, 50, 3], max_time_ago=6)
    ref6 = CO.coal_times_np(tab, bt, tt, nodes, [5, 50, 3], spp.t, 6)
    np.testing.assert_array_equal(sub['n_coalesced'], ref6['pair_cnt'])
    assert sub['mrca'] is None and sub['by_group'] is None
    assert sub['coal_times']['edges'].tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    assert sub['coal_times']['counts'].sum() == ref6['locus_cnt'].sum()
    # ---- calc_ibd
    rates = np.zeros(L)
    rec = spp.gen_arch.recombinations
    rates[rec._positions] = rec._rates
    pos, brk, glen = TR.tract_map(rates, 'morgans')
    assert not brk.any() and glen > 0
    ibd = mod.calc_ibd(individs=some, min_len=0, min_loci=1, n_classes=4, max_dist=12.0,
                       tract_edges=[0.0, 0.2, np.inf], cover=True)
    assert sorted(ibd) == sorted(['ids', 'n_tracts', 'shared_len', 'longest', 'by_dist', 'hist',
                                  'cover', 'work', 'unit', 'f_ibd', 'genome_len'])
    refs = CO.coal_segments_np(tab, bt, tt, nodes, np.arange(L), pos, brk, spp.t, -1, 1, 0,
                               [0, TR.to_units(0.2, 'morgans'), TR.INT64_MAX], True)
    cnt, tot, longest = CO.fold_to_individuals(refs['cnt'], refs['len'], refs['longest'])
    np.testing.assert_array_equal(ibd['n_tracts'], cnt)
    np.testing.assert_array_equal(ibd['shared_len'], tot / 2 ** 32)
    np.testing.assert_array_equal(ibd['longest'], longest / 2 ** 32)
    np.testing.assert_array_equal(ibd['hist']['tracts'], refs['hist'][:, 0])
    np.testing.assert_array_equal(ibd['cover'], refs['cover'])
    np.testing.assert_array_equal(ibd['f_ibd'], np.diagonal(tot) / glen)
    assert ibd['genome_len'] == glen / 2 ** 32 and ibd['work'] == refs['work']
    assert ibd['unit'] == 'morgans' and cnt.sum() > 0
    want = TR.sharing_stats(mod.get_x()[rows], mod.get_y()[rows], cnt, tot,
                            ibd['by_dist']['edges'])
    np.testing.assert_array_equal(ibd['by_dist']['pairs'], want['pairs'])
    np.testing.assert_array_equal(ibd['by_dist']['mean_len'], want['mean_len'] / 2 ** 32)
    dflt = mod.calc_ibd(individs=some, max_time_ago=8)
    refd = CO.coal_segments_np(tab, bt, tt, nodes, np.arange(L), pos, brk, spp.t, 8, 50,
                               TR.to_units(0.02, 'morgans'))
    np.testing.assert_array_equal(dflt['n_tracts'], CO.fold_to_individuals(
        refd['cnt'], refd['len'], refd['longest'])[0])
    assert dflt['hist'] is None and dflt['cover'] is None
    # descent implies state where no mutation has hit the segment, and this model runs with
    # mutation off: an individual's two haplotypes are identical wherever they are identical by
    # descent, so its realised autozygosity is at most its F_ROH at the same thresholds and unit
    roh = mod.calc_roh(individs=some, min_len=0, min_loci=1)
    assert (ibd['f_ibd'] <= roh['f_roh']).all()
    print('f_ibd: mean %.4f, max %.4f; f_roh: mean %.4f'
          % (ibd['f_ibd'].mean(), ibd['f_ibd'].max(), roh['f_roh'].mean()))
    # ---- an extra simplification renumbers the nodes and changes nothing else
    who = _by_individual(res, tt)
    hit = res['mrca'] >= 0
    anc = tt.ids[np.maximum(res['mrca'], 0) >> 1].copy(), res['mrca'] & 1
    n_rows = tt.ids.size
    before, after = spp._sort_and_simplify_table_collection()
    assert before == n_rows and after < before
    res2 = mod.calc_tmrca(individs=some, time_edges=te, n_classes=4, max_dist=12.0,
                          return_mrca=True)
    for a, b in zip(who, _by_individual(res2, spp._tt)):
        np.testing.assert_array_equal(a, b)
    assert (res2['nodes'] != res['nodes']).any()
    for k in ('tmrca', 'n_coalesced'):
        np.testing.assert_array_equal(res2[k], res[k])
    for k in ('edges', 'counts', 'at_risk', 'ne'):
        np.testing.assert_array_equal(res2['coal_times'][k], res['coal_times'][k])
    np.testing.assert_array_equal(res2['mrca'] >= 0, hit)
    # the same ancestors, by (individual id, homologue)
    np.testing.assert_array_equal(spp._tt.ids[np.maximum(res2['mrca'], 0) >> 1][hit], anc[0][hit])
    np.testing.assert_array_equal((res2['mrca'] & 1)[hit], anc[1][hit])
    ibd2 = mod.calc_ibd(individs=some, min_len=0, min_loci=1, n_classes=4, max_dist=12.0,
                        tract_edges=[0.0, 0.2, np.inf], cover=True)
    for k in ('n_tracts', 'shared_len', 'longest', 'cover', 'f_ibd'):
        np.testing.assert_array_equal(ibd2[k], ibd[k])
    np.testing.assert_array_equal(ibd2['hist']['tracts'], ibd['hist']['tracts'])
    # ---- refusals
    dead = np.setdiff1d(spp._tt.ids, ids)[-1:]
    for f in (mod.calc_tmrca, mod.calc_ibd):
        with pytest.raises(ValueError, match='not alive'):
            f(individs=np.r_[some[:3], dead])
        with pytest.raises(ValueError, match='exceed max_work = 1.*max_work'):
            f(individs=some, max_work=1)
        with pytest.raises(ValueError, match='max_time_ago'):
            f(individs=some, max_time_ago=-2)
    with pytest.raises(ValueError, match='time_edges'):
        mod.calc_tmrca(individs=some, time_edges=[3, 3])
    for name in ('_calc_tmrca', '_calc_ibd'):
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            getattr(TiledSpecies, name)(object())


def test_species_without_a_pedigree_is_refused():
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    mod = gnx.make_model(small_params(T=3, L=16))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(3, 'main', verbose=False)
    for f in (mod.calc_tmrca, mod.calc_ibd):
        with pytest.raises(ValueError, match='no pedigree was recorded'):
            f()
