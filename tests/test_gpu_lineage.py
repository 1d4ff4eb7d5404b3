"""Lineages through the recorded pedigree on the device (csrc/gnx_lineage.hip:
gnx_lineage_trace / gnx_lineage_chains; Species._get_lineage_dicts, _calc_lineage_stats,
_check_coalescence) against the host walk (TreeTables.trace / lineages, which
tests/test_lineage_host.py checks against the edge rows and by hand).  Everything compared
here is integer node ids, or floats computed on the host from the same ids: equality is exact."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _device_for(tag, cap=2048, n=200, seed=4):
    """a Device with fixture G17's path set `tag` uploaded and genomes assigned"""
    import gnx_oracle as O
    from test_gpu_parity import make_dev
    g = load_golden('g17_pedigree_segments')
    L = int(g[tag + '_L'][0])
    bp_off, bp_loci = g[tag + '_bp_off'], g[tag + '_bp_loci']
    n_paths = bp_off.size - 1
    cross = np.zeros((n_paths, L), np.uint8)
    for k in range(n_paths):
        cross[k, bp_loci[bp_off[k]:bp_off[k + 1]]] = 1
    dev = make_dev(40, 40, L=L, cap=cap, seed=seed, mating_radius=3.0, K_factor=1.0)
    dev.set_recomb_paths(O.pack_bits(O.recomb_paths(cross)))
    dev.init_population(n)
    dev.assign_genomes(O.starting_mutation_counts(dev.N, np.full(L, 0.5)))
    return dev, L, bp_off, bp_loci


def _assert_trace_equal(got, want, nodes_sl=slice(None), loci_sl=slice(None)):
    for k in ('root', 'first', 'last', 'n_kept'):
        assert got[k].dtype == np.int32
        np.testing.assert_array_equal(got[k][loci_sl][:, nodes_sl], want[k], k)


@pytest.mark.parametrize('tag', ['sparse', 'homog', 'free'])
def test_device_trace_and_chains_equal_host_walk(tag):
    from test_lineage_host import make_pedigree
    dev, L, bp_off, bp_loci = _device_for(tag)
    tt, t_curr, last = make_pedigree(bp_off, bp_loci, L, n_founders=10, n_gen=36, per_gen=8,
                                     seed=3)
    tab, bt = tt.node_table()
    rng = np.random.RandomState(7)
    rows = np.searchsorted(tt.ids, np.concatenate([last, tt.ids[40:45]]))
    nodes = rng.permutation(np.stack([2 * rows, 2 * rows + 1], 1).ravel())
    for loci in (rng.permutation(L)[:37],                    # not contiguous, not sorted
                 np.array([L - 1, 0, 5, 5, 3]),              # a short list with a repeat
                 np.arange(L)[:130]):
        for kw in (dict(), dict(drop_before_sim=False), dict(min_time_ago=3, max_time_ago=20.5),
                   dict(drop_before_sim=False, min_time_ago=30)):
            want = tt.trace(nodes, loci, t_curr, **kw)
            got = dev.lineage_trace(tab, bt, nodes, loci, t_curr, **kw)
            _assert_trace_equal(got, want)
            np.testing.assert_array_equal(got['locus_lo'], want['last'].min(axis=1))
            np.testing.assert_array_equal(got['locus_hi'], want['last'].max(axis=1))
            off_w, chain_w = tt.lineages(nodes, loci, t_curr, **kw)
            off, chain = dev.lineage_chains(tab, bt, nodes, loci, t_curr, n_kept=got['n_kept'],
                                            **kw)
            np.testing.assert_array_equal(off, off_w)
            np.testing.assert_array_equal(chain, chain_w)
            assert chain.dtype == np.int32 and off.dtype == np.int64
    # the test means something: most lineages are at least two nodes long
    assert (tt.trace(nodes, np.arange(L)[:130], t_curr)['n_kept'] >= 2).mean() >= 0.5
    # only some outputs, or only the per-locus range: the others are not computed
    loci = np.arange(0, L, 7)
    want = tt.trace(nodes, loci, t_curr)
    got = dev.lineage_trace(tab, bt, nodes, loci, t_curr, want=('last',), locus_range=False)
    assert sorted(got) == ['last']
    np.testing.assert_array_equal(got['last'], want['last'])
    got = dev.lineage_trace(tab, bt, nodes, loci, t_curr, want=())
    assert sorted(got) == ['locus_hi', 'locus_lo']
    np.testing.assert_array_equal(got['locus_lo'], want['last'].min(axis=1))
    np.testing.assert_array_equal(got['locus_hi'], want['last'].max(axis=1))
    # the table is uploaded once and found again while nothing is appended to it
    assert dev.lineage_info()['uploaded'] is False and dev.lineage_info()['launches'] == 1
    tt.add_births(t_curr + 1, [int(tt.ids[-1]) + 1], [[int(last[0]), int(last[1])]], [[0, 1]],
                  [[1, 0]], [[1.0, 2.0]])
    tab2, bt2 = tt.node_table()
    n2 = [2 * tt.ids.size - 2, 2 * tt.ids.size - 1]
    got = dev.lineage_trace(tab2, bt2, n2, loci, t_curr + 1)
    assert dev.lineage_info()['uploaded'] is True
    _assert_trace_equal(got, tt.trace(n2, loci, t_curr + 1))
    dev.close()


def test_small_pedigree_by_hand_on_the_device():
    """the dozen individuals of tests/test_lineage_host.py, whose lineages are written out by
    hand there"""
    import gnx_oracle as O
    from test_gpu_parity import make_dev
    from test_lineage_host import SMALL_LINEAGES, small_pedigree
    tt = small_pedigree()
    paths = np.zeros((3, 8), np.uint8)
    paths[1, 4] = 1
    paths[2, [2, 6]] = 1
    dev = make_dev(16, 16, L=8, cap=1024, seed=1)
    dev.set_recomb_paths(O.pack_bits(O.recomb_paths(paths)))
    dev.init_population(50)
    dev.assign_genomes(O.starting_mutation_counts(dev.N, np.full(8, 0.5)))
    tab, bt = tt.node_table()
    for (node, locus), full in SMALL_LINEAGES.items():
        off, chain = dev.lineage_chains(tab, bt, [node], [locus], 3, drop_before_sim=False)
        assert chain.tolist() == full and off.tolist() == [0, 5]
        off, chain = dev.lineage_chains(tab, bt, [node], [locus], 3)
        assert chain.tolist() == full[:3]                  # born in steps 3, 2, 1: time < 0
    tr = dev.lineage_trace(tab, bt, [20, 21, 22, 23], [0], 3)
    assert tr['last'][0].tolist() == [12, 12, 12, 14]
    assert (tr['locus_lo'][0], tr['locus_hi'][0]) == (12, 14)
    tr = dev.lineage_trace(tab, bt, [20, 21, 22], [0], 3)
    assert (tr['locus_lo'][0], tr['locus_hi'][0]) == (12, 12)
    dev.close()


def _lineage_model(T):
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    p = small_params(seed=8, traits=True, L=56, T=T)
    ga = p['comm']['species']['spp_0']['gen_arch']
    ga['use_tskit'] = True
    ga['mu_neut'] = 1e-4          # (the expected mutations of T steps must fit the neutral loci)
    mod = gnx.make_model(p)
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(T, 'main', verbose=False)
    return mod, mod.comm[0]


def test_model_lineage_stats_coalescence_and_dicts():
    from geonomics_amd.structs import pedigree as P
    T = 40
    mod, spp = _lineage_model(T)
    tt = spp._tt
    assert tt is not None and spp.t == T - 1 and len(tt._new_muts) > 0
    ids = np.array([*spp])
    rows = np.searchsorted(tt.ids, ids)
    nodes = np.stack([2 * rows, 2 * rows + 1], 1).ravel()
    L = spp.gen_arch.L
    loci = np.arange(L)
    host = tt.trace(nodes, loci, spp.t)
    print('model: %d living, %d rows, n_kept >= 2 in %.2f of the queries'
          % (ids.size, tt.ids.size, (host['n_kept'] >= 2).mean()))
    assert (host['n_kept'] >= 2).mean() >= 0.5
    curr = np.repeat(spp._get_coords(), 2, axis=0)
    # -- the statistics, both shapes, both settings of use_individs_curr_pos
    for use_curr in (True, False):
        want = P.lineage_stats(tt, nodes, host['first'], host['last'], host['n_kept'], spp.t,
                               curr_xy=curr if use_curr else None)
        arr = spp._calc_lineage_stats(use_individs_curr_pos=use_curr, as_arrays=True)
        np.testing.assert_array_equal(arr['nodes'], nodes)
        np.testing.assert_array_equal(arr['loci'], loci)
        for st in P.LINEAGE_STATS:
            assert arr[st].dtype == np.float64 and arr[st].shape == (L, nodes.size)
            np.testing.assert_array_equal(arr[st], want[st])        # NaN == NaN here
        dct = spp._calc_lineage_stats(use_individs_curr_pos=use_curr)
        assert [*dct] == ['dir', 'dist', 'time', 'speed'] and [*dct['dir']] == loci.tolist()
        for st in P.LINEAGE_STATS:
            for i in (0, 17, L - 1):
                got = dct[st][i]
                assert len(got) == nodes.size
                assert [v is None for v in got] == np.isnan(want[st][i]).tolist()
                assert [v for v in got if v is not None] == \
                    want[st][i][~np.isnan(want[st][i])].tolist()
    a = spp._calc_lineage_stats(as_arrays=True)
    b = spp._calc_lineage_stats(use_individs_curr_pos=False, as_arrays=True)
    own = host['first'] == nodes[None, :]
    moved = own & (host['n_kept'] >= 2)
    assert moved.any() and (a['dist'][moved] != b['dist'][moved]).any()   # they did move
    np.testing.assert_array_equal(a['time'], b['time'])
    # a subset by individuals, a window, a subset of the statistics
    some = ids[::7]
    sub = spp._calc_lineage_stats(individs=some, loci=[5, 3], stats=['time'], min_time_ago=2,
                                  max_time_ago=12, as_arrays=True)
    sn = np.stack([2 * rows[::7], 2 * rows[::7] + 1], 1).ravel()
    hw = tt.trace(sn, [5, 3], spp.t, min_time_ago=2, max_time_ago=12)
    want = P.lineage_stats(tt, sn, hw['first'], hw['last'], hw['n_kept'], spp.t, ['time'],
                           curr_xy=np.repeat(spp._get_coords(individs=some), 2, axis=0))
    assert sorted(sub) == ['loci', 'nodes', 'time']
    np.testing.assert_array_equal(sub['time'], want['time'])
    assert np.nanmax(sub['time']) <= 10
    # -- coalescence: from chains walked on the host
    off, chain = tt.lineages(nodes, loci, spp.t)
    oldest = np.where(host['n_kept'] > 0, chain[np.maximum(off[1:] - 1, 0)].reshape(L, -1), -1)
    want_co = {l: bool((oldest[l] >= 0).all() and np.unique(oldest[l]).size == 1)
               for l in range(L)}
    assert spp._check_coalescence() == want_co
    assert spp._check_coalescence(all_loci=True) == all(want_co.values())
    # a pair of siblings' shared parent chromosome would coalesce; search a few small samples
    # so that both answers occur
    seen = set()
    for k in range(0, ids.size - 1, 3):
        pair = ids[k:k + 2]
        r = rows[k:k + 2]
        pn = np.stack([2 * r, 2 * r + 1], 1).ravel()
        ho = tt.trace(pn, [0, L // 2], spp.t)
        w = {l: bool((ho['last'][i] >= 0).all() and np.unique(ho['last'][i]).size == 1)
             for i, l in enumerate([0, L // 2])}
        assert spp._check_coalescence(individs=pair, loci=[0, L // 2]) == w
        seen |= set(w.values())
    one = spp._check_coalescence(individs=ids[-1:], loci=[0])
    ho = tt.trace(2 * rows[-1:] + np.arange(2), [0], spp.t)
    assert one == {0: bool(ho['last'][0, 0] == ho['last'][0, 1] >= 0)}
    print('pairs: coalescence answers seen', seen)
    # -- the nested dicts: the reference's nesting and order, youngest first
    dl = [L - 1, 2]
    good = np.nonzero((host['n_kept'][dl] >= 2).all(axis=0))[0]     # lineages worth showing
    dn = nodes[good[[5, 4, 50]]]
    for kw in (dict(), dict(use_individs_curr_pos=False, time_before_present=False),
               dict(drop_before_sim=False, max_time_ago=6)):
        d = spp._get_lineage_dicts(dl, nodes=dn, **kw)
        tkw = {k: v for k, v in kw.items() if k in ('drop_before_sim', 'max_time_ago')}
        off, chain = tt.lineages(dn, dl, spp.t, **tkw)
        assert [*d] == dl
        tbp = kw.get('time_before_present', True)
        for i, l in enumerate(dl):
            assert [*d[l]] == dn.tolist()
            for j, n in enumerate(dn.tolist()):
                q = i * len(dn) + j
                ch = chain[off[q]:off[q + 1]].tolist()
                assert [*d[l][n]] == ch
                for c in ch:
                    t, loc = d[l][n][c]
                    assert isinstance(t, float) and loc.shape == (2,)
                    assert t == float(tt._bt[0][c >> 1]) + (spp.t if tbp else 0)
                    if c == n and kw.get('use_individs_curr_pos', True):
                        np.testing.assert_array_equal(loc, curr[np.nonzero(nodes == n)[0][0]])
                    else:
                        np.testing.assert_array_equal(loc, tt._ind_xy[0][c >> 1])
    with pytest.raises(ValueError, match='as_arrays'):
        old = type(spp)._LINEAGE_DICT_MAX
        type(spp)._LINEAGE_DICT_MAX = 10                   # (at least 12 entries here)
        try:
            spp._get_lineage_dicts(dl, nodes=dn)
        finally:
            type(spp)._LINEAGE_DICT_MAX = old


@pytest.mark.timeout(600)
def test_larger_pedigree_in_chunks_equals_host_on_a_sample():
    """6000 sample chromosomes, 120 steps deep, all loci; the byte budget forces many launches"""
    from test_lineage_host import make_pedigree
    dev, L, bp_off, bp_loci = _device_for('sparse', cap=4096)
    tt, t_curr, last = make_pedigree(bp_off, bp_loci, L, n_founders=3000, n_gen=120,
                                     per_gen=3000, seed=11)
    tab, bt = tt.node_table()
    rows = np.searchsorted(tt.ids, last)
    nodes = np.stack([2 * rows, 2 * rows + 1], 1).ravel()
    loci = np.random.RandomState(1).permutation(L)
    dev.lineage_budget(1 << 20)
    got = dev.lineage_trace(tab, bt, nodes, loci, t_curr)
    info = dev.lineage_info()
    print('larger case: %d rows, %d nodes x %d loci, %d launches, %.2f ms in the kernels'
          % (bt.size, nodes.size, loci.size, info['launches'], info['kernel_ms']))
    assert info['launches'] >= 8
    rng = np.random.RandomState(2)
    ns = np.sort(rng.choice(nodes.size, 150, replace=False))
    ls = np.sort(rng.choice(loci.size, 40, replace=False))
    want = tt.trace(nodes[ns], loci[ls], t_curr)
    assert (want['n_kept'] >= 2).mean() >= 0.5
    for k in ('root', 'first', 'last', 'n_kept'):
        np.testing.assert_array_equal(got[k][np.ix_(ls, ns)], want[k], k)
    # the per-locus range of the whole sample, without anything n_loci x n_nodes
    rng_only = dev.lineage_trace(tab, bt, nodes, loci, t_curr, want=())
    np.testing.assert_array_equal(rng_only['locus_lo'], got['last'].min(axis=1))
    np.testing.assert_array_equal(rng_only['locus_hi'], got['last'].max(axis=1))
    np.testing.assert_array_equal(got['locus_lo'], rng_only['locus_lo'])
    assert dev.lineage_info()['launches'] == 1
    # chains of the sampled queries, in chunks as well
    dev.lineage_budget(64 << 10)
    off, chain = dev.lineage_chains(tab, bt, nodes[ns], loci[ls], t_curr)
    assert dev.lineage_info()['launches'] >= 4
    off_w, chain_w = tt.lineages(nodes[ns], loci[ls], t_curr)
    np.testing.assert_array_equal(off, off_w)
    np.testing.assert_array_equal(chain, chain_w)
    dev.close()


def test_refusals_launch_nothing():
    import geonomics_amd as gnx
    from geonomics_amd.structs.tiled import TiledSpecies
    from test_gpu_model_api import small_params
    from test_gpu_parity import make_dev, native
    from test_lineage_host import small_pedigree
    nat = native()
    tt = small_pedigree()
    tab, bt = tt.node_table()
    # a handle without genomes, and one without paths
    dev = make_dev(16, 16, L=0, cap=1024)
    with pytest.raises(nat.GnxError, match='genomes not assigned'):
        dev.lineage_trace(tab, bt, [20], [0], 3)
    dev.close()
    dev, L, _, _ = _device_for('sparse')
    ok = dev.lineage_trace(tab, bt, [20], [0], 3)            # (keys 0..2 exist in this path set)
    assert ok['root'][0, 0] >= 0 and dev.lineage_info()['launches'] == 1
    for bad_nodes, bad_loci, msg in (([24], [0], 'sample node'), ([-1], [0], 'sample node'),
                                     ([20], [L], 'locus'), ([20], [-1], 'locus'),
                                     ([], [0], 'at least one')):
        with pytest.raises(nat.GnxError, match=msg):
            dev.lineage_trace(tab, bt, bad_nodes, bad_loci, 3)
        with pytest.raises(nat.GnxError, match=msg):
            dev.lineage_chains(tab, bt, bad_nodes, bad_loci, 3, n_kept=np.zeros((1, 1), np.int32)
                               if len(bad_nodes) else np.zeros((1, 0), np.int32))
    n_paths = load_golden('g17_pedigree_segments')['sparse_bp_off'].size - 1
    for r, c, v, msg in ((10, 1, 2 * n_paths, 'path key'), (10, 1, -2, 'path key'),
                         (10, 0, 10, 'parent row'), (10, 0, 12, 'parent row'),
                         (11, 2, -5, 'parent row')):
        t2 = tab.reshape(-1, 4).copy()
        t2[r, c] = v
        with pytest.raises(nat.GnxError, match=msg):
            dev.lineage_trace(t2.reshape(-1, 2), bt, [20], [0], 3)
    with pytest.raises(nat.GnxError, match='offsets'):
        dev.lineage_chains(tab, bt, [20], [0], 3, n_kept=np.array([[2]], np.int32))
    with pytest.raises(ValueError):
        dev.lineage_trace(tab, bt[:-1], [20], [0], 3)
    # after all these the good request still gives the good answer
    np.testing.assert_array_equal(dev.lineage_trace(tab, bt, [20], [0], 3)['last'], ok['last'])
    dev.close()
    # no pedigree
    mod = gnx.make_model(small_params(T=3, L=16))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(3, 'main', verbose=False)
    spp = mod.comm[0]
    for call in (lambda: spp._calc_lineage_stats(), lambda: spp._check_coalescence(),
                 lambda: spp._get_lineage_dicts([0])):
        with pytest.raises(ValueError, match='no pedigree was recorded'):
            call()
    # a tiled species refuses before it looks at anything
    for name in ('_calc_lineage_stats', '_check_coalescence', '_get_lineage_dicts'):
        with pytest.raises(NotImplementedError, match='tiled over several GPUs'):
            getattr(TiledSpecies, name)(object())


def test_tiled_handle_is_refused():
    """a handle that holds ghost records (a tile's halo) refuses lineage requests"""
    from test_gpu_parity import native
    from test_lineage_host import small_pedigree
    nat = native()
    dev, L, _, _ = _device_for('sparse')
    tab, bt = small_pedigree().node_table()
    rec = np.zeros(1, nat.IND_REC)
    rec['x'], rec['y'], rec['id'] = 1.0, 1.0, 10 ** 6
    dev.tile_import_ghosts(rec)
    with pytest.raises(nat.GnxError, match='ghost records'):
        dev.lineage_trace(tab, bt, [20], [0], 3)
    dev.close()
