"""Simplification of the recorded pedigree, host side (geonomics_amd/structs/pedigree.py:
TreeTables.ancestral_masks / simplify; reference structs/species.py:1107-1142).

 - ancestral_masks (the cohort recurrence) against the marking of every node on every chain
   TreeTables.lineages returns for the sample at all loci, on the synthetic pedigrees of
   tests/test_lineage_host.py over fixture G17's three path sets
 - simplify: the sample's chains and genotypes are what they were, the brute-force walk over
   the edge rows still agrees, a second pass drops nothing, births can be added afterwards
 - the dozen individuals of small_pedigree(), followed by hand below
 - edge cases: everybody sampled, one founder sampled, founders only, a step without births,
   mutations of dropped and of kept individuals
Everything compared is integers or bits: equality is exact."""
import numpy as np
import pytest

from conftest import load_golden
from geonomics_amd.structs.pedigree import TreeTables
from test_lineage_host import check_against_brute, make_pedigree, small_pedigree

TAGS = ['sparse', 'homog', 'free']


def g17_pedigree(tag, genotypes=False):
    g = load_golden('g17_pedigree_segments')
    L = int(g[tag + '_L'][0])
    tt, t_curr, last = make_pedigree(g[tag + '_bp_off'], g[tag + '_bp_loci'], L, n_founders=10,
                                     n_gen=36, per_gen=8, seed=3, genotypes=genotypes)
    return tt, t_curr, last, L


def sample_nodes(rows):
    rows = np.asarray(rows, dtype=np.int64)
    return np.stack([2 * rows, 2 * rows + 1], 1).ravel()


def brute_masks(tt, rows, t_curr):
    """bool [2 n_rows][L]: every node on every chain of the sample, marked at the chain's locus"""
    nodes = sample_nodes(rows)
    off, chain = tt.lineages(nodes, np.arange(tt.L), t_curr, drop_before_sim=False)
    locus = np.repeat(np.arange(tt.L * nodes.size) // nodes.size, np.diff(off))
    mark = np.zeros((2 * tt.ids.size, tt.L), bool)
    mark[chain, locus] = True
    return mark


def chains_by_id(tt, rows, t_curr):
    """the sample's chains at all loci as (individual id, homologue) per entry"""
    nodes = sample_nodes(rows)
    off, chain = tt.lineages(nodes, np.arange(tt.L), t_curr, drop_before_sim=False)
    return off, tt.ids[chain >> 1], chain & 1


@pytest.mark.parametrize('tag', TAGS)
def test_ancestral_masks_equal_the_marking_of_every_chain(tag):
    tt, t_curr, last, L = g17_pedigree(tag)
    rows = np.searchsorted(tt.ids, last)
    got = tt.ancestral_masks(rows)
    assert got.dtype == bool and got.shape == (2 * tt.ids.size, L)
    np.testing.assert_array_equal(got, brute_masks(tt, rows, t_curr))
    anc = got.any(axis=1)
    no_node = ~(anc[0::2] | anc[1::2])
    one_node = anc[0::2] ^ anc[1::2]
    print('%s: %.0f %% of the rows without an ancestral node, %d rows with exactly one'
          % (tag, 100 * no_node.mean(), one_node.sum()))
    assert no_node.mean() >= 0.10 and one_node.sum() >= 1
    assert got[sample_nodes(rows)].all()


@pytest.mark.parametrize('tag', TAGS)
def test_simplify_keeps_what_the_sample_descends_from(tag):
    tt, t_curr, last, L = g17_pedigree(tag, genotypes=True)
    rows = np.searchsorted(tt.ids, last)
    n_old = tt.ids.size
    old_ids = tt.ids.copy()
    anc = tt.ancestral_masks(rows).any(axis=1)
    keep = anc[0::2] | anc[1::2]
    off_b, id_b, hom_b = chains_by_id(tt, rows, t_curr)
    geno_b = tt.genotypes_of(last)
    founders_kept = int(keep[:10].sum())
    new_row = tt.simplify(rows)
    assert new_row.dtype == np.int64 and new_row.shape == (n_old,)
    np.testing.assert_array_equal(new_row >= 0, keep)
    np.testing.assert_array_equal(new_row[keep], np.arange(keep.sum()))
    np.testing.assert_array_equal(tt.ids, old_ids[keep])
    assert tt.ids.size < n_old
    rows2 = np.searchsorted(tt.ids, last)
    np.testing.assert_array_equal(rows2, new_row[rows])
    off_a, id_a, hom_a = chains_by_id(tt, rows2, t_curr)
    np.testing.assert_array_equal(off_a, off_b)
    np.testing.assert_array_equal(id_a, id_b)
    np.testing.assert_array_equal(hom_a, hom_b)
    np.testing.assert_array_equal(tt.genotypes_of(last), geno_b)
    assert tt.n_founders == founders_kept == tt._founder_g.shape[0]
    assert (tt.node_table()[1][:tt.n_founders] == 1).all()
    assert (tt.node_table()[1][tt.n_founders:] <= 0).all()
    nodes = sample_nodes(rows2[:3])[::-1].copy()
    loci = np.random.RandomState(5).permutation(L)[:24]
    loci[:2] = [0, L - 1]
    check_against_brute(tt, nodes, loci, t_curr)
    check_against_brute(tt, nodes, loci, t_curr, drop_before_sim=False)
    # the table shapes go together
    tab, bt = tt.node_table()
    n = tt.ids.size
    assert tab.shape == (2 * n, 2) and tab.dtype == np.int32 and bt.shape == (n,)
    assert tt._ind_xy[0].shape == (n, 2) and tt._ind_time[0].shape == (n,)
    e = tt.tables()['edges']
    assert e['child'].size and e['child'].max() < 2 * n and e['parent'].max() < 2 * n
    assert (e['parent'] >> 1 < e['child'] >> 1).all()
    # a second pass with the same sample drops nothing
    before = (tab.copy(), tt._edges[0].copy())
    again = tt.simplify(rows2)
    np.testing.assert_array_equal(again, np.arange(n))
    np.testing.assert_array_equal(tt.node_table()[0], before[0])
    np.testing.assert_array_equal(tt._edges[0], before[1])
    # births from the sample can be added, and their lineages hold
    rng = np.random.RandomState(9)
    n_paths = len(tt._bp_off) - 1
    child = int(tt.ids[-1]) + 1 + np.arange(5)
    tt.add_births(t_curr + 1, child, rng.choice(last, (5, 2)), rng.randint(0, n_paths, (5, 2)),
                  rng.randint(0, 2, (5, 2)), rng.uniform(0, 30, (5, 2)))
    new_nodes = sample_nodes(np.searchsorted(tt.ids, child[:2]))
    check_against_brute(tt, new_nodes, loci[:8], t_curr + 1)
    check_against_brute(tt, new_nodes, loci[:8], t_curr + 1, drop_before_sim=False)
    assert tt.genotypes_of(child).shape == (5, L, 2)


def test_tables_and_text_files_after_a_simplification(tmp_path):
    tt, t_curr, last, L = g17_pedigree('sparse', genotypes=True)
    tt.simplify(np.searchsorted(tt.ids, last))
    t = tt.tables()
    n = tt.ids.size
    assert t['nodes']['time'].size == 2 * n and t['individuals']['gnx_id'].size == n
    assert t['mutations']['node'].max() < 2 * tt.n_founders
    tt.write_text(str(tmp_path / 'simp'))
    tt.write_csv(str(tmp_path / 'simp'))
    with open(str(tmp_path / 'simp.individuals.txt')) as f:
        assert len(f.readlines()) == n + 1


# ---------------------------------------------------------------- a dozen individuals, by hand
def test_small_pedigree_by_hand():
    """small_pedigree() with individual 11 (row 11, nodes 22 and 23) as the sample; the gametes
    (test_lineage_host.small_pedigree: path 0 never switches, 1 at locus 4, 2 at loci 2 and 6):

      22 <- 19 at all loci;  19 <- 12 at all;  12 <- 8 at loci 0-3, 9 at 4-7;
      8 <- 0 at all;  9 <- 3 at loci 0-3, 2 at 4-7
      23 <- 17 at all;  17 <- 14 at 0-3, 15 at 4-7;  14 <- 9 at all;  15 <- 8 at all

    so node 9 is reached at 4-7 through 12 and at 0-3 through 14, node 8 at 0-3 through 12 and
    at 4-7 through 15, and of the founders node 0 at all loci, 3 at 0-3, 2 at 4-7.  Nodes 1,
    13, 16, 18, 20, 21 and rows 2, 3, 5 (nodes 4-7, 10, 11) carry nothing: the rows 2, 3, 5
    and 10 go; 13 loses its parent row 5 and becomes a root, 16 and 18 keep theirs."""
    tt = small_pedigree()
    want = {22: 8, 23: 8, 19: 8, 17: 8, 12: 8, 14: 4, 15: 4, 8: 8, 9: 8, 0: 8, 2: 4, 3: 4}
    m = tt.ancestral_masks([11])
    np.testing.assert_array_equal(m.sum(axis=1), [want.get(v, 0) for v in range(24)])
    assert m[14, :4].all() and m[15, 4:].all() and m[3, :4].all() and m[2, 4:].all()
    tab_old = tt.node_table()[0].copy()
    new_row = tt.simplify([11])
    assert new_row.tolist() == [0, 1, -1, -1, 2, -1, 3, 4, 5, 6, -1, 7]
    assert tt.ids.tolist() == [0, 1, 4, 6, 7, 8, 9, 11] and tt.n_founders == 2
    tab, bt = tt.node_table()
    assert bt.tolist() == [1, 1, 0, -1, -1, -2, -2, -3]
    # old node 13 = new node 7: a root now; old 12 = new 6 keeps parent row 4 -> 2 and its key
    assert tab[7].tolist() == [-1, 0] and tab[6].tolist() == [2, tab_old[12, 1]]
    # old 16, 18 (new 10, 12) are not ancestral but their parent rows 6, 7 (new 3, 4) stay
    assert tab[10].tolist() == [3, tab_old[16, 1]] and tab[12].tolist() == [4, tab_old[18, 1]]
    e = tt.tables()['edges']
    assert 7 not in e['child'].tolist()
    # the sample's lineages, renumbered: (22, 0) was [22, 19, 12, 8, 0]
    off, chain = tt.lineages([14, 15], [0, 5], 3, drop_before_sim=False)
    assert chain[off[0]:off[1]].tolist() == [14, 13, 6, 4, 0]            # 22 at locus 0
    assert chain[off[1]:off[2]].tolist() == [15, 11, 8, 5, 3]            # 23 at 0: 17 14 9 3
    assert chain[off[2]:off[3]].tolist() == [14, 13, 6, 5, 2]            # 22 at 5: 19 12 9 2
    assert chain[off[3]:off[4]].tolist() == [15, 11, 9, 4, 0]            # 23 at 5: 17 15 8 0
    check_against_brute(tt, [14, 15], np.arange(8), 3, drop_before_sim=False)


# ---------------------------------------------------------------- edge cases
def test_sample_of_every_row_drops_nothing():
    tt = small_pedigree()
    tab, e = tt.node_table()[0].copy(), tt._edges[0].copy()
    assert tt.ancestral_masks(np.arange(12)).all()
    np.testing.assert_array_equal(tt.simplify(np.arange(12)), np.arange(12))
    np.testing.assert_array_equal(tt.node_table()[0], tab)
    np.testing.assert_array_equal(tt._edges[0], e)


def test_sample_of_one_founder_keeps_that_row_only():
    tt = small_pedigree()
    m = tt.ancestral_masks([2])
    assert m[4:6].all() and m.sum() == 16
    new_row = tt.simplify([2])
    assert new_row.tolist() == [-1, -1, 0] + [-1] * 9
    assert tt.ids.tolist() == [2] and tt.n_founders == 1
    assert tt.node_table()[0].tolist() == [[-1, 0], [-1, 0]] and tt._edges[0].shape == (0, 4)
    assert tt.tables()['edges']['child'].size == 0


def test_founders_only():
    tt = TreeTables(8, [0, 0, 1, 3], [4, 2, 6])
    g = np.arange(4 * 8 * 2).reshape(4, 8, 2) % 2
    tt.add_founders(np.arange(4), np.arange(8.0).reshape(4, 2), g)
    assert tt.ancestral_masks([1, 3]).sum(axis=1).tolist() == [0, 0, 8, 8, 0, 0, 8, 8]
    assert tt.simplify([3, 1]).tolist() == [-1, 0, -1, 1]
    assert tt.ids.tolist() == [1, 3] and tt.n_founders == 2
    np.testing.assert_array_equal(tt.genotypes_of([1, 3]), g[[1, 3]])
    with pytest.raises(ValueError):
        tt.simplify([2])
    with pytest.raises(ValueError):
        tt.simplify([])


def test_a_step_without_births():
    """births in steps 0 and 2, none in step 1: the cohorts' birth times have a gap"""
    tt = TreeTables(8, [0, 0, 1, 3], [4, 2, 6])
    tt.add_founders(np.arange(3), np.zeros((3, 2)))
    tt.add_births(0, [3, 4], [(0, 1), (1, 1)], [(1, 0), (2, 0)], [(0, 0), (1, 0)],
                  np.zeros((2, 2)))
    tt.add_births(1, [], np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2)))
    tt.add_births(2, [5], [(3, 3)], [(0, 1)], [(0, 1)], np.zeros((1, 2)))
    assert tt.node_table()[1].tolist() == [1, 1, 1, 0, 0, -2]
    m = tt.ancestral_masks([5])
    np.testing.assert_array_equal(m, brute_masks(tt, [5], 2))
    # 10 <- 6 at all loci, 11 <- 7 at 0-3 and 6 at 4-7; 6 <- 0 at 0-3, 1 at 4-7; 7 <- 2
    assert m.sum(axis=1).tolist() == [4, 4, 4, 0, 0, 0, 8, 4, 0, 0, 8, 8]
    assert tt.simplify([5]).tolist() == [0, 1, -1, 2, -1, 3]
    check_against_brute(tt, [6, 7], np.arange(8), 2, drop_before_sim=False)


def test_mutations_of_dropped_individuals_go():
    tt = small_pedigree()
    tt.add_mutations([10, 9, 5], [1, 6, 3], [0, 1, 1])     # ids 10 and 5 go, 9 stays (sample 11)
    before = tt.tables()['mutations']
    assert sorted(before['node'].tolist()) == [11, 19, 20]
    tt.simplify([11])
    assert tt._new_muts == [(6, 9, 1)]
    t = tt.tables()
    assert t['mutations']['node'].tolist() == [13] and t['sites']['position'].tolist() == [6.0]
