"""Pairwise coalescence through the recorded pedigree, host side (geonomics_amd/sim/coal.py): the
numpy restatement of gnx_coal_times / gnx_coal_segments (include/gnx_hip.h) and the statistics
computed from the device's integers.

 - coal_mrca_np against a brute-force set intersection of the chains followed over the EDGE rows
   (tests/test_lineage_host.brute_lineage: nothing of the node table), on fixture G17's three path
   sets, and against the hand-followed dozen of tests/test_lineage_host.py
 - the segment restatement on an MRCA row made by hand
 - the inverse coalescence rate on a histogram computed by hand, the fold from nodes to
   individuals, the means
"""
import numpy as np
import pytest

from conftest import load_golden
from geonomics_amd.sim import coal as CO
from test_lineage_host import (SMALL_LINEAGES, brute_lineage, edges_by_child, make_pedigree,
                               small_pedigree)


def brute_mrca(tt, nodes, loci):
    """int [n_loci][n_pairs]: max of the intersection of the two chains, from the edge rows"""
    tabs = tt.tables()
    by_child = edges_by_child(tabs)
    i, j = np.triu_indices(len(nodes), 1)
    out = np.full((len(loci), i.size), -1, np.int64)
    for q, locus in enumerate(loci):
        chains = [set(brute_lineage(tabs, by_child, int(v), int(locus))) for v in nodes]
        for p, (a, b) in enumerate(zip(i, j)):
            both = chains[a] & chains[b]
            out[q, p] = max(both) if both else -1
    return out


def path_bits(bp_off, bp_loci, L):
    """bool [n_paths][L]: the parity of a path's switch points <= l"""
    bits = np.zeros((len(bp_off) - 1, L), bool)
    for k in range(len(bp_off) - 1):
        flips = np.zeros(L, np.int64)
        np.add.at(flips, np.asarray(bp_loci[bp_off[k]:bp_off[k + 1]], dtype=np.int64), 1)
        bits[k] = np.cumsum(flips) & 1
    return bits


# ---------------------------------------------------------------- the MRCA
@pytest.mark.parametrize('tag', ['sparse', 'homog', 'free'])
def test_mrca_equals_set_intersection_over_the_edge_rows(tag):
    g = load_golden('g17_pedigree_segments')
    L = int(g[tag + '_L'][0])
    tt, t_curr, last = make_pedigree(g[tag + '_bp_off'], g[tag + '_bp_loci'], L, n_founders=10,
                                     n_gen=36, per_gen=8, seed=3)
    tab, bt = tt.node_table()
    # three of the youngest and the parents of the first of them: a parent's node lies on its
    # child's chain, so an MRCA is a sample node
    rows = np.searchsorted(tt.ids, np.unique(np.concatenate([last[:3],
                                                             tt.parents_of(last[:1])[0]])))
    nodes = np.stack([2 * rows, 2 * rows + 1], 1).ravel()[::-1].copy()      # not sorted
    loci = np.random.RandomState(5).permutation(L)[:24]
    loci[:2] = [0, L - 1]
    want = brute_mrca(tt, nodes, loci)
    got = CO.coal_mrca_np(tab, bt, tt, nodes, loci)
    assert got.dtype == np.int32 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    # the same from the path bits instead of the tables' own walk
    bits = path_bits(g[tag + '_bp_off'], g[tag + '_bp_loci'], L)
    np.testing.assert_array_equal(CO.coal_mrca_np(tab, bt, bits, nodes, loci), want)
    # both outcomes occur, and an ancestor of the sample is the MRCA of some pair
    print('%s: %.2f of the cells have an MRCA' % (tag, (want >= 0).mean()))
    assert (want >= 0).any() and (want < 0).any()
    assert np.isin(want, nodes).any()
    # the restated entry point: sums, counts, histogram from those MRCAs
    for max_ago in (-1, 20):
        r = CO.coal_times_np(tab, bt, tt, nodes, loci, t_curr, max_ago, [2, 5, 10, 36])
        ago = np.where(want >= 0, bt[np.maximum(want, 0) >> 1].astype(np.int64) + t_curr, -1)
        hit = (want >= 0) & ((ago <= max_ago) | (max_ago < 0))
        np.testing.assert_array_equal(r['mrca'], np.where(hit, want, -1))
        i, j = np.triu_indices(nodes.size, 1)
        np.testing.assert_array_equal(r['pair_cnt'][i, j], hit.sum(axis=0))
        np.testing.assert_array_equal(r['pair_sum'][j, i], (ago * hit).sum(axis=0))
        assert (np.diagonal(r['pair_cnt']) == 0).all() and (np.diagonal(r['pair_sum']) == 0).all()
        np.testing.assert_array_equal(r['locus_cnt'], hit.sum(axis=1))
        np.testing.assert_array_equal(r['locus_sum'], (ago * hit).sum(axis=1))
        for q in range(loci.size):
            assert r['locus_max'][q] == (ago[q][hit[q]].max() if hit[q].any() else -1)
        t = ago[hit]
        assert r['thist'].tolist() == [int(((t >= a) & (t < b)).sum())
                                       for a, b in ((2, 5), (5, 10), (10, 36))]
        assert r['work'] == i.size * loci.size


def test_small_pedigree_mrca_by_hand():
    """the lineages written out in tests/test_lineage_host.py (SMALL_LINEAGES), and the MRCA of
    three pairs read off them by hand:
      locus 0: 20 -> 16 -> 12 -> 8 -> 0, 21 -> 19 -> 12 -> 8 -> 0, 22 -> 19 -> 12 -> 8 -> 0
      mrca(20, 21) = 12 (their first common node), mrca(21, 22) = 19, mrca(20, 22) = 12"""
    tt = small_pedigree()
    tab, bt = tt.node_table()
    assert SMALL_LINEAGES[(20, 0)][2] == SMALL_LINEAGES[(21, 0)][2] == 12
    got = CO.coal_mrca_np(tab, bt, tt, [20, 21, 22], [0])
    assert got.tolist() == [[12, 12, 19]]                   # pairs (20,21), (20,22), (21,22)
    # every pair of the hand-followed lineages that share a locus
    for (a, la), ca in SMALL_LINEAGES.items():
        for (b, lb), cb in SMALL_LINEAGES.items():
            if la == lb and a < b:
                both = set(ca) & set(cb)
                assert CO.coal_mrca_np(tab, bt, tt, [a, b], [la])[0, 0] == \
                    (max(both) if both else -1)
    # one node on the other's chain: 16 is the parent node of 20 at locus 0, so it is the MRCA
    assert CO.coal_mrca_np(tab, bt, tt, [20, 16], [0, 3, 7]).tolist() == [[16], [16], [16]]
    assert CO.coal_mrca_np(tab, bt, tt, [12, 20], [0, 3]).tolist() == [[12], [-1]]
    # different founders: 23 -> 17 -> 14 -> 9 -> 3 at locus 0 (followed by hand: node 23 is the
    # gamete of individual 8 with path 0 from homologue 1, node 17 that of individual 7 with
    # path 1 from homologue 0, node 14 that of individual 4 from homologue 1, node 9 that of
    # founder 1 from homologue 1), and 20's chain ends in founder node 0
    assert CO.coal_mrca_np(tab, bt, tt, [20, 23], [0]).tolist() == [[-1]]
    assert CO.coal_mrca_np(tab, bt, tt, [23, 21], [1, 5]).tolist() == [[-1], [-1]]
    # ages: t_curr = 3, node 12 was born in step 1 -> 2 steps ago, node 19 in step 2 -> 1
    r = CO.coal_times_np(tab, bt, tt, [20, 21, 22], [0], 3)
    assert r['pair_sum'].tolist() == [[0, 2, 2], [2, 0, 1], [2, 1, 0]]
    assert r['locus_sum'].tolist() == [5] and r['locus_max'].tolist() == [2]
    r = CO.coal_times_np(tab, bt, tt, [20, 21, 22], [0], 3, max_ago=1)
    assert r['mrca'].tolist() == [[-1, -1, 19]] and r['pair_cnt'].sum() == 2
    r = CO.coal_times_np(tab, bt, tt, [20, 23], [0], 3)
    assert r['locus_max'].tolist() == [-1] and r['locus_cnt'].tolist() == [0]


# ---------------------------------------------------------------- segments
def loop_segments(m, pos, brk, min_loci, min_len):
    """the definition of include/gnx_hip.h followed position by position"""
    out, s = [], None
    for q in range(len(m) + 1):
        goes_on = s is not None and q < len(m) and m[q] == m[s] and not (brk is not None
                                                                          and brk[q])
        if s is not None and not goes_on:
            if q - s >= max(1, min_loci) and pos[q - 1] - pos[s] >= min_len:
                out.append((s, q - 1, int(pos[q - 1] - pos[s])))
            s = None
        if s is None and q < len(m) and m[q] >= 0:
            s = q
    return out


def test_segments_of_a_hand_made_row():
    # rows 0..4 were born at table times 1, 0, -2, -5, -8; t_curr = 10: 11, 10, 8, 5, 2 steps ago
    bt = np.array([1, 0, -2, -5, -8], np.int32)
    #        q:  0  1  2  3   4  5  6  7   8   9  10  11  12  13
    raw = [8, 8, 8, 8, -1, 6, 4, 4, 8, 8, 2, 8, 8, 8]
    pos = [0, 1, 2, 3, 5, 6, 10, 11, 20, 30, 31, 32, 33, 40]
    brk = np.zeros(14, np.uint8)
    brk[2] = 1                                              # inside the first run
    brk[4] = 1                                              # where nothing coalesces: no effect

    def segs(max_ago=-1, min_loci=1, min_len=0, b=brk):
        m, _ = CO.coal_mask(raw, bt, 10, max_ago)
        row, s, e, count, length = CO.segments_of(m, pos, b, min_loci, min_len)
        assert (row == 0).all() and (count == e - s + 1).all()
        got = [*zip(s.tolist(), e.tolist(), length.tolist())]
        assert got == loop_segments(m, pos, b, min_loci, min_len)
        return got

    # the break splits 0..3; position 5 is a run of 1; 8..9 | 10 | 11..13 are three runs (three
    # stretches of one MRCA each), and the last run ends at the list's last locus
    assert segs() == [(0, 1, 1), (2, 3, 1), (5, 5, 0), (6, 7, 1), (8, 9, 10), (10, 10, 0),
                      (11, 13, 8)]
    assert segs(b=None)[0] == (0, 3, 3) and len(segs(b=None)) == 6
    # min_loci = 3 leaves out all but the last; min_len = 9 all but 8..9 (length 10)
    assert segs(min_loci=2) == [(0, 1, 1), (2, 3, 1), (6, 7, 1), (8, 9, 10), (11, 13, 8)]
    assert segs(min_loci=3) == [(11, 13, 8)]
    assert segs(min_len=9) == [(8, 9, 10)]
    assert segs(min_loci=3, min_len=9) == []
    # max_ago = 9: node 2 (10 steps ago) is too old; what it separated stays two segments
    assert segs(max_ago=9) == [(0, 1, 1), (2, 3, 1), (5, 5, 0), (6, 7, 1), (8, 9, 10),
                               (11, 13, 8)]
    # max_ago = 5 also takes node 4 (8 steps ago), max_ago = 1 everything
    assert segs(max_ago=5) == [(0, 1, 1), (2, 3, 1), (5, 5, 0), (8, 9, 10), (11, 13, 8)]
    assert segs(max_ago=1) == []
    # a limit that takes the middle of a stretch with ONE ancestor cannot occur (one node, one
    # age); a limit in the middle of a stretch that coalesces throughout splits it
    m, _ = CO.coal_mask([6, 6, 2, 2, 6, 6], bt, 10, 9)
    assert m.tolist() == [6, 6, -1, -1, 6, 6]
    assert [*zip(*[a.tolist() for a in CO.segments_of(m, np.arange(6))[1:3]])] == [(0, 1), (4, 5)]


def test_segments_restated_on_the_small_pedigree():
    tt = small_pedigree()
    tab, bt = tt.node_table()
    nodes, loci = [20, 21, 22, 23], np.arange(8)
    pos = np.array([0, 2, 3, 7, 8, 10, 15, 16])
    brk = np.array([0, 0, 0, 0, 0, 1, 0, 0], np.uint8)
    M = brute_mrca(tt, nodes, loci).T                                # [n_pairs][n_loci]
    assert (M >= 0).any() and (M < 0).any()
    i, j = np.triu_indices(4, 1)
    for max_ago, min_loci, min_len, b in ((-1, 1, 0, None), (-1, 2, 0, brk), (2, 1, 0, brk),
                                          (-1, 1, 3, brk), (3, 2, 2, None)):
        edges = [0, 2, 5, 100]
        r = CO.coal_segments_np(tab, bt, tt, nodes, loci, pos, b, 3, max_ago, min_loci, min_len,
                                edges, True)
        cnt = np.zeros((4, 4), np.int64)
        tot = np.zeros((4, 4), np.int64)
        longest = np.zeros((4, 4), np.int64)
        hist = np.zeros((3, 2), np.int64)
        cover = np.zeros(8, np.int64)
        for p in range(6):
            m, _ = CO.coal_mask(M[p], bt, 3, max_ago)
            for s, e, ln in loop_segments(m, pos, b, min_loci, min_len):
                for a, c in ((i[p], j[p]), (j[p], i[p])):
                    cnt[a, c] += 1
                    tot[a, c] += ln
                    longest[a, c] = max(longest[a, c], ln)
                k = np.searchsorted(edges, ln, side='right') - 1
                hist[k] += (1, ln)
                cover[s:e + 1] += 1
        np.testing.assert_array_equal(r['cnt'], cnt)
        np.testing.assert_array_equal(r['len'], tot)
        np.testing.assert_array_equal(r['longest'], longest)
        np.testing.assert_array_equal(r['hist'], hist)
        np.testing.assert_array_equal(r['cover'], cover)
        assert r['cnt'].dtype == np.int32 and r['work'] == 48
    assert cnt.sum() > 0
    with pytest.raises(ValueError, match='ascending'):
        CO.coal_segments_np(tab, bt, tt, nodes, [3, 3, 4], [0, 1, 2])


# ---------------------------------------------------------------- the statistics
def test_coal_rate_by_hand():
    """100 cells.  Bin [0, 2): 19 of 100 coalesce, 1 - 0.81^(1/2) = 0.1 per step, Ne = 5.
    Bin [2, 4): none of 81: inf.  Bin [4, 8): 65 of 81, 1 - (16/81)^(1/4) = 1/3, Ne = 1.5.
    Bin [8, 9): all 16 left: p = 1, Ne = 0.5.  Bin [9, 12): nothing left at risk: NaN"""
    r = CO.coal_rate([19, 0, 65, 16, 0], [0, 2, 4, 8, 9, 12], 100)
    assert r['at_risk'].tolist() == [100, 81, 81, 16, 0]
    assert r['counts'].tolist() == [19, 0, 65, 16, 0]
    np.testing.assert_allclose(r['ne'][[0, 2, 3]], [5.0, 1.5, 0.5], rtol=1e-12)
    assert r['ne'][1] == np.inf and np.isnan(r['ne'][4])
    # 10 more cells coalesce before the first edge: they leave R before bin 0
    r2 = CO.coal_rate([19, 0, 65, 16, 0], [3, 5, 7, 11, 12, 15], 110, n_before=10)
    assert r2['at_risk'].tolist() == [100, 81, 81, 16, 0]
    np.testing.assert_array_equal(r2['ne'], r['ne'])
    # cells that never coalesce stay at risk
    r3 = CO.coal_rate([50], [0, 1], 200)
    assert r3['ne'].tolist() == [2.0] and r3['at_risk'].tolist() == [200]


def test_fold_from_nodes_to_individuals():
    rng = np.random.RandomState(3)
    m = 3
    U = np.triu(rng.randint(0, 9, (2 * m, 2 * m)), 1)
    cnt, tot, longest = (U + U.T).astype(np.int32), (7 * (U + U.T)).astype(np.int64), \
        (U + U.T).astype(np.int64)
    c, t, g = CO.fold_to_individuals(cnt, tot, longest)
    for a in range(m):
        for b in range(m):
            if a == b:
                assert c[a, a] == cnt[2 * a, 2 * a + 1] and t[a, a] == tot[2 * a, 2 * a + 1]
                assert g[a, a] == longest[2 * a, 2 * a + 1]
            else:
                four = [(2 * a + h, 2 * b + k) for h in (0, 1) for k in (0, 1)]
                assert c[a, b] == sum(cnt[x] for x in four)
                assert t[a, b] == sum(tot[x] for x in four)
                assert g[a, b] == max(longest[x] for x in four)
    assert c.dtype == np.int32 and t.dtype == np.int64 and (c == c.T).all()


def test_means_and_branch_diversity_by_hand():
    # three nodes, two loci: pairs (0,1): T = 2, 4; (0,2): T = 6 at one locus; (1,2): never
    ps = np.array([[0, 6, 6], [6, 0, 0], [6, 0, 0]], np.int64)
    pc = np.array([[0, 2, 1], [2, 0, 0], [1, 0, 0]], np.int32)
    tm, per, share = CO.tmrca_stats(ps, pc, np.array([8, 4]), np.array([2, 1]),
                                    np.array([6, 4], np.int32))
    np.testing.assert_array_equal(tm, [[np.nan, 3, 6], [3, np.nan, np.nan],
                                       [6, np.nan, np.nan]])
    assert per['mean'].tolist() == [4.0, 4.0] and per['max'].tolist() == [6.0, 4.0]
    np.testing.assert_allclose(per['share_coalesced'], [2 / 3, 1 / 3])
    assert share == 0.5
    total, by = CO.branch_diversity(ps, pc, [np.array([0, 1]), np.array([2])])
    assert total == 2 * 12 / 3 and by['within'][0] == 2 * 3.0 and np.isnan(by['within'][1])
    assert by['between'][0, 1] == by['between'][1, 0] == 2 * 6.0
    assert CO.branch_diversity(ps, pc)[1] is None
    e = CO.default_time_edges(36, 20)
    assert e[0] == 0 and e[-1] == 37 and (np.diff(e) > 0).all() and e.size <= 21
    assert CO.default_time_edges(2, 20).tolist() == [0, 1, 2, 3]


def test_library_exports_and_binding_exist():
    from geonomics_amd import _native as nat
    assert {'gnx_coal_times', 'gnx_coal_segments'} <= set(nat.EXPORTS)
    assert callable(nat.Device.coal_times) and callable(nat.Device.coal_segments)
