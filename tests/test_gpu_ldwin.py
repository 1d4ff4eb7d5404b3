"""Model.prune_ld, clump, calc_ld_scores and run_ldsc on the device (csrc/gnx_ldwin.hip,
sim/ldwin.py, Species._prune_ld / _clump / _calc_ld_scores): gnx_ld_window against the numpy
restatement geonomics_amd/sim/ldwin.brute_window (every pair brute-forced as include/gnx_ldwin.h
specifies), the greedy choices through the Species methods against greedy_independent on the
restatement's edges, and the Model methods feeding the calls that take loci= and weights=.
Needs an MI355X.

Bounds.  c1, partners, n_edges, ei, ej and work are integers: equal.  er2 comes from integers
by the same three IEEE roundings on both sides: bit-equal.  score[j] is a sum of m_j =
partners[j] such terms, all >= 0; the restatement's sum is the correctly rounded sum of its
terms (math.fsum: 1 unit of 2^-53 score), the device's sum in any order adds m_j units (the
any-order bound of _ld.sum_bounds):

    |score[j] - score_ref[j]| <= (m_j + 1) 2^-53 score_ref[j].

A call repeated is bit-equal in every output; so is a call under another byte budget.
Measured on an MI355X, worst error / bound: 0.189 (case A), 0.0998 (B), 0.117 (C, in one block
and in four or five: the same bytes), 0.0385 (D)."""
import numpy as np
import pytest

import _ld as T
import _ldwin as W
from test_gpu_parity import native
from geonomics_amd.sim import ldwin as LW

pytestmark = pytest.mark.gpu

BIG = 1 << 50
EDGES = 1 << 20
KEYS = ('c1', 'partners', 'score', 'ei', 'ej', 'er2')


def _handle(nat, gts, seed=20):
    """a population with genotypes gts [n][L][2] scattered on a 24 x 20 landscape"""
    import gnx_oracle as O
    n, L = gts.shape[:2]
    rng = np.random.RandomState(seed)
    dev = nat.Device(24, 20, 1, L=L, n_traits=0, cap_inds=n + 64, cap_rows=n + 64, seed=seed)
    dev.upload_rasters(np.ones((1, 20, 24), np.float32))
    dev.set_species_params(nat.default_species_params())
    dev.upload_population(rng.uniform(0, 24, n).astype(np.float32),
                          rng.uniform(0, 20, n).astype(np.float32), np.zeros(n), np.zeros(n),
                          np.arange(n))
    dev.upload_genomes(O.pack_genomes(np.ascontiguousarray(gts, dtype=np.uint8)))
    return dev


def _same(a, b, keys=KEYS):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in keys) \
        and a['n_edges'] == b['n_edges'] and a['work'] == b['work']


def _check(dev, gts, loci, pos, window, min_minor, r2_min, slots=None, label='', scores=True,
           max_edges=EDGES, ref=None):
    """one call against the restatement within the bounds of the module's docstring, and
    bit-equal when repeated -> (the call's dict, the restatement's, worst error / bound)"""
    if ref is None:
        bits = T.bits_of(gts if slots is None else gts[slots])[:, loci]
        ref = LW.brute_window(bits, pos, window, min_minor, r2_min)
    got = dev.ld_window(loci, pos, window, slots, min_minor, r2_min, max_edges, BIG, scores)
    info = dev.ld_window_info()
    np.testing.assert_array_equal(got['c1'], ref['c1'], err_msg=label)
    worst = 0.0
    if scores:
        np.testing.assert_array_equal(got['partners'], ref['partners'], err_msg=label)
        bound = W.score_bound(ref)
        err = np.abs(got['score'] - ref['score'])
        ok = bound > 0
        if ok.any():
            worst = float((err[ok] / bound[ok]).max())
        print('%s: worst score error / bound %.3g' % (label, worst))
        assert (err <= bound).all(), (label, err, bound)
        assert not got['score'][~ref['kept']].any() and not got['partners'][~ref['kept']].any()
    else:
        assert got['partners'] is None and got['score'] is None
    if max_edges:
        assert got['n_edges'] == ref['ei'].size, label
        np.testing.assert_array_equal(got['ei'], ref['ei'], err_msg=label)
        np.testing.assert_array_equal(got['ej'], ref['ej'], err_msg=label)
        assert got['er2'].tobytes() == ref['er2'].tobytes(), label
    else:
        assert got['n_edges'] is None and got['ei'] is None and got['er2'] is None
    n_chrom = 2 * (dev.N if slots is None else len(slots))
    nq, nt = (n_chrom + 63) // 64, (len(loci) + 63) // 64
    print('%s: %d chromosomes (%d words), %d loci (%d kept), window %g: %d in-window pairs, %d '
          'edges, work %d, %s' % (label, n_chrom, nq, len(loci), ref['kept'].sum(), window,
                                  ref['partners'].sum() // 2, ref['ei'].size, got['work'], info))
    assert got['work'] % nq == 0 and nt * nq <= got['work'] <= nt * (nt + 1) // 2 * nq, label
    only = dev.ld_window(loci, pos, window, slots, min_minor, r2_min, max_edges, 0, scores)
    assert only['work'] == got['work'] and only['c1'] is None
    assert dev.ld_window_info()['launches'] == 0
    again = dev.ld_window(loci, pos, window, slots, min_minor, r2_min, max_edges, BIG, scores)
    assert _same(again, got), label
    return got, ref, worst


@pytest.fixture(scope='module')
def case_a():
    nat = native()
    D, pos = W.case_a()
    gts = W.gts_of(D)
    dev = _handle(nat, gts)
    yield nat, dev, gts, pos
    dev.close()


def test_case_a_windows_inside_a_tile_over_its_boundary_the_ties_and_everything(case_a):
    nat, dev, gts, pos = case_a
    loci = np.arange(130)
    assert pos[39] == pos[40] == pos[41] and pos[90] - pos[89] > 39.0
    # 0.3 Morgans: a dozen loci, most windows end inside their own tile
    got, ref, _ = _check(dev, gts, loci, pos, 0.3, 2, 0.01, label='case A, 0.3 M')
    assert ref['kept'].sum() == 127 and not ref['kept'][[5, 70, 129]].any()
    assert 0 < ref['partners'].max() < 40 and got['work'] == 5 * 5      # not (0, 2): the break
    # 2 Morgans: from tile 0 far into tile 1, never over the break before locus 90
    got, ref, _ = _check(dev, gts, loci, pos, 2.0, 2, 0.01, label='case A, 2 M')
    assert ref['in_window'][:64, 64:90].any() and not ref['in_window'][:90, 90:].any()
    assert got['work'] == 5 * 5
    # 0: only the tied positions; tile 1 is not reached from tile 0
    got, ref, _ = _check(dev, gts, loci, pos, 0.0, 2, 0.0, label='case A, window 0')
    assert got['n_edges'] == 3 and got['ei'].tolist() == [39, 39, 40] and got['work'] == 3 * 5
    assert got['partners'][[39, 40, 41]].tolist() == [2, 2, 2] and got['partners'].sum() == 6
    # inf: every kept pair
    got, ref, _ = _check(dev, gts, loci, pos, np.inf, 2, 0.0, label='case A, inf')
    assert got['n_edges'] == 127 * 126 // 2 and got['work'] == 6 * 5
    assert (got['partners'][ref['kept']] == 126).all()
    assert dev.ld_window_info()['locus_blocks'] == 1
    # min_minor = 1 takes the singleton in; 0 and negative values mean 1
    one, ref1, _ = _check(dev, gts, loci, pos, 2.0, 1, 0.01, label='case A, min_minor 1')
    assert ref1['kept'].sum() == 128
    for mm in (0, -3):
        assert _same(dev.ld_window(loci, pos, 2.0, None, mm, 0.01, EDGES, BIG), one)


def test_case_b_loci_in_any_order_a_subset_of_the_individuals_and_absent_outputs(case_a):
    nat, dev, gts, pos = case_a
    rng = np.random.RandomState(3)
    # 70 loci in no order, among them both sides of a word boundary and the last valid bit
    rest = rng.permutation([l for l in range(130) if l not in (63, 64, 129)])[:67]
    loci = rng.permutation(np.r_[64, 63, 129, rest])
    assert (np.diff(loci) < 0).sum() > 20 and np.unique(loci).size == 70
    slots = rng.choice(131, 77, replace=False).astype(np.int64)
    p = np.sort(pos[rng.choice(130, 70, replace=False)])        # the request's own coordinates
    both, ref, _ = _check(dev, gts, loci, p, 1.0, 2, 0.02, slots, label='case B')
    _check(dev, gts, loci[:1], p[:1], 1.0, 1, 0.0, slots[:1], label='one locus, one individual')
    _check(dev, gts, loci[:2], p[:2], np.inf, 1, 0.0, slots[:9], label='two loci')
    # the edges alone (partners and score NULL), the scores alone (max_edges = 0)
    e, _, _ = _check(dev, gts, loci, p, 1.0, 2, 0.02, slots, label='case B, edges only',
                     scores=False, ref=ref)
    s, _, _ = _check(dev, gts, loci, p, 1.0, 2, 0.02, slots, label='case B, scores only',
                     max_edges=0, ref=ref)
    assert all(e[k].tobytes() == both[k].tobytes() for k in ('c1', 'ei', 'ej', 'er2'))
    assert all(s[k].tobytes() == both[k].tobytes() for k in ('c1', 'partners', 'score'))


def test_case_c_several_lds_stages_and_locus_blocks_with_halos():
    """1100 individuals: 2200 chromosomes = 34 words and 24 bits, two full LDS stages of 16
    words and a partial one (rows of 48 words: 24576 bytes a tile); L = 320 (five tiles).  With
    scores a tile pair adds 2048 bytes of partials"""
    nat = native()
    rng = np.random.RandomState(23)
    n, L = 1100, 320
    D = rng.binomial(2, rng.uniform(0.02, 0.98, L), size=(n, L))
    for l in range(1, L, 3):                    # neighbours in LD: most copy the locus before
        same = rng.rand(n) < 0.7
        D[same, l] = D[same, l - 1]
    from geonomics_amd.sim import ld as LD
    pos = LD.map_positions(np.r_[0.0, rng.uniform(0.0005, 0.01, L - 1)])
    gts = W.gts_of(D)
    dev = _handle(nat, gts)
    tile, part = 64 * 48 * 8, 2048
    try:
        loci = np.arange(L)
        worst = 0.0
        # (window, budget, blocks): a tile reaches the next one / the next two
        for window, budget, blocks in ((0.1, 2 * tile + 2 * part + 1000, 5),
                                       (0.5, 3 * tile + 3 * part + 1000, 4)):
            reach = 2 if window == 0.1 else 3
            assert pos[64 * reach] - pos[63] > window >= pos[64 * (reach - 1)] - pos[63]
            dev.ld_budget(0)
            whole, ref, w1 = _check(dev, gts, loci, pos, window, 40, 0.1,
                                    label='case C, window %g, one block' % window)
            assert dev.ld_window_info()['locus_blocks'] == 1 and ref['ei'].size > 50
            dev.ld_budget(budget)
            cut, _, w2 = _check(dev, gts, loci, pos, window, 40, 0.1, ref=ref,
                                label='case C, window %g, %d blocks' % (window, blocks))
            info = dev.ld_window_info()
            assert info['locus_blocks'] == blocks >= 3 and info['launches'] >= 4 * blocks
            # the integers and the edges are those of one block; so are the scores, whose order
            # does not follow the blocks
            assert _same(cut, whole)
            worst = max(worst, w1, w2)
            # below one tile with its halo and their partials: refused with the bytes
            need = reach * (tile + part)
            dev.ld_budget(need - 1)
            with pytest.raises(nat.GnxError, match='take %d bytes .* above the budget of %d'
                               % (need, need - 1)):
                dev.ld_window(loci, pos, window, None, 40, 0.1, EDGES, BIG)
            assert dev.ld_window_info()['launches'] == 0
            dev.ld_budget(need)                          # a tile with its halo fits exactly
            assert _same(dev.ld_window(loci, pos, window, None, 40, 0.1, EDGES, BIG), whole)
            assert dev.ld_window_info()['locus_blocks'] == blocks
        print('case C: worst score error / bound %.3g' % worst)
    finally:
        dev.ld_budget(0)
        dev.close()


class _Spp:
    """a Species as far as the LD analyses ask: a handle, its individuals in slot order"""
    from geonomics_amd.structs.analyses import SpeciesAnalyses as A
    _prune_ld, _clump, _calc_ld_scores = A._prune_ld, A._clump, A._calc_ld_scores
    _ld_request, _ldw_call, _geno_loci = A._ld_request, A._ldw_call, A._geno_loci
    _LD_MAX_WORK, _LDW_MAX_EDGES = A._LD_MAX_WORK, A._LDW_MAX_EDGES

    def __init__(self, dev, rates):
        self.__dict__.update(_dev=dev, _genomes_assigned=True, gen_arch=self)
        self.recombinations = self
        self._positions, self._rates = np.arange(len(rates)), np.asarray(rates)

    def _geno_sample(self, individs):
        ids = np.arange(self._dev.N, dtype=np.int64) if individs is None else \
            np.sort(np.asarray(individs, dtype=np.int64))
        return ids, ids.copy()


def test_case_d_real_ld_the_whole_edge_list_its_overflow_and_the_greedy_choices():
    """a Wright-Fisher population of 60 after 20 generations at r = 0.01 between neighbours: LD
    is real and the edges many"""
    nat = native()
    bits = T.wright_fisher(60, 300, 0.01, 20, 41)
    gts = W.gts_of_bits(bits)
    assert (T.bits_of(gts) == bits).all()
    dev = _handle(nat, gts)
    try:
        loci, pos = np.arange(300), np.arange(300.0)
        mm = 6                                                   # min_maf 0.05 of 120
        got, ref, worst = _check(dev, gts, loci, pos, 50.0, mm, 0.2, label='case D')
        m = got['n_edges']
        assert m > 300 and got['work'] == (5 + 4) * 2       # 50 loci: a tile and the next one
        with pytest.raises(nat.GnxError, match='exceed max_edges = %d' % (m - 1)) as exc:
            dev.ld_window(loci, pos, 50.0, None, mm, 0.2, m - 1, BIG)
        assert exc.value.n_found == m
        exact = dev.ld_window(loci, pos, 50.0, None, mm, 0.2, m, BIG)
        assert _same(exact, got)
        # ---- prune_ld through the Species method
        spp = _Spp(dev, np.r_[0.0, np.full(299, 0.01)])
        res = spp._prune_ld(r2=0.2, window=50, unit='loci', min_maf=0.05)
        rank = LW.maf_rank(ref['c1'], 120)
        keep, claimed = LW.greedy_independent(300, ref['ei'], ref['ej'], rank)
        kept = ref['kept']
        np.testing.assert_array_equal(res['loci'], np.flatnonzero(kept & keep))
        np.testing.assert_array_equal(res['removed'], np.flatnonzero(kept & ~keep))
        np.testing.assert_array_equal(res['claimed_by'], claimed[kept & ~keep])
        np.testing.assert_array_equal(res['c1'], ref['c1'])
        assert res['n_edges'] == m and res['n_chrom'] == 120 and res['kernel_ms'] > 0
        assert 10 < res['loci'].size < kept.sum() and res['removed'].size > 10
        # the two properties, against the brute r2 matrix
        with np.errstate(invalid='ignore'):
            adj = ref['in_window'] & (ref['r2'] >= 0.2)
        adj = adj | adj.T
        mine = np.ones(300, bool)
        mine[res['removed']] = False
        by = np.full(300, -1, np.int64)
        by[res['removed']] = res['claimed_by']
        W.check_independent(mine, by, rank, adj)
        with pytest.raises(ValueError, match='prune_ld: n_found = %d pairs .* exceed max_edges = 9'
                           % m):
            spp._prune_ld(r2=0.2, window=50, max_edges=9)
        with pytest.raises(ValueError, match='prune_ld: .*exceed max_work = 1: analyse a sample'):
            spp._prune_ld(max_work=1)
        # in map units the same request: 50 loci at r = 0.01 are 0.5 (1 - 0.98^50) in c
        from geonomics_amd.sim import ld as LD
        mpos = LD.map_positions(np.r_[0.0, np.full(299, 0.01)])
        wm = float(mpos[50] - mpos[0]) * (1 + 1e-12)
        inm = spp._prune_ld(r2=0.2, window=wm, unit='morgans', min_maf=0.05)
        refm = LW.brute_window(bits, mpos, wm, mm, 0.2)
        km, _ = LW.greedy_independent(300, refm['ei'], refm['ej'], rank)
        np.testing.assert_array_equal(inm['loci'], np.flatnonzero(kept & km))
        # ---- clump: planted p-values, the hits among every third locus
        rng = np.random.RandomState(2)
        p = rng.uniform(0.02, 1.0, 300)
        hits = rng.choice(300, 60, replace=False)
        p[hits] = 10.0 ** rng.uniform(-8, -2.1, 60)
        p[hits[:4]] = 1e-5                                       # ties: by locus number
        tested = np.ones(300, bool)
        tested[hits[5]] = False
        p[hits[6]] = np.nan
        result = dict(p=np.column_stack([np.ones(300), p]), loci=np.arange(300), tested=tested,
                      ids=np.arange(60), trait_loci=np.sort(hits[:10]))
        cl = spp._clump(result, r=1, p1=1e-4, p2=1e-2, r2=0.3, window=100, unit='loci')
        with np.errstate(invalid='ignore'):
            sel = np.flatnonzero(tested & np.isfinite(p) & (p <= 1e-2))
        assert cl['n_candidates'] == sel.size == 58
        refc = LW.brute_window(bits[:, sel], sel.astype(np.float64), 100.0, 1, 0.3)
        prank = LW.p_rank(p[sel])
        kc, cc = LW.greedy_independent(sel.size, refc['ei'], refc['ej'], prank)
        idx, mem = LW.clumps(p[sel], kc, cc, 1e-4)
        np.testing.assert_array_equal(cl['index_loci'], sel[idx])
        assert cl['index_p'].tobytes() == p[sel][idx].tobytes()
        assert cl['n_clumps'] == idx.size == len(cl['members']) > 3
        for a, b in zip(cl['members'], mem):
            np.testing.assert_array_equal(a, sel[b])
        assert cl['n_edges'] == refc['ei'].size > 0 and sum(x.size for x in cl['members']) > 0
        with np.errstate(invalid='ignore'):
            adjc = refc['in_window'] & (refc['r2'] >= 0.3)
        W.check_independent(kc, cc, prank, adjc | adjc.T)
        assert (np.diff(cl['index_p']) >= 0).all() and (cl['index_p'] <= 1e-4).all()
        want_hit = [bool(np.isin(np.r_[i, m_], hits[:10]).any())
                    for i, m_ in zip(cl['index_loci'], cl['members'])]
        assert cl['trait_loci_hit'].tolist() == want_hit and any(want_hit)
        # ---- LD scores through the Species method
        sc = spp._calc_ld_scores(window=50, unit='loci', min_maf=0.05)
        np.testing.assert_array_equal(sc['partners'], ref['partners'])
        assert sc['score'].tobytes() == got['score'].tobytes()
        want = LW.ld_scores(ref['partners'], ref['score'], kept, 120)
        ok = kept
        assert np.isnan(sc['ld_score'][~ok]).all()
        assert (np.abs(sc['ld_score'][ok] - want[ok]) <= 1e-12 * np.abs(want[ok])).all()
        assert sc['weights'].shape == (300,) and not sc['weights'][~ok].any()
        assert ((sc['weights'][ok] > 0) & (sc['weights'][ok] <= 1)).all()
        assert np.nanmean(sc['ld_score']) > 3                    # LD is real
        print('case D: %d edges, %d of %d loci kept, %d clumps, mean LD score %.2f, worst score '
              'error / bound %.3g' % (m, res['loci'].size, kept.sum(), cl['n_clumps'],
                                      np.nanmean(sc['ld_score']), worst))
    finally:
        dev.close()


def test_refusals_come_before_any_launch(case_a):
    nat, dev, gts, pos = case_a
    loci = np.arange(130)
    before = dev.ld_window(loci, pos, 0.3, None, 2, 0.01, EDGES, BIG)

    def refused(match, *a, **kw):
        with pytest.raises(nat.GnxError, match=match):
            dev.ld_window(*a, **kw)
        assert dev.ld_window_info()['launches'] == 0

    for w in (-1e-9, np.nan, -np.inf):
        refused('window must be >= 0', loci, pos, w, None, 2, 0.01, EDGES, BIG)
    for r in (-0.01, 1.01, np.nan):
        refused('r2_min must be in 0..1', loci, pos, 0.3, None, 2, r, EDGES, BIG)
    for e in (-1, 2 ** 26 + 1):
        refused(r'max_edges must be in 0..2\^26', loci, pos, 0.3, None, 2, 0.01, e, BIG)
    refused('exceed max_work = %d' % (before['work'] - 1), loci, pos, 0.3, None, 2, 0.01, EDGES,
            before['work'] - 1)
    refused('slot out of range', loci, pos, 0.3, np.array([0, dev.N]), 2, 0.01, EDGES, BIG)
    refused('slot 7 is listed twice', loci, pos, 0.3, np.array([7, 3, 7]), 2, 0.01, EDGES, BIG)
    refused('individuals', loci, pos, 0.3, np.zeros(0, np.int64), 2, 0.01, EDGES, BIG)
    bad = loci.copy()
    bad[9] = 130
    refused('locus out of range', bad, pos, 0.3, None, 2, 0.01, EDGES, BIG)
    bad[9] = 8
    refused('locus 8 is listed twice', bad, pos, 0.3, None, 2, 0.01, EDGES, BIG)
    refused('at least one locus', loci[:0], pos[:0], 0.3, None, 2, 0.01, EDGES, BIG)
    p = pos.copy()
    p[50] = p[49] - 1e-9
    refused(r'non-decreasing \(pos\[50\]', loci, p, 0.3, None, 2, 0.01, EDGES, BIG)
    p = pos.copy()
    p[-1] = np.inf
    refused('pos must be finite', loci, p, 0.3, None, 2, 0.01, EDGES, BIG)
    with pytest.raises(ValueError, match='pos'):
        dev.ld_window(loci, pos[:-1], 0.3, None, 2, 0.01, EDGES, BIG)
    exact = dev.ld_window(loci, pos, 0.3, None, 2, 0.01, before['n_edges'], before['work'])
    assert _same(exact, before)
    # r2_min = 1 and window = inf are taken
    dev.ld_window(loci, pos, np.inf, None, 2, 1.0, EDGES, BIG)
    assert _same(dev.ld_window(loci, pos, 0.3, None, 2, 0.01, EDGES, BIG), before)


def test_model_prune_ld_clump_ld_scores_and_ldsc_feed_the_other_analyses():
    import geonomics_amd as gnx
    from test_gpu_ld import _ld_params
    mod = gnx.make_model(_ld_params(8))
    for f in (mod.prune_ld, mod.calc_ld_scores):
        with pytest.raises(ValueError, match='burn the model in first'):
            f()
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(20, 'main', verbose=False)
    spp = mod.comm[0]
    gts = mod.get_genotypes(biallelic=True)
    n = gts.shape[0]
    bits = T.bits_of(gts)
    # ---- prune_ld against the restatement on the downloaded genotypes
    pr = mod.prune_ld(r2=0.1, window=30)
    mm = max(1, int(np.ceil(0.05 * 2 * n - 1e-9)))
    ref = LW.brute_window(bits, np.arange(100.0), 30.0, mm, 0.1)
    keep, _ = LW.greedy_independent(100, ref['ei'], ref['ej'], LW.maf_rank(ref['c1'], 2 * n))
    np.testing.assert_array_equal(pr['loci'], np.flatnonzero(ref['kept'] & keep))
    assert pr['n_edges'] == ref['ei'].size and (pr['ids'] == np.array([*spp])).all()
    assert 2 <= pr['loci'].size <= ref['kept'].sum()
    print('prune_ld: %d edges, %d of %d loci kept' % (pr['n_edges'], pr['loci'].size,
                                                      ref['kept'].sum()))
    # the list goes where loci in linkage equilibrium are expected
    pca = mod.calc_genetic_PCA(n_pcs=2, loci=pr['loci'])
    assert pca[1].shape == (n, 2) and np.isfinite(pca[1]).all()
    anc = mod.calc_ancestry(2, loci=pr['loci'], max_sweeps=20)
    assert np.isfinite(anc['Q']).all()
    grm = mod.calc_grm(loci=pr['loci'])
    assert grm['G'].shape == (n, n) and set(grm['loci_used']) <= set(pr['loci'].tolist())
    # ---- LD scores: the weights go into calc_grm
    sc = mod.calc_ld_scores(window=30)
    refs = LW.brute_window(bits, np.arange(100.0), 30.0, mm, 0.0)
    np.testing.assert_array_equal(sc['partners'], refs['partners'])
    assert (np.abs(sc['score'] - refs['score']) <= W.score_bound(refs)).all()
    want = LW.ld_scores(refs['partners'], refs['score'], refs['kept'], 2 * n)
    k = refs['kept']
    assert (np.abs(sc['ld_score'][k] - want[k]) <= 1e-12 * np.abs(want[k])).all()
    assert sc['weights'].shape == (100,) and sc['n_chrom'] == 2 * n
    wg = mod.calc_grm(weights=sc['weights'])
    assert np.isfinite(wg['G']).all() and wg['G'].shape == (n, n)
    half = mod.calc_ld_scores(window=0.3, unit='c', adjust=False, loci=np.arange(20, 80))
    assert half['loci'].tolist() == list(range(20, 80)) and half['ld_score'].shape == (60,)
    assert not half['weights'][:20].any() and not half['weights'][80:].any()
    # ---- clump a scan: sorted, disjoint clumps under p1
    gw = mod.run_gwas()
    cl = mod.clump(gw, p1=0.05, p2=0.3, r2=0.1, window=30)
    print('clump: %d candidates, %d clumps, %d members' %
          (cl['n_candidates'], cl['n_clumps'], sum(m.size for m in cl['members'])))
    assert cl['n_clumps'] == cl['index_loci'].size == len(cl['members']) >= 1
    assert (np.diff(cl['index_p']) >= 0).all() and (cl['index_p'] <= 0.05).all()
    everything = np.concatenate([cl['index_loci']] + cl['members'])
    assert np.unique(everything).size == everything.size
    assert all((np.diff(m) > 0).all() for m in cl['members'])
    assert cl['trait_loci_hit'].shape == (cl['n_clumps'],)
    pcol = gw['p'][:, 0]
    assert (pcol[cl['index_loci']] == cl['index_p']).all()
    assert all((pcol[m] <= 0.3).all() for m in cl['members'])
    # ---- LD-score regression on the pair
    reg = mod.run_ldsc(gw, sc, n_blocks=20)
    print('run_ldsc: %s' % reg)
    assert all(np.isfinite(reg[k]) for k in ('intercept', 'slope', 'h2', 'intercept_se',
                                             'slope_se', 'h2_se', 'mean_chi2'))
    assert reg['n_blocks'] == 20 and 3 <= reg['n_loci'] <= 100
    assert mod.run_ldsc(gw, sc, n_blocks=10 ** 6)['n_blocks'] == reg['n_loci']
