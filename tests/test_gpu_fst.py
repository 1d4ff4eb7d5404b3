"""gnx_stats_group_counts (csrc/gnx_group_counts.hip) and what stands on it - Device.
stats_group_counts, Species._group_counts, Model.calc_fst / calc_diversity / calc_sfs - against
counts taken with numpy from the downloaded genomes.  Every count comparison is integer
equality.  Needs an MI355X.

The kernel flushes its bit-sliced counters after FLUSH = 511 individuals of a group (2^9 - 1:
GC_CHUNK); a larger group spans several chunks, whose counts meet in the atomic adds."""
import numpy as np
import pytest

import gnx_oracle as O
from test_gpu_parity import native
from test_fst_host import assert_meets_reference, counts_numpy, fixture
from geonomics_amd.sim import fst as F

pytestmark = pytest.mark.gpu

FLUSH = 511
U53 = 2.0 ** -53


def _unpack(packed, L):
    """genotypes uint8 [n][L][2] of packed genomes uint64 [n][2][W64]"""
    by = np.ascontiguousarray(packed).view(np.uint8).reshape(packed.shape[0], 2, -1)
    return np.transpose(np.unpackbits(by, axis=2, bitorder='little')[:, :, :L], (0, 2, 1))


def _handle(nat, gts, ids=None, W=24, H=24, seed=20, cap=None, cap_rows=None, paths=None,
            K_factor=1.0):
    """a population with genotypes gts [n][L][2] on a handle over a flat W x H landscape"""
    n, L = gts.shape[:2]
    rng = np.random.RandomState(seed)
    cap = n + 64 if cap is None else cap
    dev = nat.Device(W, H, 1, L=L, cap_inds=cap, cap_rows=cap if cap_rows is None else cap_rows,
                     seed=seed)
    dev.upload_rasters(np.ones((1, H, W), np.float32))
    dev.set_species_params(nat.default_species_params(mating_radius=3.0, K_factor=K_factor))
    if paths is not None:
        dev.set_recomb_paths(paths)
    dev.upload_population((rng.rand(n) * W).astype(np.float32), (rng.rand(n) * H).astype(np.float32),
                          rng.randint(0, 4, n), np.zeros(n), np.arange(n) if ids is None else ids)
    dev.upload_genomes(O.pack_genomes(gts.astype(np.uint8)))
    return dev


def _random_gts(rng, n, L):
    """clines of allele frequency over the individuals, and loci fixed at 0 and at 1"""
    p = np.clip(rng.uniform(0, 1, L)[None, :] + rng.uniform(-0.5, 0.5, L)[None, :]
                * np.linspace(-1, 1, n)[:, None], 0, 1)
    p[:, ::17] = 0.0
    p[:, 5::29] = 1.0
    return (rng.rand(n, L, 2) < p[:, :, None]).astype(np.uint8)


def _expected(dev, slots, group_start):
    gts = _unpack(dev.download_genomes(np.asarray(slots, np.int64)), dev.L).astype(np.int64)
    G = len(group_start) - 1
    c1, ch = np.zeros((G, dev.L), np.int32), np.zeros((G, dev.L), np.int32)
    for g in range(G):
        part = gts[group_start[g]:group_start[g + 1]]
        c1[g] = part.sum(axis=(0, 2))
        ch[g] = (part.sum(axis=2) == 1).sum(axis=0)
    return c1, ch


def _check(dev, slots, group_start):
    c1, ch = dev.stats_group_counts(slots, group_start)
    e1, eh = _expected(dev, slots, group_start)
    assert c1.dtype == ch.dtype == np.int32 and c1.shape == ch.shape == e1.shape
    np.testing.assert_array_equal(c1, e1)
    np.testing.assert_array_equal(ch, eh)
    c1b, chb = dev.stats_group_counts(slots, group_start)       # back to back: the same
    np.testing.assert_array_equal(c1b, c1)
    np.testing.assert_array_equal(chb, ch)
    return c1, ch


@pytest.fixture(scope='module')
def small():
    """L = 200 (one block, the last word partial), n = 131"""
    nat = native()
    gts = _random_gts(np.random.RandomState(1), 131, 200)
    dev = _handle(nat, gts)
    yield nat, dev, gts
    dev.close()


def test_uneven_groups_an_empty_group_and_slots_out_of_order(small):
    nat, dev, gts = small
    rng = np.random.RandomState(2)
    slots = rng.permutation(131)[:111]                # 20 individuals in no group, no slot order
    assert (np.diff(slots) < 0).any()
    group_start = np.array([0, 70, 70, 103, 111])     # 70, none, 33 and 8 individuals
    c1, ch = _check(dev, slots, group_start)
    assert (c1[1] == 0).all() and (ch[1] == 0).all() and c1[[0, 2, 3]].any(axis=1).all()
    # the upload itself, not only the download, is what was counted
    lab = np.full(131, -1)
    for g in range(4):
        lab[slots[group_start[g]:group_start[g + 1]]] = g
    n, e1, eh = counts_numpy(gts, lab, 4)
    np.testing.assert_array_equal(c1, e1)
    np.testing.assert_array_equal(ch, eh)
    # nobody in any group, and a single group of nobody
    c1, ch = dev.stats_group_counts(np.zeros(0, np.int64), [0, 0, 0])
    assert c1.shape == (2, 200) and not c1.any() and not ch.any()


def test_one_group_of_everybody_equals_locus_counts(small):
    nat, dev, gts = small
    c1, ch = dev.stats_group_counts(np.arange(dev.N), [0, dev.N])
    l1, lh = dev.stats_locus_counts()
    np.testing.assert_array_equal(c1[0], l1)
    np.testing.assert_array_equal(ch[0], lh)


@pytest.mark.parametrize('L', [4096, 4097])
def test_whole_waves_of_words(L):
    """L = 4096: 64 words exactly (one wave's tile), no padding; 4097: one locus more"""
    nat = native()
    gts = _random_gts(np.random.RandomState(L), 70, L)
    gts[:, -1] = np.random.RandomState(3).randint(0, 2, (70, 2))
    dev = _handle(nat, gts)
    try:
        assert dev.W64 >= (L + 63) // 64
        slots = np.random.RandomState(4).permutation(70)
        c1, ch = _check(dev, slots, [0, 1, 30, 70])
        assert c1[:, -1].sum() == gts[:, -1].sum()
        l1, lh = dev.stats_locus_counts()
        np.testing.assert_array_equal(c1.sum(axis=0), l1)
        np.testing.assert_array_equal(ch.sum(axis=0), lh)
    finally:
        dev.close()


def test_walked_relatives_across_blocks_with_a_pending_crossover():
    """L = 10 000: 157 words in blocks that a wave's 64 words cross; n = 700 uploaded, then
    walks on a 2^20-slot handle (the product path: every step of a walk but its last leaves the
    dead in their slots, the crossover is deferred, children share blocks with their parents)
    with mutations between them, and the call made with this step's offspring still waiting
    for their genomes.  Groups of 1, 2 and more than one flush interval.

    Dead individuals sitting in their slots AT the call cannot be presented through the API:
    holes exist only between the steps of a walk, and every exit of a walk - its last step, and
    its error exit (test_gpu_deferred.py::test_walk_many_failure_leaves_other_handles_dense) -
    gathers the living into slots [0, N).  The walks here do go through that state (asserted on
    path_counts: lazy mortalities happened), and the entry point's gnx_l_make_dense is a
    defensive no-op like geno_ready's (asserted: it gathered nothing)."""
    nat = native()
    L = 10000
    rng = np.random.RandomState(7)
    cross = (rng.rand(64, L) < 1.0 / L).astype(np.uint8)
    cross[:, 0] = 0
    paths = O.pack_bits(O.recomb_paths(cross))
    dev = _handle(nat, _random_gts(rng, 700, L), W=28, H=28, cap=1 << 20, cap_rows=4096,
                  paths=paths)
    try:
        info = dev.genome_info()
        assert info['NB'] > 1 and info['BW'] < 64, info     # a wave's 64 words cross blocks
        dev.set_defer_crossover(True)
        for T in (3, 2, 3):
            dev.walk(T, False, False)
            who = rng.choice(dev.N, 5, replace=False).astype(np.int64)
            dev.mutate(who, rng.randint(1, L, 5).astype(np.int32),
                       rng.randint(0, 2, 5).astype(np.uint8))
        dev.age()
        dev.move()
        dev.pop_dynamics_mate(False)
        N = dev.N
        assert dev.counts()[1] > 0 and dev.genome_info()['deferred'] == 1
        assert dev.totals()['deaths'] > 0                           # some have died
        pc = dev.path_counts()
        assert pc['lazy_mortalities'] > 0, pc           # ... and were left in their slots
        assert N >= FLUSH + 60, N
        slots = rng.permutation(N)
        big = FLUSH + 30                               # two chunks: 511 and 30
        group_start = np.array([0, 1, 3, 3 + big, N])
        c1, ch = dev.stats_group_counts(slots, group_start)
        assert dev.genome_info()['deferred'] == 0      # the call cut the pending births
        assert dev.path_counts()['make_dense'] == 0    # ... and found the living in [0, N)
        e1, eh = _expected(dev, slots, group_start)
        np.testing.assert_array_equal(c1, e1)
        np.testing.assert_array_equal(ch, eh)
        assert dev.N == N
        l1, lh = dev.stats_locus_counts()
        np.testing.assert_array_equal(c1.sum(axis=0), l1)
        np.testing.assert_array_equal(ch.sum(axis=0), lh)
        c1, ch = dev.stats_group_counts(np.arange(N), [0, N])       # G = 1, several chunks
        np.testing.assert_array_equal(c1[0], l1)
        np.testing.assert_array_equal(ch[0], lh)
    finally:
        dev.close()


def test_every_refusal_leaves_the_handle_alone(small):
    nat, dev, gts = small
    before = dev.stats_locus_counts()
    N = dev.N
    ok = np.arange(10)
    for slots, gs, msg in (
            (ok, [0], '1..1024 groups'),                               # G = 0
            (ok, np.zeros(1026, np.int64), '1..1024 groups'),          # G = 1025
            (ok, [1, 10], 'start at 0'),
            (ok, [0, 9], 'end at n'),
            (ok, [0, 7, 5, 10], 'decreases'),
            (np.array([0, 1, N]), [0, 3], 'slot out of range'),
            (np.array([0, -1, 2]), [0, 3], 'slot out of range'),
            (np.array([0, 2 ** 40]), [0, 2], 'slot out of range')):
        with pytest.raises(nat.GnxError, match=msg):
            dev.stats_group_counts(slots, gs)
    # a group of 2^30 individuals, through the library itself: group_start is checked before
    # any slot is read (the order of the checks in gnx_stats_group_counts), so one slot stands
    # in for the 2^30 the call announces; nothing is written to the one-element outputs
    import ctypes as C
    one, gs = np.zeros(1, np.int32), np.array([0, 2 ** 30], np.int64)
    o1, oh = np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    rc = dev.lib.gnx_stats_group_counts(dev.h, C.c_int64(2 ** 30), nat._ptr(one),
                                        C.c_int32(1), nat._ptr(gs),
                                        nat._ptr(o1), nat._ptr(oh))
    assert rc == 1 and o1[0] == oh[0] == -7
    assert b'group 0 holds 2^30 individuals or more' in dev.lib.gnx_last_error()
    gs[1] = 2 ** 30 - 1                              # one fewer passes that check: the slots
    rc = dev.lib.gnx_stats_group_counts(dev.h, C.c_int64(2 ** 30 - 1),     # are looked at next
                                        nat._ptr(np.full(1, -1, np.int32)),
                                        C.c_int32(1), nat._ptr(gs),
                                        nat._ptr(o1), nat._ptr(oh))
    assert rc == 1 and b'slot out of range' in dev.lib.gnx_last_error() and o1[0] == -7
    # G * L above the cap of 2^26 counts per table: a handle with L = 70 000 and 1000 groups
    wide = nat.Device(16, 16, 1, L=70000, cap_inds=64, cap_rows=64, seed=1)
    wide.upload_rasters(np.ones((1, 16, 16), np.float32))
    wide.set_species_params(nat.default_species_params())
    wide.upload_population(np.ones(4), np.ones(4), np.zeros(4), np.zeros(4), np.arange(4))
    with pytest.raises(nat.GnxError, match='genomes not assigned'):
        wide.stats_group_counts(np.arange(4), [0, 4])
    wide.upload_genomes(np.zeros((4, 2, wide.W64), np.uint64))
    with pytest.raises(nat.GnxError, match='at most 67108864'):
        wide.stats_group_counts(np.arange(4), np.minimum(np.arange(1001), 4))
    wide.close()
    after = dev.stats_locus_counts()
    np.testing.assert_array_equal(before[0], after[0])
    np.testing.assert_array_equal(before[1], after[1])


def test_end_to_end_on_the_reference_fixture():
    """the fixture's genotypes uploaded: device counts -> fst_hsht is the host path's result
    bit for bit (the same integers through the same function) and meets the reference"""
    nat = native()
    fx = fixture()
    dev = _handle(nat, fx['genotypes'], ids=fx['ids'])
    try:
        names, order, gs = F.make_groups(fx['ids'], fx['labels'])
        c1, ch = dev.stats_group_counts(order, gs)           # uploaded in id order: slot = rank
        n, e1, eh = counts_numpy(fx['genotypes'], fx['labels'])
        np.testing.assert_array_equal(np.diff(gs), n)
        np.testing.assert_array_equal(c1, e1)
        np.testing.assert_array_equal(ch, eh)
        for est in (False, True):
            for a, b in fx['pairs']:
                np.testing.assert_array_equal(
                    F.fst_hsht(c1, ch, n, int(a), int(b), est_Hs=est),
                    F.fst_hsht(e1, eh, n, int(a), int(b), est_Hs=est))
        worst = assert_meets_reference(fx, c1, ch, n)
        print('device counts -> fst_hsht against the reference: worst error / bound %.3g' % worst)
    finally:
        dev.close()


def test_model_calc_fst_diversity_and_sfs():
    import geonomics_amd as gnx
    from test_gpu_model_api import small_params
    mod = gnx.make_model(small_params(T=6))
    mod.walk(10000, 'burn', verbose=False)
    mod.walk(4, 'main', verbose=False)
    spp = mod.comm[0]
    gts = mod.get_genotypes(biallelic=True).astype(np.uint8)
    nn, L = gts.shape[:2]
    lab = mod.group_by_grid(2, 1)
    assert lab.shape == (nn,) and set(np.unique(lab)) == {0, 1}
    np.testing.assert_array_equal(lab, (mod.get_x() >= 15).astype(int))
    n, e1, eh = counts_numpy(gts, lab)
    res = mod.calc_fst(lab, mean=False)
    assert [*res] == [(0, 1)]
    np.testing.assert_array_equal(res[(0, 1)], F.fst_hsht(e1, eh, n, 0, 1))
    assert mod.calc_fst(lab)[(0, 1)] == np.nanmean(F.fst_hsht(e1, eh, n, 0, 1))
    # the dict form, with a few individuals in no group, and a subset of the loci
    ids = np.array([*spp])
    groups = {'west': ids[lab == 0][3:], 'east': ids[lab == 1][:-2]}
    lab2 = np.full(nn, -1)
    lab2[np.flatnonzero(lab == 1)[:-2]] = 0           # 'east' sorts first
    lab2[np.flatnonzero(lab == 0)[3:]] = 1
    n2, f1, fh = counts_numpy(gts[:, 5:40], lab2)
    got = mod.calc_fst(groups, loci=np.arange(5, 40), method='hudson', mean=False)
    num, den = F.fst_hudson(f1, n2, 0, 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        np.testing.assert_array_equal(got[('east', 'west')], num / den)
    # by layer: lyr_1 rises from 0 to 1 with x
    labl = mod.group_by_layer('lyr_1', [0.0, 0.3, 0.6])
    e = mod.get_e()[:, 1]
    np.testing.assert_array_equal(labl, np.where(e >= 0.6, -1, np.digitize(e, [0.0, 0.3, 0.6]) - 1))
    assert (labl == -1).any() and (labl == 0).any() and (labl == 1).any()
    # everybody as one group: Ho is _calc_het's mean, pi the brute-force sum
    d = mod.calc_diversity()
    assert d['n'][0] == nn and d['names'] == [0]
    from geonomics_amd.sim import stats as S
    het = S._calc_het(spp, mean=True)
    # both are means over L terms cnt_het / n of the same integers
    assert abs(d['Ho'][0] - het) <= L * U53 * het
    c = gts.astype(np.int64).sum(axis=(0, 2))
    m = 2 * nn
    terms = c * (m - c) / (m * (m - 1) / 2)
    assert abs(d['pi'][0] - terms.sum()) <= L * U53 * np.abs(terms).sum()
    names, s = mod.calc_sfs(lab, folded=True)
    assert names == [0, 1] and (s.sum(axis=1) == L).all()
    np.testing.assert_array_equal(s, F.sfs(e1, n, folded=True))
