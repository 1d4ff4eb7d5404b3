"""The block-compaction kernels at the sizes where their tails and clamped loads can go wrong.

k_alive, k_ord_flags, k_ord_write, k_dead_rows, k_pair_flags and k_pair_compact share the
blocking of csrc/gnx_compact.h: a workgroup of 256 threads takes 1024 items, a thread four of
them ("rounds").  k_alive, k_dead_rows and k_pair_flags issue the loads of all four rounds
together, dependency level by level, from indices clamped into the live range; the others go
round by round behind a guard - either way what can go wrong is the tail: the last
partial wave, round and workgroup, a grid that reaches past N, N = 0 under a capacity-sized
grid, an individual without a mate standing in for its mate.  The sizes are the smallest that
reach each of them: one lane, a wave's edge, a round's edge and a workgroup's edge on both
sides, two and three workgroups with a partial last one.  Capacities sit barely above what a
step needs and are no multiple of 1024.

Expected values are the oracle's (oracle/gnx_draws.py, oracle/gnx_oracle.py): the death draws,
the keep draws, the mate choice and the pair rules restated on the host.  Everything goes through
the C-ABI.  Needs an MI355X."""
import numpy as np
import pytest

import gnx_oracle as O
import gnx_draws as D
from test_gpu_parity import make_dev, upload_simple, native

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 3071]
R = 2.0                      # mating radius
PITCH = 4.0                  # clumps sit on a grid of this pitch, members within 0.4 of a node


def _cap(n):
    """room for n individuals and a step's births - one per pair; the tests that let a step give
    birth thin the pairs with b = 0.2, far below every second individual - odd: no multiple of
    1024 (a step whose births do not fit fails loudly)"""
    return (n + n // 2 + 3) | 1


def _clumps(rng, n, sizes=(2, 3, 1, 2, 2, 4)):
    """n individuals in clumps of the given sizes (cycled), one clump per node of a grid whose
    pitch is twice the mating radius: everybody in a clump is within 1.14 of everybody else in it
    (< R) and at least 3.2 from anybody outside (> R) - no distance anywhere near the radius, so
    the oracle's neighbour sets are the device's whatever the rounding.  Couples are each
    other's only choice (a reciprocal pair whenever both are kept), a clump of one has no
    neighbour.  Returns x, y, ids (ascending, sparse), the clump of everybody, W = H."""
    clump = []
    k = 0
    while len(clump) < n:
        clump += [k] * sizes[k % len(sizes)]
        k += 1
    clump = np.array(clump[:n])
    side = int(np.ceil(np.sqrt(clump.max() + 1)))
    W = int(PITCH * side)
    cx = (clump % side) * PITCH + PITCH / 2
    cy = (clump // side) * PITCH + PITCH / 2
    x = (cx + (rng.rand(n) - 0.5) * 0.8).astype(np.float32)
    y = (cy + (rng.rand(n) - 0.5) * 0.8).astype(np.float32)
    ids = np.sort(rng.choice(10 ** 6, n, replace=False)) + 1000
    perm = rng.permutation(n)             # storage order is not clump order
    return x[perm], y[perm], ids, clump[perm], max(W, 8)


# ------------------------------------------------------------------ death draws: k_alive
@pytest.mark.parametrize('d', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('n', SIZES)
def test_death_draws_at_the_tails(n, d):
    """the survivors' ids are {id : death_draws(seed, id, step) >= d} (d_min = d_max = d: the
    same death probability for everybody, as in test_death_draws_match_oracle).  d = 0: nobody
    dies; d = 1: everybody does - a total of 0 and every row freed."""
    nat = native()
    rng = np.random.RandomState(1000 + n)
    seed, step = 99, 12
    x, y, ids, _, W = _clumps(rng, n)
    dev = make_dev(W, W, cap=_cap(n), seed=seed, mating_radius=R, d_min=d, d_max=d)
    upload_simple(dev, x, y, ids=ids)
    dev.step_index = step
    dev.pop_dynamics_mate(True)
    id_before = dev.download(nat.F_ID)
    assert id_before.size == n + dev.counts()[1] and _cap(n) % 1024 != 0
    dev.pop_dynamics_die(True, False)
    id_after = dev.download(nat.F_ID)
    u = D.death_draws(seed, id_before, step)
    exp = np.sort(id_before[~(u.astype(np.float64) < d)])
    np.testing.assert_array_equal(np.sort(id_after), exp)
    assert dev.counts()[0] == exp.size and dev.counts()[2] == id_before.size - exp.size
    if d == 0.0:
        assert exp.size == id_before.size
    if d == 1.0:
        assert exp.size == 0 and dev.N == 0
    dev.close()


@pytest.mark.parametrize('n', SIZES)
def test_named_dead_at_the_tails(n):
    """gnx_op_mortality with a mask whose first and last individual are dead: the survivors, in
    their order, with their genome rows' contents; the dead's rows are free again"""
    nat = native()
    rng = np.random.RandomState(2000 + n)
    L = 96
    x, y, ids, _, W = _clumps(rng, n)
    dev = make_dev(W, W, L=L, cap=n + 2 if (n + 2) % 1024 else n + 3, mating_radius=R)
    upload_simple(dev, x, y, ids=ids)
    g = (rng.rand(n, L, 2) < 0.5).astype(np.uint8)
    dev.upload_genomes(O.pack_genomes(g))
    dev.set_recomb_paths(O.pack_bits(np.zeros((1, L), np.uint8)))
    dead = rng.rand(n) < 0.3
    dead[0] = dead[-1] = True
    dev.op_mortality(dead)
    assert dev.N == (~dead).sum()
    np.testing.assert_array_equal(dev.download(nat.F_ID), ids[~dead])
    np.testing.assert_array_equal(dev.download(nat.F_X), x[~dead])
    if dev.N:
        np.testing.assert_array_equal(O.unpack_genomes(dev.download(nat.F_GENO), L), g[~dead])
        rows = dev.download(nat.F_GROW)
        assert rows.min() >= 0 and np.unique(rows).size == rows.size
    # the freed rows serve again: as many offspring as there were dead fit the rows (the handle
    # has n + 2 of them)
    B = int(dead.sum()) if dev.N else 0
    if B:
        n2 = dev.N
        ps = rng.randint(0, n2, (B, 2))
        dev.op_crossover(ps, np.zeros(ps.shape), np.zeros(ps.shape))
        G3 = O.unpack_genomes(dev.download(nat.F_GENO), L)
        np.testing.assert_array_equal(G3[:n2], g[~dead])
        np.testing.assert_array_equal(G3[n2:, :, 0], g[~dead][ps[:, 0], :, 0])
        rows = dev.download(nat.F_GROW)
        assert np.unique(rows).size == rows.size
    dev.close()


# ------------------------------------------------------------------ pair list: k_pair_flags, k_pair_compact
def _pairs_by_id(dev, nat, pairs):
    id_s = dev.download(nat.F_ID)                       # slot order after the cell sort
    return [(int(id_s[a]), int(id_s[b])) for a, b in pairs], id_s


def _expected_pairs(x, y, ids, W, seed, step, keep, sexed=False, sex=None):
    """the oracle's pair list as (focal id, mate id): the mate choice restated from the focal
    individuals' own streams, the thinning, and the pair rules"""
    mate = O.choose_mates(x, y, ids, R, seed, step, mode='uniform', dim=(W, W))
    if sexed:
        pr = O.sexed_pairs(mate, keep, sex)
    else:
        pr = O.pairs_from_mates(mate, keep, ids=ids)
    return {(int(ids[a]), int(ids[b])) for a, b in pr}, mate


@pytest.mark.parametrize('b', [0.35, 1.0])
@pytest.mark.parametrize('n', SIZES)
def test_pair_list_at_the_tails(n, b):
    """focal ids = kept and has a mate, minus the reciprocal duplicate with the larger id -
    here the whole pairs, (focal id, mate id), against the oracle's.  The kernel no longer
    draws the thinning in the radius path (the mate list implies it): the expectation does,
    from oracle/gnx_draws.py.  b = 1 keeps everybody: every couple is a reciprocal pair and the
    rare branch runs in most waves."""
    nat = native()
    rng = np.random.RandomState(3000 + n)
    seed, step = 5150, 3
    x, y, ids, clump, W = _clumps(rng, n)
    dev = make_dev(W, W, cap=_cap(n), seed=seed, mating_radius=R, b=b)
    upload_simple(dev, x, y, ids=ids)
    dev.step_index = step
    mate, pairs = dev.op_find_pairs()
    got, id_s = _pairs_by_id(dev, nat, pairs)
    keep = D.keep_draws(seed, ids, step, b)
    exp, mate_o = _expected_pairs(x, y, ids, W, seed, step, keep)
    assert len(got) == len(set(got))
    assert set(got) == exp
    # who was searched for: the kept individuals with somebody in their clump, nobody else
    size = np.bincount(clump)[clump]
    pos = {int(i): k for k, i in enumerate(ids)}
    o = np.array([pos[int(i)] for i in id_s])           # slot -> original index
    np.testing.assert_array_equal(mate >= 0, (keep & (size > 1))[o])
    if b == 1.0 and n >= 63:
        assert keep.all() and len(exp) < (size > 1).sum()       # reciprocal pairs were dropped
    dev.close()


def test_pair_list_injected_keep():
    """gnx_op_find_pairs(keep): the caller's mask instead of the draw, in both kernels' stead"""
    nat = native()
    n = 1025
    rng = np.random.RandomState(41)
    seed, step = 77, 5
    x, y, ids, clump, W = _clumps(rng, n)
    dev = make_dev(W, W, cap=_cap(n), seed=seed, mating_radius=R, b=0.9)
    upload_simple(dev, x, y, ids=ids)
    dev.step_index = step
    keep = rng.rand(n) < 0.6
    keep[-1] = keep[0] = True
    # (the mask is by slot of the population as uploaded: ascending ids, the order a sort by
    # (cell, id) does not keep - so name the individuals through their slots after a sort)
    dev.op_find_pairs()                                  # sorts by cell
    id_s = dev.download(nat.F_ID)
    pos = {int(i): k for k, i in enumerate(ids)}
    o = np.array([pos[int(i)] for i in id_s])
    mate, pairs = dev.op_find_pairs(keep[o])
    got, id_s2 = _pairs_by_id(dev, nat, pairs)
    np.testing.assert_array_equal(id_s2, id_s)           # (already sorted: nobody moved)
    exp, _ = _expected_pairs(x, y, ids, W, seed, step, keep)
    assert len(got) == len(set(got)) and set(got) == exp
    assert ((mate >= 0) <= keep[o]).all()
    dev.close()


def test_pair_list_sexed():
    """a sexed species: female focal, male mate, no de-duplication (ops/mating.py:41-55)"""
    nat = native()
    n = 2049
    rng = np.random.RandomState(42)
    seed, step, b = 31, 8, 0.8
    x, y, ids, clump, W = _clumps(rng, n)
    sex = rng.randint(0, 2, n).astype(np.uint8)
    dev = make_dev(W, W, cap=_cap(n), seed=seed, mating_radius=R, b=b, sexed=1)
    upload_simple(dev, x, y, ids=ids, sex=sex)
    dev.step_index = step
    mate, pairs = dev.op_find_pairs()
    got, _ = _pairs_by_id(dev, nat, pairs)
    keep = D.keep_draws(seed, ids, step, b)
    exp, _ = _expected_pairs(x, y, ids, W, seed, step, keep, sexed=True, sex=sex)
    assert len(got) == len(set(got)) and set(got) == exp and len(exp) > 100
    dev.close()


def test_pair_list_panmixia_still_draws_the_thinning():
    """mating at any distance: k_panmixia draws both members of every trial, and the Bernoulli(b)
    thinning is k_pair_flags' own draw - the pair list is the kept trials, in trial order"""
    nat = native()
    n = 1025
    rng = np.random.RandomState(43)
    seed, step, b = 21, 2, 0.3
    x, y, ids, _, W = _clumps(rng, n)
    dev = make_dev(W, W, cap=_cap(n), seed=seed, mating_radius=-1.0, b=b)
    upload_simple(dev, x, y, ids=ids)
    dev.step_index = step
    mate, pairs = dev.op_find_pairs(None)
    ids_now = dev.download(nat.F_ID)
    f, m = D.panmixia_draws(seed, ids_now, step, n)
    keep = D.keep_draws(seed, ids_now, step, b)
    sel = keep & (f != m)
    np.testing.assert_array_equal(pairs, np.stack([f[sel], m[sel]], 1))
    assert 0 < len(pairs) < n and abs(len(pairs) - b * n) < 5 * np.sqrt(n * b * (1 - b))
    dev.close()


@pytest.mark.parametrize('n', [1, 257, 1025])
def test_pair_list_nobody_has_a_neighbour(n):
    """every mate == -1: zero pairs, and no births in a whole mating step"""
    rng = np.random.RandomState(44 + n)
    x, y, ids, clump, W = _clumps(rng, n, sizes=(1,))
    dev = make_dev(W, W, cap=_cap(n), seed=3, mating_radius=R, b=1.0)
    upload_simple(dev, x, y, ids=ids)
    dev.step_index = 4
    mate, pairs = dev.op_find_pairs()
    assert (mate == -1).all() and len(pairs) == 0
    assert (O.choose_mates(x, y, ids, R, 3, 4, mode='uniform', dim=(W, W)) == -1).all()
    dev.pop_dynamics_mate(True)
    assert dev.counts()[0] == n and dev.counts()[1] == 0
    dev.close()


# ------------------------------------------------------------------ index compaction, the dead's rows
BIG = 1 << 20          # slots: above the lazy walk's threshold (600 000), bench.py's path
L_WALK = 320


def _model(n, cap, seed=17, shuffle=False, **sp_kw):
    """n founders with genomes of L_WALK loci and one trait on a 48 x 48 two-layer landscape,
    carrying capacity ~n"""
    nat = native()
    W = H = 48
    rng = np.random.RandomState(seed)
    rasts = np.stack([np.ones((H, W)), np.tile(np.linspace(0, 1, W), (H, 1))]).astype(np.float32)
    dev = nat.Device(W, H, 2, L=L_WALK, n_traits=1, cap_inds=cap, cap_rows=min(cap, 16384),
                     seed=seed)
    dev.upload_rasters(rasts)
    kw = dict(mating_radius=3.0, K_factor=max(n, 40) / float(W * H))
    kw.update(sp_kw)
    dev.set_species_params(nat.default_species_params(**kw))
    loci = np.sort(rng.choice(L_WALK, 8, replace=False))
    dev.set_trait(0, loci, 0.1 * np.where(np.arange(8) % 2, -1.0, 1.0), 1, 0.05, 1.0, False)
    cross = (rng.rand(16, L_WALK) < 2.0 / L_WALK).astype(np.uint8)
    cross[:, 0] = 0
    dev.set_recomb_paths(O.pack_bits(O.recomb_paths(cross)))
    ids = np.arange(n) * 3 + 7
    if shuffle:
        ids = ids[rng.permutation(n)]
    dev.upload_population(rng.rand(n) * W, rng.rand(n) * H, rng.randint(0, 4, n), np.zeros(n), ids)
    g = (rng.rand(n, L_WALK, 2) < 0.5).astype(np.uint8)
    dev.upload_genomes(O.pack_genomes(g))
    dev.set_z()
    dev.set_defer_crossover(True)
    dev.reset_path_counts()
    return dev, nat


def _state(dev, nat):
    ids = dev.download(nat.F_ID)
    o = np.argsort(ids)
    out = dict(ids=ids[o], x=dev.download(nat.F_X)[o], y=dev.download(nat.F_Y)[o],
               age=dev.download(nat.F_AGE)[o], z=dev.download(nat.F_Z)[:, o])
    if ids.size:
        out['g'] = dev.download(nat.F_GENO)[o]
        rows = dev.download(nat.F_GROW)
        assert rows.min() >= 0 and np.unique(rows).size == rows.size
    return out


def _walk_against_steps(a, b, nat, T):
    """a.walk(T) against T single steps of b: the counts of every step, then everybody by id"""
    a.walk(T, False, True)
    got = [tuple(int(v) for v in r) for r in zip(*a.walk_history())]
    hist = []
    for _ in range(T):
        n0 = b.N
        b.step(False, True)
        hist.append((n0,) + tuple(int(v) for v in b.counts()[1:]))
    assert got == hist
    assert a.counts() == b.counts()
    sa, sb = _state(a, nat), _state(b, nat)
    assert set(sa) == set(sb)
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    return hist


@pytest.mark.parametrize('case', ['n257', 'n1025', 'n3071', 'no_births', 'fresh_upload'])
def test_lazy_walk_index_and_dead_rows(case):
    """walk(5) on a handle of 2^20 slots - lazy mortalities (k_dead_rows: nobody moves, the
    dead's rows go back), the index compacted from the death draws' flags (k_ord_flags,
    k_ord_write), the next movement launched ahead - leaves the population five single steps
    leave on a twin: positions, ages, phenotypes, genome rows' contents, counts per step.
    no_births: b = 0, no step has births - the index has no identity tail behind it.
    fresh_upload: founders uploaded in arbitrary id order and walked at once - the index is
    rebuilt by the first cell sort, not carried over."""
    n = dict(n257=257, n1025=1025, n3071=3071, no_births=1025, fresh_upload=1023)[case]
    kw = dict(b=0.0) if case == 'no_births' else {}
    a, nat = _model(n, BIG, shuffle=case == 'fresh_upload', **kw)
    b, _ = _model(n, BIG, shuffle=case == 'fresh_upload', **kw)
    if case != 'fresh_upload':
        for dev in (a, b):                 # a step first: the index exists, with a tail of newborns
            dev.step(False, True)
        a.reset_path_counts()
    hist = _walk_against_steps(a, b, nat, 5)
    assert all(h[2] > 0 for h in hist), hist                     # somebody died in every step
    if case == 'no_births':
        assert all(h[1] == 0 for h in hist), hist
    else:
        assert sum(h[1] for h in hist) > 0, hist
    pa, pb = a.path_counts(), b.path_counts()
    assert pa['lazy_mortalities'] == 4 and pa['moves_ahead'] == 4 and pa['make_dense'] == 0, pa
    assert pb['lazy_mortalities'] == 0 and pb['moves_ahead'] == 0, pb
    a.close()
    b.close()


# ------------------------------------------------------------------ the device-driven step
def test_device_driven_twin_at_a_workgroup_edge(monkeypatch):
    """GNX_DD=2: the device-driven step - the same kernels with every count read from the device
    block, under grids sized by the capacity - at N = 1025, against single host-driven steps"""
    monkeypatch.setenv('GNX_DD', '2')
    a, nat = _model(1025, 4099)
    b, _ = _model(1025, 4099)
    hist = _walk_against_steps(a, b, nat, 5)
    assert sum(h[1] for h in hist) > 0 and all(h[2] > 0 for h in hist), hist
    # (a walk's last step is host-driven: it compacts and reads the counts back)
    assert a.totals()['dd_steps'] == 4 and b.totals()['dd_steps'] == 0
    a.close()
    b.close()


def test_device_driven_walk_through_extinction(monkeypatch):
    """a population that dies out inside a device-driven walk: N == 0 under a capacity-sized grid
    in every kernel of the steps that follow.  The walk ends clean, with zero counts"""
    monkeypatch.setenv('GNX_DD', '2')
    deadly = dict(d_min=0.97, d_max=1.0)
    a, nat = _model(1025, 4099, **deadly)
    b, _ = _model(1025, 4099, **deadly)
    hist = _walk_against_steps(a, b, nat, 6)
    assert hist[0][0] == 1025 and hist[-1] == (0, 0, 0), hist
    assert a.N == 0 and a.counts() == (0, 0, 0)
    # every step but the walk's last was device-driven, those after the extinction included
    assert a.totals()['dd_steps'] == 5 and hist[4] == (0, 0, 0), hist
    a.walk(2, False, True)                              # a walk of the empty handle is a no-op
    assert [tuple(int(v) for v in r) for r in zip(*a.walk_history())] == [(0, 0, 0)] * 2
    a.close()
    b.close()
