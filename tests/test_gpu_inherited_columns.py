"""Inherited phenotypes, habitat values and fitness of the living, against the oracle, on every
path that takes a time step.

An offspring's alleles at the selected loci come from its parents' compact table
(GnxSoA.tb) inside k_offspring, its z from those words, its fit from e, z and the table's
deleterious bits - usually before it has a genome row at all - and afterwards the cell sort,
the compactions, the lazy walk's gather and the tile staging carry tb, z and e from slot to
slot.  Nothing recomputes them.  Here every checkpoint downloads the columns of everybody
alive and tests/_columns.py recomputes them in f64 from the position, the rasters and the
genome row (tests/test_columns_host.py shows that checker to be sharp).  The architectures
each cross one threshold of the code: a full table word, the second and third word, the
fifth layer and trait (GnxRec keeps four of each in registers, gnx_rec_rest copies the rest),
GNX_MAX_TRAITS, fitness from the table alone.  Needs an MI355X."""
import threading

import numpy as np
import pytest

import gnx_oracle as O
from _columns import check_columns
from test_gpu_parity import native
from test_gpu_product_path import HostGenomes

pytestmark = pytest.mark.gpu

W = H = 40
N0 = 1500
L = 5000            # ragged: 78 words + 8 bits (W64 = 80)
FORCED = [0, 63, 64, L - 1]

# name -> layers, loci per trait, deleterious loci, dominance
SPECS = {
    'small': (2, [12, 1], 5, True),         # n_sel 18, TW 1: monogenic z = g0, dominance clamp
    'w64': (2, [30, 20, 10], 4, False),     # 64: the table word exactly full
    'w65': (2, [30, 20, 10], 5, False),     # 65, TW 2: a deleterious bit alone in word 1
    'w128': (2, [50, 50, 20], 8, False),    # 128: trait 1 straddles entry 63/64; last register case
    'w129': (2, [50, 50, 20], 9, False),    # 129, TW 3: the memory path; tbw 6 -> gnx_rec_rest
    'five': (5, [4] * 5, 0, False),         # a fifth layer and trait: gnx_rec_rest for e and z only
    'many': (6, [12, 11, 11, 11] * 4, 20, True),    # 16 traits, 200 loci, TW 4
    'delet_only': (1, [], 70, False),       # fitness from tb alone, no clip
    'grow': (2, [30, 80, 10], 9, False),    # the pool test_architecture_grown_in_mid_run draws on
}


def _rasters(n_layers, Wd, Hd):
    gx = np.tile(np.linspace(0, 1, Wd), (Hd, 1))
    gy = np.tile(np.linspace(0, 1, Hd)[:, None], (1, Wd))
    grads = [gx, gy, 1 - gx, 1 - gy, (gx + gy) / 2]
    return np.stack([np.ones((Hd, Wd))] + grads[:n_layers - 1]).astype(np.float32)


def _alpha(n):
    return np.where(np.arange(n) % 2, -1.0, 1.0) / n


def _arch(name, Wd=W, Hd=H):
    n_layers, n_loci, n_delet, dominance = SPECS[name]
    rng = np.random.RandomState(3)
    n_sel = sum(n_loci) + n_delet
    pool = np.concatenate([FORCED, rng.choice(np.setdiff1d(np.arange(L), FORCED), n_sel - 4,
                                              replace=False)]).astype(np.int32)
    traits, at = [], 0
    for t, n in enumerate(n_loci):
        traits.append(dict(loci=pool[at:at + n], alpha=_alpha(n),
                           layer=1 + t % (n_layers - 1) if name != 'five' else [1, 2, 3, 2, 4][t],
                           phi=0.01 if name == 'many' else 0.05, gamma=1.0, univ_adv=False))
        at += n
    if name == 'many':
        traits[3]['phi'] = np.tile(np.linspace(0.005, 0.015, Wd), (Hd, 1)).astype(np.float32)
        traits[5]['univ_adv'] = True
        traits[7]['gamma'] = 2.0
        traits[9]['gamma'] = 0.5
    dom = None
    if dominance:
        dom = np.zeros(L, np.uint8)
        dom[pool[:at][::2]] = 1             # every second trait locus
    assert at + n_delet == n_sel == pool.size == np.unique(pool).size
    return dict(name=name, n_layers=n_layers, rasts=_rasters(n_layers, Wd, Hd), traits=traits,
                dom=dom, delet_loci=pool[at:], delet_s=np.full(n_delet, 0.002))


def _n_sel(arch):
    return sum(t['loci'].size for t in arch['traits']) + arch['delet_loci'].size


def _paths():
    rng = np.random.RandomState(7)
    cross = (rng.rand(64, L) < 2e-3).astype(np.uint8)
    cross[:, 0] = 0
    return O.pack_bits(O.recomb_paths(cross))


def _set_arch(dev, arch):
    for t, tr in enumerate(arch['traits']):
        dev.set_trait(t, tr['loci'], tr['alpha'], tr['layer'], tr['phi'], tr['gamma'],
                      tr['univ_adv'])
    if arch['dom'] is not None:
        dev.set_dominance(arch['dom'])
    dev.set_deleterious(arch['delet_loci'], arch['delet_s'])


def _founders(N, Wd, Hd):
    rng = np.random.RandomState(5)
    x = rng.rand(N) * Wd
    y = rng.rand(N) * Hd
    age = rng.randint(0, 4, N)
    W64 = O.words_per_hom(L)
    g = rng.randint(0, 2 ** 63, (N, 2, W64), dtype=np.int64).astype(np.uint64)
    g ^= rng.randint(0, 2, g.shape).astype(np.uint64) << np.uint64(63)
    g[:, :, L // 64] &= np.uint64((1 << (L % 64)) - 1)
    g[:, :, L // 64 + 1:] = 0
    return x, y, age, g


def _make(arch, paths, cap_inds=4096, defer=True, Wd=W, Hd=H, upload=True, seed=29):
    nat = native()
    dev = nat.Device(Wd, Hd, arch['n_layers'], L=L, n_traits=len(arch['traits']),
                     cap_inds=cap_inds, cap_rows=4096, seed=seed)
    assert dev.W64 == 80
    dev.upload_rasters(arch['rasts'])
    dev.set_species_params(nat.default_species_params(mating_radius=3.0, K_factor=1.0))
    _set_arch(dev, arch)
    dev.set_recomb_paths(paths)
    g = None
    if upload:
        x, y, age, g = _founders(N0, Wd, Hd)
        dev.upload_population(x, y, age, np.zeros(N0), np.arange(N0))
        dev.upload_genomes(g)
        dev.set_z()
    dev.set_defer_crossover(defer)
    return dev, g


def _download(dev, nat):
    return dict(ids=dev.download(nat.F_ID), x=dev.download(nat.F_X), y=dev.download(nat.F_Y),
                e=dev.download(nat.F_E), z=dev.download(nat.F_Z), fit=dev.download(nat.F_FIT),
                geno=dev.download(nat.F_GENO))


def _check(dev, nat, arch, check_fit, tag):
    cols = _download(dev, nat)
    assert cols['ids'].size == dev.N
    try:
        check_columns(cols, arch['rasts'], arch, check_fit)
    except AssertionError as err:
        raise AssertionError('%s, %s: %s' % (arch['name'], tag, err)) from None
    return cols


def _segregating(geno, loci, hom=None):
    """which of `loci` carry both alleles among these genomes (on one homologue, if given)"""
    loci = np.asarray(loci, np.int64)
    bits = (geno[:, :, loci >> 6] >> (loci & 63).astype(np.uint64)) & np.uint64(1)
    if hom is not None:
        bits = bits[:, hom:hom + 1]
    ones = bits.sum(axis=(0, 1))
    return (ones > 0) & (ones < bits.shape[0] * bits.shape[1])


def _assert_not_vacuous(cols, arch, births, n0=N0, born_share=0.95):
    """the conditions under which a checkpoint that passes says something: the living are
    mostly offspring, selection spreads their fitness, the selected loci still segregate, and
    whatever rides behind the fourth layer, trait or table word differs between individuals
    (a lost tail copy would otherwise be invisible)"""
    ids, fit, geno = cols['ids'], cols['fit'], cols['geno']
    name = arch['name']
    print('%s: N %d, born in the run %.3f, births %d, fit %.4f .. %.4f'
          % (name, ids.size, (ids >= n0).mean(), births, fit.min(), fit.max()))
    assert (ids >= n0).mean() >= born_share, (name, (ids >= n0).mean())
    assert births >= 5000, (name, births)
    assert fit.max() - fit.min() >= 0.02, (name, fit.min(), fit.max())
    sel = np.concatenate([t['loci'] for t in arch['traits']] + [arch['delet_loci']])
    seg = _segregating(geno, sel)
    assert seg.sum() * 2 >= sel.size, (name, seg.sum(), sel.size)
    for l in range(4, arch['n_layers']):
        assert np.unique(cols['e'][l]).size > 1, (name, l)
    for t in range(4, len(arch['traits'])):
        assert np.unique(cols['z'][t]).size > 1, (name, t)
    TW = (sel.size + 63) // 64
    if 2 * TW > 4:
        # words 4.. of an individual's 2 * TW table words: homologue 1, entries from here on
        assert TW <= 4
        first = (4 - TW) * 64
        n_tl = sel.size - arch['delet_loci'].size
        tail = _segregating(geno, sel[first:], hom=1)
        assert tail.sum() * 2 >= tail.size, (name, tail.sum(), tail.size)
        assert tail[:n_tl - first].any() and tail[n_tl - first:].any(), name


# ------------------------------------------------------------------ a. gnx_step
STEP_CASES = [(n, True) for n in SPECS if n != 'grow'] + [('small', False), ('many', False)]


@pytest.mark.parametrize('name,defer', STEP_CASES)
def test_step_columns_match_oracle(name, defer):
    """gnx_step, the bench's path, 30 steps: z, e and fit of everybody alive after steps 1, 2,
    10 and 30 (deferred crossover: most of them got z and fit before they had a genome row)"""
    nat = native()
    arch = _arch(name)
    dev, _ = _make(arch, _paths(), defer=defer)
    assert _n_sel(arch) == {'small': 18, 'w64': 64, 'w65': 65, 'w128': 128, 'w129': 129,
                            'five': 20, 'many': 200, 'delet_only': 70}[name]
    births = 0
    for t in range(1, 31):
        dev.step(False, True)
        n, b, _ = dev.counts()
        births += b
        assert n >= 700, (name, t, n)
        if t in (1, 2, 10, 30):
            cols = _check(dev, nat, arch, True, 'step %d' % t)
    _assert_not_vacuous(cols, arch, births)
    dev.close()


# ------------------------------------------------------------------ b. the Model's split step
def _split_step(dev, host, arch, rng=None):
    """one step the way Species._do_pop_dynamics drives it: age, move, mate, [mutation], die.
    Up to 9 of the step's newborns mutate, half of them at selected loci (trait and
    deleterious alike); a slot hit at a trait locus gets set_z_range(slot, 1), as
    Species._do_mutation does.  -> births, mutations that changed a selected allele"""
    dev.age()
    dev.move()
    n0 = dev.N
    dev.pop_dynamics_mate(False)
    B = dev.counts()[1]
    child, par, keys, starts, _ = dev.last_births()
    assert dev.genome_info()['deferred'] == (1 if B else 0)
    host.births(child, par, keys, starts)
    changed = 0
    if rng is not None and B > 0:
        trait_loci = np.concatenate([t['loci'] for t in arch['traits']])
        sel = np.concatenate([trait_loci, arch['delet_loci']])
        n_mut = min(B, 9)
        k = rng.choice(B, n_mut, replace=False)
        n_s = (n_mut + 1) // 2
        loci = np.concatenate([rng.choice(sel, n_s),
                               rng.choice(np.setdiff1d(np.arange(L), sel), n_mut - n_s)])
        loci = loci.astype(np.int32)
        homs = rng.randint(0, 2, n_mut).astype(np.uint8)
        for i, l, hh in zip(child[k[:n_s]], loci[:n_s], homs[:n_s]):
            changed += int(not (int(host.g[int(i)][hh, l >> 6]) >> int(l & 63)) & 1)
        dev.mutate((n0 + k).astype(np.int64), loci, homs)       # joins: every birth is cut now
        host.mutate(child[k], loci, homs)
        for s in sorted(set(int(n0 + kk) for kk, l in zip(k, loci) if l in trait_loci)):
            dev.set_z_range(s, 1)
    dev.pop_dynamics_die(False, True)
    dev.step_index = dev.step_index + 1
    return B, changed


@pytest.mark.parametrize('name', ['small', 'w129', 'many'])
def test_split_step_with_selected_mutations_matches_oracle(name):
    """the split step of the Model API with mutations at selected loci of newborns that are
    still deferred (gnx_mutate -> gnx_l_tb_from_rows on their slots, then set_z_range): the
    mutant's z and fit follow at once and its offspring inherit the bit through tb.  Births
    and mutations are replayed with O.crossover, so the genome the checker reads z from is
    itself anchored."""
    nat = native()
    arch = _arch(name)
    paths = _paths()
    dev, g = _make(arch, paths)
    host = HostGenomes(np.arange(N0), g, paths)
    rng = np.random.RandomState(11)
    births = changed = 0
    for t in range(1, 31):
        B, c = _split_step(dev, host, arch, rng if t % 3 == 0 else None)
        births += B
        changed += c
        assert dev.N >= 700, (name, t, dev.N)
        if t in (3, 4, 12, 30):
            host.check(dev, nat, '%s, step %d' % (name, t))
            cols = _check(dev, nat, arch, True, 'split step %d' % t)
    assert changed >= 10, changed
    _assert_not_vacuous(cols, arch, births)
    dev.close()


# ------------------------------------------------------------------ c, d. gnx_walk
WALK_PIECES = [1, 2, 3, 7, 17]


def _walk(name, cap_inds):
    nat = native()
    arch = _arch(name)
    dev, _ = _make(arch, _paths(), cap_inds=cap_inds)
    births = 0
    for c, T in enumerate(WALK_PIECES):
        dev.walk(T, False, True)
        n0, b, _ = dev.walk_history()
        assert n0.size == T and min(int(n0.min()), dev.N) >= 700, (name, c, n0)
        births += int(b.sum())
        cols = _check(dev, nat, arch, True, 'walk piece %d (%d steps)' % (c, T))
    _assert_not_vacuous(cols, arch, births)
    return dev


@pytest.mark.parametrize('name', ['small', 'w65', 'w129', 'many'])
def test_walk_columns_match_oracle(name):
    """gnx_walk at a small capacity - the device-driven step, one graph launch per step - in
    pieces of 1, 2, 3, 7 and 17 steps"""
    dev = _walk(name, 4096)
    assert dev.totals()['dd_steps'] > 0 and dev.path_counts()['lazy_mortalities'] == 0
    dev.close()


@pytest.mark.parametrize('name', ['small', 'w129', 'many'])
def test_large_capacity_walk_columns_match_oracle(name):
    """gnx_walk on a handle with 2^20 slots, what bench.py times: the dead stay in their slots
    between the steps of a piece and the next cell sort gathers the living - the gather must
    bring every layer, trait and table word along"""
    dev = _walk(name, 1 << 20)
    pc = dev.path_counts()
    assert pc['lazy_mortalities'] == sum(T - 1 for T in WALK_PIECES), pc
    dev.close()


# ------------------------------------------------------------------ e. the table grows
def test_architecture_grown_in_mid_run():
    """gnx_l_rebuild_sel in mid-run, as Species._upload_gen_arch does after a non-neutral
    mutation: 64 selected loci -> 65 (TW 1 -> 2: tb is reallocated and rebuilt from the rows)
    -> 129 (TW 3, the memory path).  The added loci already segregate."""
    nat = native()
    pool = _arch('grow')
    T0, T1, T2 = (t['loci'] for t in pool['traits'])
    D = pool['delet_loci']

    def stage(n1, nd):
        a = dict(pool, delet_loci=D[:nd], delet_s=np.full(nd, 0.002))
        a['traits'] = [dict(pool['traits'][0]), dict(pool['traits'][1], loci=T1[:n1],
                                                     alpha=_alpha(n1)),
                       dict(pool['traits'][2])]
        return a

    arch = stage(20, 4)
    assert _n_sel(arch) == 64
    dev, _ = _make(arch, _paths())
    births = 0
    for n1, nd, n_sel in [(20, 4, 64), (20, 5, 65), (80, 9, 129)]:
        if n_sel > 64:
            arch = stage(n1, nd)
            assert _n_sel(arch) == n_sel
            tr = arch['traits'][1]
            if n1 > 20:
                dev.set_trait(1, tr['loci'], tr['alpha'], tr['layer'], tr['phi'], tr['gamma'],
                              tr['univ_adv'])
            dev.set_deleterious(arch['delet_loci'], arch['delet_s'])
            dev.set_z()
            _check(dev, nat, arch, False, 'grown to %d, before the next step' % n_sel)
        for t in range(10):
            dev.step(False, True)
            n, b, _ = dev.counts()
            births += b
            assert n >= 700, (n_sel, t, n)
        cols = _check(dev, nat, arch, True, '10 steps at %d selected loci' % n_sel)
    _assert_not_vacuous(cols, arch, births)
    dev.close()


# ------------------------------------------------------------------ f. two tiles
@pytest.mark.parametrize('name', ['w129', 'many'])
def test_two_tiles_columns_match_oracle(name):
    """two tiles (threads of this process) through the library's own step protocol: migrants
    carry z[n][n_traits] and get tb rebuilt from their rows on import, offspring of ghost
    mates get tb and z a second time from their finished row.  Each tile checks its own
    individuals after steps 1, 5 and 20."""
    import torch
    from _local_comm import Hub, LocalComm
    from geonomics_amd.parallel import DeviceShard, TiledStepper
    nat = native()
    Wt, Ht, N = 80, 40, 3000
    arch = _arch(name, Wt, Ht)
    paths = _paths()
    x, y, age, g = _founders(N, Wt, Ht)
    lock = threading.Lock()
    hub = Hub(2, library_group=True)
    errs, last, births = [], [None, None], [0]

    def body(rank):
        try:
            torch.cuda.set_device(0)
            comm = LocalComm(hub, rank)
            dev, _ = _make(arch, paths, Wd=Wt, Hd=Ht, upload=False)
            shard = DeviceShard(dev)
            stepper = TiledStepper(shard, comm, Wt, Ht, 3.0, move=True, max_id=N - 1,
                                   fixed_births=1, use_library=True)
            assert stepper.v3
            mine = stepper.rank_of(x, y) == rank
            dev.upload_population(x[mine], y[mine], age[mine], np.zeros(mine.sum()),
                                  np.arange(N)[mine])
            dev.upload_genomes(g[mine])
            dev.set_z()
            dev.set_defer_crossover(True)
            shard.has_genomes = True

            def after(first_id, total):
                if rank == 0:
                    births[0] += total

            for t in range(1, 21):
                n, _, _ = stepper.step(False, True, after_births=after)
                assert n >= 700, (name, t, n)
                if t in (1, 5, 20):
                    with lock:
                        last[rank] = _check(dev, nat, arch, True,
                                            'tile %d, step %d' % (rank, t))
                    hub.barrier.wait()
            dev.close()
        except BaseException as e:       # noqa: BLE001 - re-raised in the main thread
            errs.append(e)
            hub.abort()

    ths = [threading.Thread(target=body, args=(r,)) for r in range(2)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    if errs:
        raise errs[0]
    assert min(c['ids'].size for c in last) > 350
    both = {k: np.concatenate([c[k] for c in last], axis=1 if k in ('e', 'z') else 0)
            for k in last[0]}
    assert np.unique(both['ids']).size == both['ids'].size
    # (20 steps, not 30: 0.8 ** 20 of the founders are left, ~1 %)
    _assert_not_vacuous(both, arch, births[0], n0=N, born_share=0.85)
