"""Model.walk / Model.run through Species._walk_on_device against the Model's function queue.

walk(T >= 2, verbose=False) and every run() iteration of a model with one moving species, no
mutation, no pedigree, no change events and no collectors hand their main steps to
Species._walk_on_device: one gnx_walk call per piece, the per-step counts read back afterwards.
GNX_MODEL_WALK=0 forces the function queue, one step per turn, which the oracle tests pin.  Every
draw is keyed by (seed, id, step, op) and no arithmetic differs between the routes, so every
comparison here is bit for bit: Nt, n_births, n_deaths (burn-in included), t of the Model, the
Community and the Species, max_ind_idx, extinct, the device's step index, every column and the
genotypes by ascending id, and the density raster.  A recorder around Device.walk and
Device.pop_dynamics_mate proves which route every step took.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _model_walk as W          # noqa: E402

pytestmark = pytest.mark.gpu

CAP_TIGHT = '1.05'               # int(1.05 * 450) + 1024 = 1496 slots
CAP_ROOMY = '20'                 # 10 024 slots: no run here comes near them


@pytest.fixture
def route(monkeypatch):
    return W.Route(monkeypatch)


def _both(monkeypatch, route, make_p, script, cap_factor=None, ref_cap_factor=None):
    """(the function queue's run, the run under test) of one script"""
    ref = W.run_script(monkeypatch, route, make_p(), script, False, ref_cap_factor)
    got = W.run_script(monkeypatch, route, make_p(), script, True, cap_factor)
    assert all(pieces == [] for pieces, _ in ref['route']), ref['route']
    assert ref['cap'] == ref['cap0']                  # (and never had to grow)
    # the births of every step ever taken, and nothing else, moved max_ind_idx
    for s in (ref, got):
        assert s['max_ind_idx'] == 300 - 1 + sum(s['n_births'])
    return ref, got


@pytest.mark.parametrize('variant', ['traits', 'sexed', 'neutral'])
def test_plain_walk(variant, monkeypatch, route):
    """walk(12): one piece of 12 and no queue step"""
    kw = dict(traits=dict(seed=3), sexed=dict(seed=4, sex=True),
              neutral=dict(seed=5, traits=False))[variant]

    def make_p():
        p = W.params(**kw)
        if variant == 'sexed':          # (half the pairs of an unsexed species: twice the room)
            p['comm']['species']['spp_0']['init']['K_factor'] = 1.0
        return p
    ref, got = _both(monkeypatch, route, make_p, [W.walk(12)])
    W.assert_lively(ref, 12)
    assert ref['route'] == [([], 12)] and got['route'] == [([12], 0)]
    assert got['t'] == (11, 11, 11) and got['step_index'] == got['nburn'] + 12
    assert got['z'].shape[0] == (0 if variant == 'neutral' else 2)
    if variant == 'sexed':
        assert set(got['sex'].tolist()) == {0, 1}
    W.assert_same_state(ref, got, variant)


def test_walk_in_pieces(monkeypatch, route):
    """1496 slots for ~320 individuals: walk(40) goes in pieces, all of them on the device, each
    as long as the version before _walk_piece made it - half the free slots at R / 4 a step"""
    ref, got = _both(monkeypatch, route, lambda: W.params(seed=3), [W.walk(40)],
                     cap_factor=CAP_TIGHT, ref_cap_factor=CAP_ROOMY)
    W.assert_lively(ref, 40)
    assert got['cap'] == got['cap0'] == 1496
    (pieces, queue), = got['route']
    print('pieces of walk(40) in 1496 slots:', pieces, 'from N =', route.piece_n)
    assert queue == 0 and sum(pieces) == 40 and len(pieces) >= 3 and min(pieces) >= 2
    left = 40
    for k, n in zip(pieces, route.piece_n):
        assert k == W.parent_piece(left, n, 1496), (pieces, route.piece_n)
        left -= k
    W.assert_same_state(ref, got)


def test_large_capacity_walk(monkeypatch, route):
    """more than gnx_dd_max_cap() = 600 000 slots: gnx_walk drives the steps from the host, every
    one but a piece's last leaves its dead in their slots and launches the next movement - and the
    model ends where the default capacity's function queue takes it.  walk(1) takes the queue."""
    script = [W.walk(5), W.walk(1), W.walk(3)]
    ref, got = _both(monkeypatch, route, lambda: W.params(seed=3), script, cap_factor='1400')
    W.assert_lively(ref, 9)
    assert got['cap'] == 1400 * 450 + 1024 > 600_000 and ref['cap'] == 2149
    assert got['route'] == [([5], 0), ([], 1), ([3], 0)]
    pc = got['path_counts']
    assert pc['lazy_mortalities'] > 0 and pc['moves_ahead'] > 0, pc
    assert ref['path_counts']['lazy_mortalities'] == 0
    W.assert_same_state(ref, got)


def _remove_by_rank(mod):
    ids = np.array([*mod.comm[0]])
    mod.remove_individuals(individs=ids[[0, 3, 10, 50, 51, 120, 199, len(ids) - 1]])


def _move_by_rank(mod):
    """the reference's scripts move individuals like this (tests/validation/wf/wf_test.py:69-76)"""
    spp = mod.comm[0]
    ids = np.array([*spp])[[1, 7, 77, 150, -2]]
    for k, ind in enumerate(spp._get_individs(ids).values()):
        ind.x = 2.5 + 5 * k
        ind.y = 29.25 - 3 * k
    spp._set_coords_and_cells()


def _set_b(mod):
    mod.comm[0].b = 0.4


def test_interventions_between_walks(monkeypatch, route):
    """individuals removed and moved by a script and a parameter assigned between device walks:
    the device walk picks the population and the parameters up as the queue does"""
    script = [W.walk(5), _remove_by_rank, _move_by_rank, W.walk(4), _set_b, W.walk(3)]
    ref, got = _both(monkeypatch, route, lambda: W.params(seed=7), script)
    W.assert_lively(ref, 12)
    assert got['route'] == [([5], 0), ([], 0), ([], 0), ([4], 0), ([], 0), ([3], 0)]
    assert ref['route'] == [([], 5), ([], 0), ([], 0), ([], 4), ([], 0), ([], 3)]
    # (b = 0.4 took hold: twice the births of the steps before it)
    assert np.mean(got['n_births'][-3:]) > 1.5 * np.mean(got['n_births'][-12:-3])
    W.assert_same_state(ref, got)


def _growth_params():
    p = W.params(seed=3)
    p['comm']['species']['spp_0']['mating']['n_births_distr_lambda'] = 3
    return p


def _K_times_4(mod):
    spp = mod.comm[0]
    spp.K = spp.K * 4


def test_growth_through_the_gate(monkeypatch, route):
    """three offspring per pair and a carrying capacity quadrupled by a script, in 1496 slots: the
    population outgrows the device state inside walk(30).  The device walk's pieces stop short of
    what their births could fill, the function queue takes over and moves the population to a
    larger state, and the next walk is the device's again - all of it the run that 10 024 slots
    and the queue alone give."""
    script = [_K_times_4, W.walk(30), W.walk(6)]
    ref, got = _both(monkeypatch, route, _growth_params, script, cap_factor=CAP_TIGHT,
                     ref_cap_factor=CAP_ROOMY)
    W.assert_lively(ref, 36)
    assert got['cap0'] == 1496 and ref['cap'] == 10024
    (_, _), (pieces, queue), (last_pieces, last_queue) = got['route']
    print('growth: pieces of walk(30)', pieces, 'from N =', route.piece_n[:len(pieces)],
          'then', queue, 'queue steps; slots', got['cap0'], '->', got['cap'],
          '; walk(6):', last_pieces, last_queue, '; N', ref['Nt'][ref['nburn']:])
    assert len(pieces) >= 1 and queue >= 1 and sum(pieces) + queue == 30
    # in this order: device pieces, the queue for the rest of walk(30), the device for walk(6)
    # (the events of the run under test follow the 36 queue steps of the reference run)
    assert route.events == (['queue'] * 36 + ['walk'] * len(pieces) + ['queue'] * queue +
                            ['walk'] * len(last_pieces))
    assert max(ref['Nt']) > 1496 and got['cap'] > 1496          # it had to grow, and did
    assert got['n'] < 0.66 * got['cap']
    assert sum(last_pieces) == 6 and last_queue == 0
    W.assert_same_state(ref, got)


def _deadly(mod):
    mod.comm[0].d_min = 0.9


def test_extinction_inside_a_device_walk(monkeypatch, route):
    """death probabilities of 0.9 and more from the first main step on: an ordinary run to N = 0
    inside a device walk.  The step that kills the last ones counts, with its births and deaths,
    and appends no Nt; the walk after it does nothing - on either route."""
    seen = {}

    def look(mod):
        seen.setdefault(os.environ.get('GNX_MODEL_WALK', '1'), []).append(W.state_of(mod))

    script = [_deadly, W.walk(10), look, W.walk(3), look]
    ref, got = _both(monkeypatch, route, lambda: W.params(seed=3), script)
    assert got['route'][1][1] == 0 and sum(got['route'][1][0]) >= 2       # all on the device
    assert got['route'][3] == ([], 0) and ref['route'][3] == ([], 0)
    for s, (first, second) in ((ref, seen['0']), (got, seen['1'])):
        W.assert_same_state(first, second)
        W.assert_same_state(second, s)
        steps = len(s['n_births']) - s['nburn']
        assert 2 <= steps < 10 and len(s['Nt']) - s['nburn'] == steps - 1
        assert len(s['n_deaths']) == len(s['n_births'])
        assert s['Nt'][-1] + s['n_births'][-1] - s['n_deaths'][-1] == 0 and s['Nt'][-1] > 0
        assert s['extinct'] is True and s['n'] == 0 and s['ids'].size == 0
        assert s['t'] == (steps - 1,) * 3 and s['step_index'] == s['nburn'] + steps
    # (not Species.N: the queue leaves the density of the step that killed the last ones, taken
    # before its deaths; the library steps the empty population to the end of the piece, and
    # the raster an extinct Species is left with there is the empty one's: zeros)
    W.assert_same_state(ref, got, skip=('N',))


def test_model_run_iterations(monkeypatch, route):
    """Model.run(): three iterations of eight steps, each restored from the burned-in snapshot;
    iteration_log and the state at the end of every iteration"""
    import geonomics_amd as gnx

    def run(model_walk):
        if model_walk:
            monkeypatch.delenv('GNX_MODEL_WALK', raising=False)
        else:
            monkeypatch.setenv('GNX_MODEL_WALK', '0')
        monkeypatch.delenv('GNX_CONCURRENT_ITS', raising=False)
        mod = gnx.make_model(W.params(seed=9, n_its=3, T=8))
        ends = {}
        mod._on_iteration_end = lambda m: ends.__setitem__(m.it, W.state_of(m))
        route.take()
        route.on = True
        try:
            mod.run(verbose=False)
        finally:
            route.on = False
        for spp in mod.comm.values():
            spp._dev.close()
        return mod.iteration_log, ends, route.take()

    log0, ends0, route0 = run(False)
    log1, ends1, route1 = run(True)
    assert route0 == ([], 24) and route1 == ([8, 8, 8], 0)
    assert sorted(log0) == sorted(ends0) == sorted(ends1) == [0, 1, 2]
    assert log0 == log1
    for it in range(3):
        s = ends0[it]
        assert s['t'] == (7, 7, 7) and min(s['Nt'][-8:]) > 200 and min(s['n_births'][-8:]) > 0
        assert log0[it]['spp_0']['Nt'] == s['Nt']
        W.assert_same_state(s, ends1[it], 'iteration %d' % it)


def test_restored_iteration_numbers_offspring_from_max_ind_idx(monkeypatch):
    """the snapshot every later iteration starts from may have lost its newest individuals: the
    restored device still numbers offspring from max_ind_idx + 1, so the host's count and the ids
    on the device stay one sequence (a device grown later is told max_ind_idx, and
    add_individuals starts from it)"""
    import geonomics_amd as gnx
    monkeypatch.setenv('GNX_MODEL_WALK', '0')        # (the queue keeps the last step's births)
    monkeypatch.delenv('GNX_CONCURRENT_ITS', raising=False)
    from geonomics_amd import _native as nat
    mate, newest_born = nat.Device.pop_dynamics_mate, []

    def rec_mate(dev, burn):
        out = mate(dev, burn)
        child = dev.last_births(with_gametes=False)[0]       # (readable until the deaths)
        newest_born[:] = [int(child.max()) if child.size else None, int(child.size)]
        return out
    monkeypatch.setattr(nat.Device, 'pop_dynamics_mate', rec_mate)
    mod = gnx.make_model(W.params(seed=9, n_its=3, T=3))
    snapshot, seen = mod._snapshot_comm, {}

    def without_the_newest():
        ids = np.array([*mod.comm[0]])
        mod.remove_individuals(individs=ids[-2:])
        assert mod.comm[0].max_ind_idx >= ids[-1]
        return snapshot()

    def at_end(m):
        spp = m.comm[0]
        seen[m.it] = (newest_born[0], newest_born[1], spp.max_ind_idx, spp.n_births[-1])
    mod._snapshot_comm = without_the_newest
    mod._on_iteration_end = at_end
    mod.run(verbose=False)
    assert sorted(seen) == [0, 1, 2]
    for it, (newest, n_children, max_ind_idx, births) in seen.items():
        assert n_children == births > 0
        assert newest == max_ind_idx, (it, seen)
    for spp in mod.comm.values():
        spp._dev.close()


def _two_species_params():
    import geonomics_amd as gnx
    from geonomics_amd.sim import params as P
    d = P.default_params_dict(layers=[{'type': 'defined'}, {'type': 'defined'}],
                              species=[{'genomes': True}, {'genomes': True}])
    d['landscape']['main']['dim'] = (24, 24)
    for k in ('lyr_0', 'lyr_1'):
        d['landscape']['layers'][k]['init']['defined']['rast'] = np.ones((24, 24))
    for k in ('spp_0', 'spp_1'):
        s = d['comm']['species'][k]
        s['init'].update({'N': 200, 'K_factor': 0.5})
        s['mating'].update({'mating_radius': 4})
        s['gen_arch'].update({'L': 16, 'n_recomb_sims': 50, 'use_tskit': False})
    d['model'].update({'T': 4, 'burn_T': 30, 'seed': {'num': 2}})
    return gnx.make_params_dict(d, 'two_spp')


QUEUE_ONLY = ['verbose', 'T1', 'mutation', 'pedigree', 'stats', 'data', 'land_change',
              'spp_change', 'no_movement', 'two_species']


@pytest.mark.parametrize('case', QUEUE_ONLY)
def test_routes_that_stay_on_the_queue(case, monkeypatch, route, tmp_path, capsys):
    """whatever needs the host between two steps keeps the device walk off: Device.walk is never
    called, every step is the queue's, and the model's clock advanced by T"""
    import geonomics_amd as gnx
    from geonomics_amd.sim.params import ParametersDict
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('GNX_MODEL_WALK', raising=False)
    T, verbose, n_spp = 3, False, 1
    p = W.params(seed=3, L=32, T=T)
    s = p['comm']['species']['spp_0']
    none = dict(rate=None, interval=None, distr=None, n_cycles=None, size_range=None,
                start_t=None, end_t=None)
    if case == 'verbose':
        verbose = True
    elif case == 'T1':
        T = 1
    elif case == 'mutation':
        s['gen_arch'].update({'mu_neut': 1e-3, 'mu_delet': 0})
    elif case == 'pedigree':
        s['gen_arch']['use_tskit'] = True
    elif case == 'stats':
        p['model']['stats'] = ParametersDict({'Nt': {'calc': True, 'freq': 1},
                                              'het': {'calc': True, 'freq': 2, 'mean': False}})
    elif case == 'data':
        p['model']['data'] = ParametersDict({
            'sampling': {'scheme': 'random', 'n': 10, 'points': None, 'transect_endpoints': None,
                         'n_transect_points': None, 'radius': None, 'when': 2,
                         'include_landscape': False, 'include_fixed_sites': False},
            'format': {'gen_format': 'vcf', 'geo_vect_format': 'csv', 'geo_rast_format': 'txt',
                       'nonneut_loc_format': None}})
    elif case == 'land_change':
        p['landscape']['layers']['lyr_0']['change'] = ParametersDict(
            {0: {'change_rast': np.full((30, 30), 0.9), 'start_t': 0, 'end_t': 2, 'n_steps': 2}})
    elif case == 'spp_change':
        s['change'] = ParametersDict(
            {'dem': {0: dict(none, kind='custom', timesteps=[1], sizes=[0.9])}})
    elif case == 'no_movement':
        s['movement']['move'] = False
    elif case == 'two_species':
        p, n_spp = _two_species_params(), 2
    mod = gnx.make_model(p)
    mod.walk(10000, 'burn', verbose=False)
    assert mod.comm.burned and len(mod.comm) == n_spp
    route.on = True
    try:
        mod.walk(T, 'main', verbose=verbose)
    finally:
        route.on = False
    assert route.take() == ([], T * n_spp)
    assert mod.t == mod.comm.t == T - 1
    for spp in mod.comm.values():
        assert spp.t == T - 1 and len(spp) > 0 and not spp.extinct
        assert int(spp._dev.step_index) == len(spp.Nt)
        spp._dev.close()
    capsys.readouterr()
