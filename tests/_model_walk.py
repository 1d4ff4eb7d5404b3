"""Shared by tests/test_gpu_model_walk.py: one runner that builds a small model, burns it in,
applies a script of Model.walk calls and host interventions and returns everything the two routes
of a main step - Species._walk_on_device and the Model's function queue - must agree on, and a
recorder that proves which route every step took."""
import numpy as np


def params(**kw):
    from test_gpu_model_api import small_params
    return small_params(**kw)


class Route:
    """what the script's steps went through: the lengths of the gnx_walk calls (and the
    population each started from), and the main steps of the function queue (its
    _do_pop_dynamics makes one successful pop_dynamics_mate call per step and Species)"""

    def __init__(self, monkeypatch):
        from geonomics_amd import _native as nat
        self.pieces, self.piece_n, self.queue = [], [], 0
        self.events = []            # 'walk' / 'queue', in the order they happened
        self.on = False
        walk, mate = nat.Device.walk, nat.Device.pop_dynamics_mate
        rec = self

        def rec_walk(dev, T, burn, with_selection):
            if rec.on:
                rec.pieces.append(int(T))
                rec.piece_n.append(int(dev.N))
                rec.events.append('walk')
            return walk(dev, T, burn, with_selection)

        def rec_mate(dev, burn):
            out = mate(dev, burn)          # (a call that did not fit raises and is repeated)
            if rec.on and not burn:
                rec.queue += 1
                rec.events.append('queue')
            return out

        monkeypatch.setattr(nat.Device, 'walk', rec_walk)
        monkeypatch.setattr(nat.Device, 'pop_dynamics_mate', rec_mate)

    def take(self):
        """(pieces, queue steps) since the last take()"""
        out = (list(self.pieces), self.queue)
        del self.pieces[:]
        self.queue = 0
        return out


def state_of(mod, spp_num=0):
    from geonomics_amd import _native as nat
    spp = mod.comm[spp_num]
    d = spp._dev
    ids = d.download(nat.F_ID)
    o = np.argsort(ids, kind='stable')
    s = dict(Nt=list(spp.Nt), n_births=list(spp.n_births), n_deaths=list(spp.n_deaths),
             t=(mod.t, mod.comm.t, spp.t), max_ind_idx=spp.max_ind_idx, extinct=spp.extinct,
             step_index=int(d.step_index), n=len(spp),
             ids=ids[o], x=d.download(nat.F_X)[o], y=d.download(nat.F_Y)[o],
             age=d.download(nat.F_AGE)[o], sex=d.download(nat.F_SEX)[o],
             e=d.download(nat.F_E)[:, o], z=d.download(nat.F_Z)[:, o],
             fit=d.download(nat.F_FIT)[o], N=spp.N)
    assert s['n'] == ids.size
    if ids.size and spp.gen_arch is not None:
        s['g'] = spp._get_genotypes()
        assert s['g'].shape[0] == ids.size
    return s


def walk(k):
    def op(mod):
        mod.walk(k, 'main', verbose=False)
    return op


def run_script(monkeypatch, route, p, script, model_walk, cap_factor=None):
    """make_model(p), burn-in, the script's operations in turn; -> the end state with
    'route': [(pieces, queue steps) of every operation], 'cap': the slots at the end,
    'cap0': after the burn-in, 'nburn': steps of the burn-in.  model_walk False: GNX_MODEL_WALK=0."""
    import geonomics_amd as gnx
    if model_walk:
        monkeypatch.delenv('GNX_MODEL_WALK', raising=False)
    else:
        monkeypatch.setenv('GNX_MODEL_WALK', '0')
    if cap_factor is None:
        monkeypatch.delenv('GNX_CAP_FACTOR', raising=False)
    else:
        monkeypatch.setenv('GNX_CAP_FACTOR', str(cap_factor))
    monkeypatch.delenv('GNX_CONCURRENT_ITS', raising=False)
    mod = gnx.make_model(p)
    spp = mod.comm[0]
    mod.walk(10000, 'burn', verbose=False)
    assert mod.comm.burned
    nburn, cap0 = len(spp.Nt), spp._cap
    routes = []
    route.take()
    route.on = True
    try:
        for op in script:
            op(mod)
            routes.append(route.take())
    finally:
        route.on = False
    s = state_of(mod)
    s.update(route=routes, cap=spp._cap, cap0=cap0, nburn=nburn, path_counts=spp._dev.path_counts())
    for sp in mod.comm.values():
        sp._dev.close()
    return s


BOOKKEEPING = ('Nt', 'n_births', 'n_deaths', 't', 'max_ind_idx', 'extinct', 'step_index', 'n')
COLUMNS = ('ids', 'x', 'y', 'age', 'sex', 'e', 'z', 'fit', 'g', 'N')


def assert_same_state(a, b, what='', skip=()):
    for k in BOOKKEEPING:
        assert a[k] == b[k], '%s %s: %r != %r' % (what, k, a[k], b[k])
    assert ('g' in a) == ('g' in b), what
    for k in COLUMNS:
        if k in a and k not in skip:
            np.testing.assert_array_equal(a[k], b[k], err_msg='%s %s' % (what, k))


def assert_lively(s, n_main):
    """the reference run says something: more than 200 individuals and births in every one of
    its n_main main steps"""
    assert len(s['Nt']) == s['nburn'] + n_main
    assert min(s['Nt'][s['nburn']:]) > 200, s['Nt'][s['nburn']:]
    assert min(s['n_births'][s['nburn']:]) > 0, s['n_births'][s['nburn']:]


def parent_piece(steps_left, n, cap, R=0.5):
    """the piece length of the version before _walk_piece (kept here as a number to pin)"""
    return int(max(1, min(steps_left, 256, 0.5 * max(cap - n, 1) / (max(0.02, R * 0.25) * max(n, 1)))))
