"""What the change-event tests share (tests/test_changes_host.py on the oracle,
tests/test_gpu_changes.py on the device): one small experiment - 24 x 24 cells, 500 founders,
L = 128, traits on layer 1 (and 2), mating radius 3 - the ways to take a step, the column
download, and the conditions under which a passing check says something.

A change event rewrites what the kernels read between two steps: a raster, K, or the whole
species parameter block.  The reference applies every change after the step's hot path
(sim/model.py:644-656); the habitat values of everybody are sampled again at the end of the
next mating (structs/species.py:804), so between the change and that step e is what the last
mating sampled."""
import numpy as np

import gnx_oracle as O
import gnx_step as S
from _columns import fitness_ref, ulp32

W = H = 24
N0 = 500
L = 128
SEED = 31
CAP = 4096
BIG_CAP = 1 << 20           # above the device-driven walk's capacity limit: gnx_walk loops gnx_step
F = np.float32


def rasters(n_layers=2):
    gx = np.tile(np.linspace(0, 1, W), (H, 1))
    gy = np.tile(np.linspace(0, 1, H)[:, None], (1, W))
    return np.stack([np.ones((H, W)), gx, gy][:n_layers]).astype(F)


def with_layer(rasts, layer, new):
    out = np.array(rasts, F)
    out[layer] = new
    return out


def reversed_layer(rasts, layer):
    """the rasters with the gradient of one layer reversed"""
    return with_layer(rasts, layer, rasts[layer][::-1, ::-1])


def make_arch(layers=(1,), phi=0.5):
    """one trait per entry of `layers`, 8 loci each (locus 63 and 64: both sides of a word)"""
    pool = np.array([3, 63, 64, 127, 17, 40, 90, 101, 5, 22, 70, 111, 9, 33, 77, 120], np.int32)
    traits = [dict(loci=pool[8 * t:8 * t + 8], alpha=np.where(np.arange(8) % 2, -1.0, 1.0) / 8,
                   layer=int(l), phi=phi, gamma=1.0, univ_adv=False)
              for t, l in enumerate(layers)]
    return dict(traits=traits, dom=None, delet_loci=np.zeros(0, np.int32), delet_s=np.zeros(0))


def founders(sexed=False):
    # (of the seeds 1 .. 8 the one that leaves most of the founders' generation alive four steps
    # after a change, in the oracle: 106 where the species moves, 133 where it does not)
    rng = np.random.RandomState(6)
    x = rng.rand(N0) * W
    y = rng.rand(N0) * H
    age = rng.randint(0, 4, N0)
    geno = O.pack_genomes((rng.rand(N0, L, 2) < 0.5).astype(np.uint8))
    sex = rng.randint(0, 2, N0) if sexed else np.zeros(N0, np.int64)
    return x, y, age, sex, geno


def paths():
    rng = np.random.RandomState(7)
    cross = (rng.rand(64, L) < 0.02).astype(np.uint8)
    cross[:, 0] = 0
    return O.pack_bits(O.recomb_paths(cross))


# ---------------------------------------------------------------- the oracle's run
def oracle_state(rasts, arch, **params):
    p = dict(mating_radius=3.0, K_factor=1.0)
    p.update(params)
    st = S.State(rasts, S.Params(**p), SEED, L=L, traits=arch['traits'], paths_packed=paths())
    x, y, age, sex, geno = founders(sexed=bool(p.get('sexed', False)))
    st.set_population(x, y, age, sex, np.arange(N0))
    st.set_genomes(geno)
    return st


def oracle_cols(st):
    return dict(ids=st.id.copy(), x=st.x.copy(), y=st.y.copy(), e=st.e.T.copy(), z=st.z.T.copy(),
                fit=st.fit.copy(), geno=st.geno.copy())


# ---------------------------------------------------------------- non-vacuity
def survivors(cols, before_ids):
    return np.isin(cols['ids'], before_ids)


def sharp_count(cols, who, old_rasts, arch):
    """among `who`: how many have a fitness under the old rasters' habitat values that differs
    from the one under their e column by more than the checker's tolerance - the individuals on
    whom a stale e would be caught through fit as well"""
    cx, cy = cols['x'].astype(np.int64), cols['y'].astype(np.int64)
    e_old = np.asarray(old_rasts, F)[:, cy, cx]
    w_new = fitness_ref(cols['e'], cols['z'], cx, cy, cols['geno'], arch)
    w_old = fitness_ref(e_old, cols['z'], cx, cy, cols['geno'], arch)
    return int((who & (np.abs(w_new - w_old) > ulp32(w_new))).sum())


def assert_sharp(cols, before_ids, old_rasts, arch, tag):
    """the conditions of a check after a layer change: at least 100 individuals from before
    the change are alive, and for at least 50 of them the old habitat values would give another
    fitness"""
    who = survivors(cols, before_ids)
    n_sharp = sharp_count(cols, who, old_rasts, arch)
    print('%s: N %d, from before the change %d, of them sharp %d'
          % (tag, cols['ids'].size, who.sum(), n_sharp))
    assert who.sum() >= 100, (tag, int(who.sum()))
    assert n_sharp >= 50, (tag, n_sharp)
    return int(who.sum())


# ---------------------------------------------------------------- the device
def native():
    from geonomics_amd import _native
    return _native


def make_handle(rasts, arch, cap=CAP, seed=SEED, population=None, **sp_kw):
    """a handle with the experiment's founders (or `population`: dict(x, y, age, sex, ids,
    geno) in slot order) - test_gpu_parity.make_dev at the small capacity; at BIG_CAP the
    same with 4096 genome rows, as test_large_capacity_walk_columns_match_oracle sets it up"""
    from test_gpu_parity import make_dev, upload_simple
    nat = native()
    sp = dict(mating_radius=3.0, K_factor=1.0)
    sp.update(sp_kw)
    n_traits = len(arch['traits'])
    if cap == CAP:
        dev = make_dev(W, H, rasts=rasts, L=L, n_traits=n_traits, cap=cap, seed=seed, **sp)
    else:
        dev = nat.Device(W, H, len(rasts), L=L, n_traits=n_traits, cap_inds=cap, cap_rows=4096,
                         seed=seed)
        dev.upload_rasters(np.asarray(rasts, F))
        dev.set_species_params(nat.default_species_params(**sp))
    for t, tr in enumerate(arch['traits']):
        dev.set_trait(t, tr['loci'], tr['alpha'], tr['layer'], tr['phi'], tr['gamma'],
                      tr['univ_adv'])
    dev.set_recomb_paths(paths())
    if population is None:
        x, y, age, sex, geno = founders(sexed=bool(sp.get('sexed', 0)))
        population = dict(x=x, y=y, age=age, sex=sex, ids=np.arange(N0), geno=geno)
    q = population
    upload_simple(dev, q['x'], q['y'], ids=q['ids'], age=q['age'], sex=q['sex'])
    dev.upload_genomes(q['geno'])
    dev.set_z()
    return dev


def download(dev):
    nat = native()
    cols = dict(ids=dev.download(nat.F_ID), x=dev.download(nat.F_X), y=dev.download(nat.F_Y),
                age=dev.download(nat.F_AGE), sex=dev.download(nat.F_SEX),
                e=dev.download(nat.F_E), z=dev.download(nat.F_Z), fit=dev.download(nat.F_FIT),
                geno=dev.download(nat.F_GENO))
    assert cols['ids'].size == dev.N
    return cols


STEP_PATHS = ['step', 'queue', 'split']


def take_step(dev, path):
    """one time step: gnx_step, or the Model's function queue - age, movement where the
    species moves, pop dynamics whole or in its two halves"""
    if path == 'step':
        dev.step(False, True)
        return
    dev.age()
    if dev.sp.move:
        dev.move()
    if path == 'queue':
        dev.pop_dynamics(False, True)
    else:
        assert path == 'split', path
        dev.pop_dynamics_mate(False)
        dev.pop_dynamics_die(False, True)
    dev.step_index = dev.step_index + 1


def births_of(dev, walked=False):
    """births of the last step, or of all steps of the last walk"""
    return int(dev.walk_history()[1].sum()) if walked else int(dev.counts()[1])


def twin_of(dev, max_id, rasts, arch, cap=CAP, **sp_kw):
    """a fresh handle that starts where `dev` stands: the same seed, `dev`'s population in its
    slot order with its genomes (z from set_z), its step index and the largest id it has given
    out (the founders' plus its births so far) - and the rasters and parameters given here from
    the start.  Whatever `dev` still derives from rasters or parameters it held before is what
    the two will differ in."""
    c = download(dev)
    twin = make_handle(rasts, arch, cap=cap,
                       population=dict(x=c['x'], y=c['y'], age=c['age'], sex=c['sex'],
                                       ids=c['ids'], geno=c['geno']), **sp_kw)
    twin.step_index = dev.step_index
    twin.set_max_id(max_id)
    return twin


def by_id(cols):
    o = np.argsort(cols['ids'], kind='stable')
    return {k: (v[:, o] if k in ('e', 'z') else v[o]) for k, v in cols.items()}


def assert_same_population(a, b, tag):
    """two handles hold the same individuals, bit for bit: counts, and by ascending id x, y,
    age, sex, e, z, fit and genotypes.  The message names the first column that differs."""
    ca, cb = by_id(download(a)), by_id(download(b))
    assert ca['ids'].size == cb['ids'].size, '%s: N %d against %d' % (tag, ca['ids'].size,
                                                                     cb['ids'].size)
    for k in ('ids', 'x', 'y', 'age', 'sex', 'e', 'z', 'fit', 'geno'):
        va, vb = ca[k], cb[k]
        same = va.shape == vb.shape and \
            np.ascontiguousarray(va).tobytes() == np.ascontiguousarray(vb).tobytes()
        if not same:
            bad = np.nonzero((va != vb).reshape(va.shape[0], -1).any(axis=1) if k not in ('e', 'z')
                             else (va != vb).any(axis=0))[0]
            raise AssertionError('%s: column %s differs for %d of %d individuals, first id %d'
                                 % (tag, k, bad.size, ca['ids'].size,
                                    ca['ids'][bad[0]] if bad.size else -1))
    return ca


# ---------------------------------------------------------------- life-history changes
# name -> (what the handle starts with, what the change sets), both on top of mating_radius 3,
# K_factor 1 and the parameters-file defaults, in the oracle's terms (gnx_step.Params)
PARAM_CASES = {
    'b': ({}, dict(b=0.6)),
    'R': ({}, dict(R=1.5)),
    'd_min': ({}, dict(d_min=0.3)),
    'd_max': ({}, dict(d_max=0.6)),
    'births_fixed_3': ({}, dict(n_births_lambda=3)),
    'births_poisson': ({}, dict(n_births_fixed=False, n_births_lambda=1.7)),
    'radius_shrinks': ({}, dict(mating_radius=1.2)),
    'radius_grows': (dict(mating_radius=1.2), dict(mating_radius=3.0)),
    'panmixia': ({}, dict(mating_radius=-1.0)),
    'mate_nearest': ({}, dict(mate_mode='nearest')),
    'mate_inverse': (dict(mate_mode='nearest'), dict(mate_mode='inverse')),
    'repro_age': ({}, dict(repro_age=(2, 2))),
    'max_age': ({}, dict(max_age=3)),
    'movement': ({}, dict(move_distr='wald', move_p1=1.5, move_p2=2.0, dir_mu=1.0,
                          dir_kappa=2.5)),
    'dispersal': ({}, dict(disp_distr='wald', disp_p1=0.5, disp_p2=1.0)),
    'window_width': ({}, dict(window_width=4.0)),
    'K_factor': ({}, dict(K_factor=0.5)),
    'move_off': ({}, dict(move=False)),
    'move_on': (dict(move=False), dict(move=True)),
    'p_male': (dict(sexed=True), dict(p_male=0.8)),
}
WALKED_PARAM_CASES = ['b', 'radius_shrinks', 'window_width']


def device_params(p):
    """gnx_step.Params keywords -> those of _native.default_species_params"""
    nat = native()
    out = {}
    for k, v in p.items():
        if k in ('move_distr', 'disp_distr'):
            v = nat.DIST[v]
        elif k == 'mate_mode':
            v = {'uniform': nat.MATE_UNIFORM, 'nearest': nat.MATE_NEAREST,
                 'inverse': nat.MATE_INVERSE}[v]
        elif k == 'max_age':
            v = -1 if v is None else int(v)
        elif k in ('n_births_fixed', 'sexed', 'move'):
            v = int(bool(v))
        out[k] = v
    return out


def oracle_with_params(st, arch, **params):
    """the oracle's state under other parameters: the lattice and the hash grid are rebuilt, as
    gnx_set_species_params does; population, step index and largest id stay"""
    p = dict(mating_radius=3.0, K_factor=1.0)
    p.update(params)
    new = S.State(st.rasts, S.Params(**p), st.seed, L=L, traits=arch['traits'],
                  paths_packed=st.paths)
    for k in ('x', 'y', 'age', 'sex', 'id', 'fit', 'e', 'z', 'geno'):
        setattr(new, k, getattr(st, k).copy())
    new.step, new.max_id = st.step, st.max_id
    return new
