"""Change events on the device step: what a layer upload, an explicit K and a new species
parameter block do to the steps that follow.  Needs an MI355X.

A change rewrites what the kernels read between two steps.  (a) after a layer upload the e
column keeps what the last mating sampled until the next step, and from that step on e and
fit of everybody follow the new raster - also where the species does not move and nothing on
its chain but the age kernel touches the adults; (b) K follows the layer, or the explicit
raster while one is set; (c, d) a handle that was changed in mid-run goes on exactly like a
fresh one that was given the new rasters or parameters from the start, so nothing derived from
the old ones survives (lattice, hash grid, captured graphs, surfaces); (e) the same through
the Model's change events.  The experiment and its oracle replay: tests/_changes.py,
tests/test_changes_host.py."""
import numpy as np
import pytest

import gnx_oracle as O
import _changes as X
from _columns import check_columns

pytestmark = pytest.mark.gpu

LAYER_PATHS = X.STEP_PATHS + ['walk', 'walk_big']


def _checked(dev, rasts, arch, tag):
    cols = X.download(dev)
    try:
        check_columns(cols, rasts, arch, True)
    except AssertionError as err:
        raise AssertionError('%s: %s' % (tag, err)) from None
    return cols


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ a. layers
def _layer_change(path, move, n_layers=2, layer=1, whole_stack=False):
    nat = X.native()
    arch = X.make_arch()
    old = X.rasters(n_layers)
    new = X.reversed_layer(old, layer)
    read_by_trait = any(t['layer'] == layer for t in arch['traits'])
    walked = path.startswith('walk')
    dev = X.make_handle(old, arch, cap=X.BIG_CAP if path == 'walk_big' else X.CAP, move=move)
    tag = '%s, move %d' % (path, move)

    def four_steps(rasts, before):
        for t in range(1 if walked else 4):
            if walked:
                dev.walk(4, False, True)
            else:
                X.take_step(dev, path)
            cols = _checked(dev, rasts, arch, '%s, %s step %d' % (
                tag, 'after the change,' if before is not None else '', 4 if walked else t + 1))
            if before is None:
                continue
            if read_by_trait:
                X.assert_sharp(cols, before, old, arch, tag)
            else:
                cx, cy = cols['x'].astype(int), cols['y'].astype(int)
                who = X.survivors(cols, before)
                assert who.sum() >= 100, (tag, who.sum())
                assert (who & (old[layer][cy, cx] != new[layer][cy, cx])).sum() >= 50, tag
        return cols

    cols = four_steps(old, None)
    before = cols['ids']
    e0 = dev.download(nat.F_E)
    if whole_stack:
        dev.upload_rasters(new)
    else:
        dev.upload_layer(layer, new[layer])
    # the upload itself touches nobody: e is what the last mating sampled until the next step
    assert _same_bits(e0, dev.download(nat.F_E)), tag
    four_steps(new, before)
    tot, pc = dev.totals(), dev.path_counts()
    if path == 'walk':
        assert (tot['dd_steps'] > 0) == bool(move), (tag, tot)
    if path == 'walk_big':
        assert tot['dd_steps'] == 0 and pc['lazy_mortalities'] == (6 if move else 0), (tag, tot, pc)
    dev.close()


@pytest.mark.parametrize('move', [1, 0])
@pytest.mark.parametrize('path', LAYER_PATHS)
def test_layer_change_reaches_e_and_fit(path, move):
    """4 steps, upload_layer(1, reversed), 4 steps, on every path that takes a step: e of
    everybody is the raster in force during the step at its cell, exactly, and fit the fitness
    of that e within ulp32 - for at least 100 individuals from before the change, 50 of whom the
    old raster would give another fitness.

    Against a library built from the csrc/ of the commit before the fix, every move = 0 case
    fails at its first step after the change with
    'id 2: e of layer 1 is 0.826086938, the raster at its cell (19, 9) has 0.173913047 (258 of
    303 individuals differ)' (after the walk: 145 of 260) - exactly those from before the
    change: k_age was all that touched the adults of a species that stays put."""
    _layer_change(path, move)


def test_whole_stack_upload_reaches_e_and_fit():
    """the same through upload_rasters, all layers at once, for the species that stays put"""
    _layer_change('step', 0, whole_stack=True)


def test_change_of_a_layer_no_trait_reads_reaches_e():
    """three layers, the trait on layer 1, layer 2 changes: e of layer 2 follows all the same"""
    _layer_change('queue', 0, n_layers=3, layer=2)


# ------------------------------------------------------------------ b. K
def test_K_follows_the_layer_or_the_explicit_raster():
    """d at every cell from constant density nodes (the pattern of
    test_demography_algebra_vs_reference) and the K raster itself, after a K-layer upload with
    no explicit K, with an explicit K, after another layer upload while it is set, and after
    it is dropped"""
    from test_gpu_parity import make_dev, upload_simple
    nat = X.native()
    Hk = Wk = 12
    rng = np.random.RandomState(2)
    lay = [(rng.rand(Hk, Wk) * 2).astype(np.float32) for _ in range(3)]
    for l in lay:
        l[0, :3] = 0
    K2 = rng.rand(Hk, Wk) * 3
    R, b, lam, dmin, dmax, kf = 0.5, 0.2, 1, 0.0, 1.0, 2.0
    dev = make_dev(Wk, Hk, rasts=np.stack([np.ones((Hk, Wk), np.float32), lay[0]]), K_layer=1,
                   K_factor=kf, R=R, b=b, n_births_lambda=lam, d_min=dmin, d_max=dmax, cap=512)
    xs, ys = np.meshgrid(np.arange(Wk) + 0.25, np.arange(Hk) + 0.75)
    upload_simple(dev, xs.ravel(), ys.ravel())
    jx, jy = dev.lattice_dims()

    def check(K, tag):
        np.testing.assert_array_equal(dev.download_raster(nat.R_K), K, err_msg=tag)
        for Nval, Pval in [(1.7, 0.2), (3.0, 0.0), (0.0, 0.3)]:
            p, d = dev.op_death_probs(False, np.full((jy, jx), Nval), np.full((jy, jx), Pval))
            _, _, _, d_ref = O.calc_d(np.full((Hk, Wk), Nval), K, np.full((Hk, Wk), Pval), R, b,
                                      lam, dmin, dmax)
            np.testing.assert_allclose(d.reshape(Hk, Wk), d_ref, rtol=1e-12, atol=1e-15,
                                       err_msg=tag)

    check(lay[0].astype(np.float64) * kf, 'the first layer')
    dev.upload_layer(1, lay[1])
    check(lay[1].astype(np.float64) * kf, 'after upload_layer')
    dev.set_K_raster(K2)
    check(K2, 'explicit K')
    dev.upload_layer(1, lay[2])
    check(K2, 'a layer upload while K is explicit')
    dev.set_K_raster(None)
    check(lay[2].astype(np.float64) * kf, 'explicit K dropped')
    dev.close()


# ------------------------------------------------------------------ c, d. twins
def _sp(params):
    p = dict(mating_radius=3.0, K_factor=1.0)
    p.update(X.device_params(params))
    return p


def _twin_run(arch, old_rasts, new_rasts, old_params, new_params, walked, tag):
    """A: 3 steps, the change, 3 steps.  B: a fresh handle with the new rasters and parameters
    from the start and A's population at the change.  C: another, left at the old ones.
    A == B bit for bit after every step (after the walk, if A walks); A != C at some step."""
    nat = X.native()
    A = X.make_handle(old_rasts, arch, **_sp(old_params))
    max_id = X.N0 - 1
    if walked:
        A.walk(3, False, True)
        max_id += X.births_of(A, walked=True)
    else:
        for _ in range(3):
            A.step(False, True)
            max_id += X.births_of(A)
    assert A.N >= 150, (tag, A.N)
    C = X.twin_of(A, max_id, old_rasts, arch, **_sp(old_params))
    if new_rasts is not old_rasts:
        (layer,) = [l for l in range(len(old_rasts))
                    if not np.array_equal(old_rasts[l], new_rasts[l])]
        A.upload_layer(layer, new_rasts[layer])
    if new_params is not old_params:
        A.set_species_params(nat.default_species_params(**_sp(new_params)))
    B = X.twin_of(A, max_id, new_rasts, arch, **_sp(new_params))
    differs = False
    if walked:
        A.walk(3, False, True)
    for t in range(3):
        if not walked:
            A.step(False, True)
        B.step(False, True)
        C.step(False, True)
        if not walked or t == 2:
            a = X.assert_same_population(A, B, '%s, step %d after the change: changed handle != '
                                         'fresh handle' % (tag, t + 1))
            assert a['ids'].size >= 50, (tag, a['ids'].size)
            c = np.sort(X.download(C)['ids'])
            differs = differs or not np.array_equal(a['ids'], c)
    assert differs, '%s: the change did nothing within 3 steps' % tag
    for d in (A, B, C):
        d.close()


SURFACES = {
    'move_mixture': dict(move_surf='mixture', move_surf_layer=2),
    'move_unimodal': dict(move_surf='unimodal', move_surf_layer=2),
    'dispersal': dict(disp_surf='mixture', disp_surf_layer=2),
}


@pytest.mark.parametrize('name', sorted(SURFACES))
def test_surface_layer_change_equals_fresh_handle(name):
    """a movement surface (mixture, unimodal) or a dispersal surface on layer 2, traits on
    layers 1 and 2; layer 2 is replaced after 3 steps.  The oracle tests pin what a surface
    does on a static raster; this one that nothing derived from the old raster survives."""
    nat = X.native()
    kind = {'mixture': nat.SURF_MIXTURE, 'unimodal': nat.SURF_UNIMODAL}
    params = {k: kind.get(v, v) for k, v in SURFACES[name].items()}
    old = X.rasters(3)
    # (conductances stay positive: the reversed gradient, lifted off zero like the old one is not)
    new = X.with_layer(old, 2, 0.1 + 0.9 * old[2][::-1, ::-1])
    _twin_run(X.make_arch(layers=(1, 2)), old, new, params, params, False, name)


PARAM_RUNS = [(n, False) for n in sorted(X.PARAM_CASES)] + [(n, True)
                                                            for n in X.WALKED_PARAM_CASES]


@pytest.mark.parametrize('name,walked', PARAM_RUNS)
def test_parameter_change_equals_fresh_handle(name, walked):
    """set_species_params in mid-run, one changed field per case (tests/_changes.py:
    PARAM_CASES); walked: A takes its steps as walk(3), change, walk(3), so the graphs captured
    under the old parameters must be dropped"""
    base, change = X.PARAM_CASES[name]
    rasts = X.rasters(2)
    _twin_run(X.make_arch(), rasts, rasts, base, dict(base, **change), walked,
              '%s%s' % (name, ', walked' if walked else ''))


# ------------------------------------------------------------------ e. the Model
def _model_arch(spp):
    ga = spp.gen_arch
    traits = [dict(loci=np.asarray(trt.loci), alpha=np.asarray(trt.alpha, np.float64),
                   layer=int(trt.lyr_num), phi=trt.phi, gamma=trt.gamma, univ_adv=trt.univ_adv)
              for _, trt in sorted(ga.traits.items())]
    return dict(traits=traits, dom=ga.dom if ga._use_dom else None,
                delet_loci=np.asarray(ga.delet_loci, np.int64),
                delet_s=np.asarray(ga.delet_loci_s, np.float64))


@pytest.mark.parametrize('move', [False, True])
def test_model_change_events_reach_e_fit_and_b(move):
    """the product path - _make_land_change -> _sync_changed_layers -> _set_K, and the
    life-history changer: a layer-change event (start_t 2, end_t 6, 3 steps) on the layer the
    trait reads and b -> 0.5 at t = 3; walk(1) eight times, after each the columns against
    the stack that was in force during it and the device's b against the Species'.

    Against a library built from the csrc/ of the commit before the fix the move = False case
    fails after the walk that follows the first change (t = 3) with
    'id 9: e of layer 1 is 0.956521749, the raster at its cell (22, 22) has 0.652173936 (81 of
    91 individuals differ)'."""
    import geonomics_amd as gnx
    from geonomics_amd.sim.params import ParametersDict
    from test_gpu_model_api import small_params
    p = small_params(seed=7, L=64, T=8, dim=(24, 24))
    lyr1 = p['landscape']['layers']['lyr_1']
    start = np.asarray(lyr1['init']['defined']['rast'])
    lyr1['change'] = ParametersDict({0: {'change_rast': start[:, ::-1].copy(), 'start_t': 2,
                                         'end_t': 6, 'n_steps': 3}})
    sp = p['comm']['species']['spp_0']
    sp['movement']['move'] = move
    sp['change'] = ParametersDict({'life_hist': {'b': {'timesteps': [3], 'vals': [0.5]}}})
    mod = gnx.make_model(p)
    spp = mod.comm[0]
    assert spp._move == move
    mod.walk(10000, 'burn', verbose=False)
    assert mod.comm.burned
    arch = _model_arch(spp)
    assert [t['layer'] for t in arch['traits']] == [1, 0]
    n_changes, prev_stack, prev_ids = 0, None, None
    for t in range(8):
        stack = np.array(mod.land._stack(), np.float32)
        mod.walk(1, 'main', verbose=False)
        cols = _checked(spp._dev, stack, arch, 'move %d, t %d' % (move, t))
        assert spp._dev.sp.b == spp.b == (0.5 if t >= 3 else 0.2), (t, spp._dev.sp.b, spp.b)
        if prev_stack is not None and not np.array_equal(prev_stack, stack):
            # the first step under a new raster: adults from before it, at cells whose value changed
            n_changes += 1
            cx, cy = cols['x'].astype(int), cols['y'].astype(int)
            old = np.isin(cols['ids'], prev_ids) & (prev_stack[1][cy, cx] != stack[1][cy, cx])
            print('move %d, t %d: N %d, adults at changed cells %d' % (move, t, cols['ids'].size,
                                                                       old.sum()))
            assert old.sum() >= 20, (t, old.sum())
        prev_stack, prev_ids = stack, cols['ids']
    assert n_changes == 3
    spp._dev.close()
