"""The device's time step beside the step oracle (oracle/gnx_step.py) in every life-history
regime, decision by decision: what tests/test_step_regimes_host.py (oracle alone, no GPU) and
tests/test_gpu_step_regimes.py (on the device) share.

The experiment is that of tests/_changes.py - 24 x 24 cells, 500 founders, L = 128, one trait
of 8 dyadic effect sizes on layer 1, seed 31, six main steps with selection - under 24
parameter sets, given in the oracle's terms (gnx_step.Params; _changes.device_params
translates them).

Both sides draw from the same random streams, so they take the same integer decisions unless
one of them sits on a rounding tie: the device's logf / cosf / f32 expressions differ from
numpy's in the last bits.  `census` counts, on the oracle's own step, the decisions that sit
within a margin of flipping.  A step with none is CLEAN: there births, deaths, ids, parents,
recombination keys, start homologues, ages, sexes, genotypes, z, e, fit and positions must
all agree and nothing is excused.  On the other (SOFT) steps a difference in the decisions
needs a witness - the tie that explains it, `witness` - and then the oracle is re-seated on
the device's population so that the steps after the tie are compared exactly again.

Position bound.  After every compared step the oracle takes over the device's coordinates
(`reseat_positions`), so both sides start each step from bit-identical f32 positions.  The
step adds d * cos(theta) and d * sin(theta) in f32, d and theta coming from a handful of
logf / expf / cosf / sqrtf / acosf calls of a few ulp each on either side; the sum is rounded
at most at the landscape's far edge, where f32 numbers are 2^-19 apart.  Sixteen of those
spacings, POS_TOL = 16 * 2^-19 = 3.05e-5, bound the difference of the two sides; where the drawn
distance itself is larger than the landscape (d > 24) its own spacing takes the place of
2^-19.  The census uses the same margin: a coordinate closer than that to a cell boundary may
fall on either side of it.
"""
import functools

import numpy as np

import gnx_oracle as O
import gnx_step as S
import _changes as X
from _columns import check_columns, ulp32

F = np.float32
N_STEPS = 6
POS_TOL = 16 * 2.0 ** -19           # 3.05e-5, see the module docstring
RADIUS_TOL = 1e-4                   # witness margins of test_device_step_matches_oracle_step_counts
DEATH_TOL = 1e-5
FOUNDERS_SEED = 6                   # _changes.founders

# name -> (gnx_step.Params keywords on top of mating_radius 3, K_factor 1; founders seed)
CASES = {
    'default': ({}, FOUNDERS_SEED),
    'b': (dict(b=0.6), FOUNDERS_SEED),
    'R': (dict(R=1.5), FOUNDERS_SEED),
    'd_min': (dict(d_min=0.3), FOUNDERS_SEED),
    'd_max': (dict(d_max=0.6), FOUNDERS_SEED),
    'births_fixed_3': (dict(n_births_lambda=3), FOUNDERS_SEED),
    'births_poisson': (dict(n_births_fixed=False, n_births_lambda=1.7), FOUNDERS_SEED),
    'radius_small': (dict(mating_radius=1.2), FOUNDERS_SEED),
    'panmixia': (dict(mating_radius=-1.0), FOUNDERS_SEED),
    'mate_nearest': (dict(mate_mode='nearest'), FOUNDERS_SEED),
    'mate_inverse': (dict(mate_mode='inverse'), FOUNDERS_SEED),
    'repro_age': (dict(repro_age=(2, 2)), FOUNDERS_SEED),
    'max_age': (dict(max_age=3), FOUNDERS_SEED),
    'move_wald': (dict(move_distr='wald', move_p1=1.5, move_p2=2.0, dir_mu=1.0, dir_kappa=2.5),
                  FOUNDERS_SEED),
    'move_levy': (dict(move_distr='levy', move_p1=0.0, move_p2=0.2), FOUNDERS_SEED),
    'disp_wald': (dict(disp_distr='wald', disp_p1=0.5, disp_p2=1.0), FOUNDERS_SEED),
    'window_width': (dict(window_width=4.0), FOUNDERS_SEED),
    'K_factor': (dict(K_factor=0.5), FOUNDERS_SEED),
    'move_off': (dict(move=False), FOUNDERS_SEED),
    'sexed': (dict(sexed=True), FOUNDERS_SEED),
    'p_male': (dict(sexed=True, p_male=0.8), FOUNDERS_SEED),
    'sexed_ages': (dict(sexed=True, repro_age=(1, 2), max_age=4, n_births_fixed=False,
                        n_births_lambda=2.5, b=0.5), FOUNDERS_SEED),
    'panmixia_sexed': (dict(sexed=True, mating_radius=-1.0, b=0.5), FOUNDERS_SEED),
    'K_layer_zero': (dict(K_layer=2), FOUNDERS_SEED),
}
NAMES = list(CASES)


def case_params(name):
    p = dict(mating_radius=3.0, K_factor=1.0)
    p.update(CASES[name][0])
    return p


def case_rasters(name):
    """rasters(2); for K_layer_zero three layers, the third 1.5 with columns 8 - 10 at 0"""
    if name != 'K_layer_zero':
        return X.rasters(2)
    K = np.full((X.H, X.W), 1.5, F)
    K[:, 8:11] = 0
    return X.with_layer(X.rasters(3), 2, K)


def case_population(name):
    """the founders of _changes.founders (or of the case's own seed), as make_handle takes them"""
    sexed = bool(CASES[name][0].get('sexed', False))
    seed = CASES[name][1]
    if seed == FOUNDERS_SEED:
        x, y, age, sex, geno = X.founders(sexed=sexed)
    else:
        rng = np.random.RandomState(seed)
        x = rng.rand(X.N0) * X.W
        y = rng.rand(X.N0) * X.H
        age = rng.randint(0, 4, X.N0)
        geno = O.pack_genomes((rng.rand(X.N0, X.L, 2) < 0.5).astype(np.uint8))
        sex = rng.randint(0, 2, X.N0) if sexed else np.zeros(X.N0, np.int64)
    return dict(x=x, y=y, age=age, sex=sex, ids=np.arange(X.N0), geno=geno)


def oracle_for(name):
    q = case_population(name)
    st = S.State(case_rasters(name), S.Params(**case_params(name)), X.SEED, L=X.L,
                 traits=X.make_arch()['traits'], paths_packed=X.paths())
    st.set_population(q['x'], q['y'], q['age'], q['sex'], q['ids'])
    st.set_genomes(q['geno'])
    return st


def handle_for(name, cap=X.CAP):
    return X.make_handle(case_rasters(name), X.make_arch(), cap=cap,
                         population=case_population(name),
                         **X.device_params(case_params(name)))


# ---------------------------------------------------------------- the near-tie census
def _grid(st):
    p = st.p
    r = p.mating_radius if p.mating_radius is not None else -1.0
    return O.hash_grid((st.W, st.H), r, fine=p.mate_mode == 'nearest')


def _near_boundary(v, cell, n_cells, tol, hi):
    """which of the coordinates v lie within tol of an inner boundary k * cell, 1 <= k < n_cells.
    Coordinates clamped to exactly 0 or to `hi` do not count: both sides clamp to the same
    constant."""
    v64 = np.asarray(v, np.float64)
    k = np.rint(v64 / cell)
    near = (k >= 1) & (k <= n_cells - 1) & (np.abs(v64 - k * cell) < tol)
    return near & (np.asarray(v) != F(0)) & (np.asarray(v) != hi)


def census(st):
    """The decisions of the oracle's last step (S.step(st)) that sit within a margin of
    flipping -> dict kind -> count:
      raster   a post-move or newborn coordinate within its tolerance of a raster-cell boundary
      hash     a post-move coordinate within its tolerance of a hash-cell boundary
      radius   a pair of individuals at a distance within RADIUS_TOL of the mating radius
      death    a death draw within DEATH_TOL of its probability
      low_edge a dispersal attempt, up to the one that was accepted, whose clipped coordinate
               is within POS_TOL of 0 (an attempt is rejected when it is clipped to 0 exactly)
    The tolerance of a coordinate is POS_TOL, or 16 spacings of the drawn distance if that
    exceeds the landscape."""
    out = dict(raster=0, hash=0, radius=0, death=0, low_edge=0)
    hi_x, hi_y = F(st.W - 0.001), F(st.H - 0.001)
    inv_cs, ncx, ncy = _grid(st)
    cs = 1.0 / inv_cs
    mv = st.last_move
    if mv is not None:
        tol = pos_tol(mv['dist'])
        for v, n_r, n_h, hi in ((mv['x'], st.W, ncx, hi_x), (mv['y'], st.H, ncy, hi_y)):
            out['raster'] += int(_near_boundary(v, 1.0, n_r, tol, hi).sum())
            out['hash'] += int(_near_boundary(v, cs, n_h, tol, hi).sum())
    lb = st.last_births
    if lb is not None:
        for v, n_r, hi in ((lb['x'], st.W, hi_x), (lb['y'], st.H, hi_y)):
            out['raster'] += int(_near_boundary(v, 1.0, n_r, POS_TOL, hi).sum())
        for a in range(lb['theta'].shape[0]):
            nx, ny = O.move_transform(lb['mid_x'], lb['mid_y'], lb['theta'][a], lb['dist'][a],
                                      (st.W, st.H), dtype=F)
            tried = lb['attempt'] >= a
            low = ((nx > 0) & (nx < POS_TOL)) | ((ny > 0) & (ny < POS_TOL))
            # an attempt clipped to 0 on this side may have stayed inside on the other
            zero = ((nx == 0) | (ny == 0)) & (np.minimum(
                lb['mid_x'].astype(np.float64) + np.cos(lb['theta'][a].astype(np.float64))
                * lb['dist'][a], lb['mid_y'].astype(np.float64)
                + np.sin(lb['theta'][a].astype(np.float64)) * lb['dist'][a]) > -POS_TOL)
            out['low_edge'] += int((tried & (low | zero)).sum())
    r = st.p.mating_radius
    if r is not None and r > 0:
        # everybody who was there when the pairs were made: the newborns came after
        dth = st.last_death
        old = np.ones(dth['ids'].size, bool) if lb is None else ~np.isin(dth['ids'], lb['child'])
        x, y = dth['x'][old].astype(np.float64), dth['y'][old].astype(np.float64)
        d = np.hypot(x[:, None] - x[None, :], y[:, None] - y[None, :])
        out['radius'] = int((np.abs(d - r) < RADIUS_TOL).sum()) // 2
    dth = st.last_death
    out['death'] = int((np.abs(dth['u'] - dth['p']) < DEATH_TOL).sum())
    return out


def pos_tol(dist):
    """the position bound of individuals whose drawn distances are `dist` (module docstring)"""
    dist = np.abs(np.asarray(dist, F))
    big = np.isfinite(dist) & (dist > 24)
    return np.where(big, 16.0 * np.spacing(np.where(big, dist, F(1))).astype(np.float64), POS_TOL)


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """the oracle alone, N_STEPS steps -> one record per step (computed once per case)"""
    st = oracle_for(name)
    K = st.rasts[st.p.K_layer]
    recs = []
    for t in range(N_STEPS):
        n0 = st.N
        n_pairs, B, Dth = S.step(st)
        dth, lb, lp, mv = st.last_death, st.last_births, st.last_pairs, st.last_move
        cx, cy = dth['x'].astype(np.int64), dth['y'].astype(np.int64)
        recs.append(dict(
            N0=n0, pairs=n_pairs, births=B, deaths=Dth, census=census(st),
            n_d_min=int((dth['d'] == st.p.d_min).sum()),
            n_d_max=int((dth['d'] == st.p.d_max).sum()),
            n_older_3=int((dth['age'] > 3).sum()),
            n_on_K0=int((K[cy, cx] == 0).sum()),
            births_per_pair=None if lb is None else lb['n_per_pair'].copy(),
            focal_sex=lp['sex'][:, 0].copy(), mate_sex=lp['sex'][:, 1].copy(),
            n_male=int((dth['sex'] == 1).sum()), n_female=int((dth['sex'] == 0).sum()),
            longest_move=0.0 if mv is None else float(mv['dist'].max())))
    return recs


# ---------------------------------------------------------------- the lockstep comparison
def oracle_cols(st):
    c = X.oracle_cols(st)
    c.update(age=st.age.copy(), sex=st.sex.copy())
    return X.by_id(c)


def decision_differences(dc, oc, counts_dev, counts_or, births_dev, lb):
    """(a) of the comparison -> list of messages, empty if the two sides decided alike"""
    out = []
    if counts_dev != counts_or:
        out.append('births %d / %d, deaths %d / %d (device / oracle)'
                   % (counts_dev[0], counts_or[0], counts_dev[1], counts_or[1]))
    if not np.array_equal(dc['ids'], oc['ids']):
        only_d = np.setdiff1d(dc['ids'], oc['ids'])
        only_o = np.setdiff1d(oc['ids'], dc['ids'])
        out.append('ids: %d only on the device %s, %d only in the oracle %s'
                   % (only_d.size, only_d[:4].tolist(), only_o.size, only_o[:4].tolist()))
    if births_dev is not None:
        child, par, keys, starts = births_dev
        if lb is None:
            ref = (np.zeros(0, np.int64), np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int32),
                   np.zeros((0, 2), np.uint8))
        else:
            ref = (lb['child'], lb['parents'], lb['keys'], lb['start'])
        for what, a, b in zip(('newborn ids', 'parents (focal, mate)', 'recombination keys',
                               'start homologues'), (child, par, keys, starts), ref):
            if a.shape != b.shape:
                out.append('%s: %d on the device, %d in the oracle' % (what, len(a), len(b)))
            elif not np.array_equal(a, b):
                k = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
                out.append('%s differ for %d of %d newborns, first id %d: device %s oracle %s'
                           % (what, k.size, len(a), child[k[0]], a[k[0]].tolist(),
                              b[k[0]].tolist()))
    return out


def state_differences(dc, oc, dist_of):
    """(b) and (c) for two populations with the same ids (both by ascending id) -> list of
    messages, largest position error in units of its bound, and in f32 spacings (2^-19)"""
    out = []
    ids = dc['ids']
    for k in ('age', 'sex', 'geno', 'z'):
        a, b = np.asarray(dc[k]), np.asarray(oc[k])
        if k == 'z':
            a, b = a.T.view(np.uint32), np.ascontiguousarray(b.T, F).view(np.uint32)
        bad = np.nonzero((a.astype(np.int64) != b.astype(np.int64)).reshape(ids.size, -1)
                         .any(axis=1) if k != 'geno' else
                         (a != b).reshape(ids.size, -1).any(axis=1))[0]
        if bad.size:
            out.append('column %s differs for %d of %d individuals, first id %d'
                       % (k, bad.size, ids.size, ids[bad[0]]))
    same_cell = (dc['x'].astype(np.int64) == oc['x'].astype(np.int64)) & \
                (dc['y'].astype(np.int64) == oc['y'].astype(np.int64))
    bad = np.nonzero(same_cell & (dc['e'] != oc['e']).any(axis=0))[0]
    if bad.size:
        out.append('column e differs for %d individuals in the same raster cell, first id %d'
                   % (bad.size, ids[bad[0]]))
    bad = np.nonzero(same_cell & ~(np.abs(dc['fit'].astype(np.float64) - oc['fit'])
                                   <= ulp32(oc['fit'])))[0]
    if bad.size:
        out.append('column fit differs for %d individuals, first id %d: device %.9g oracle %.9g'
                   % (bad.size, ids[bad[0]], dc['fit'][bad[0]], oc['fit'][bad[0]]))
    tol = pos_tol(dist_of(ids))
    err = np.maximum(np.abs(dc['x'].astype(np.float64) - oc['x']),
                     np.abs(dc['y'].astype(np.float64) - oc['y']))
    bad = np.nonzero(err > tol)[0]
    if bad.size:
        k = bad[np.argmax(err[bad] / tol[bad])]
        out.append('position differs by %.3g (bound %.3g) for id %d: device (%r, %r) oracle '
                   '(%r, %r); %d of %d beyond their bound'
                   % (err[k], tol[k], ids[k], dc['x'][k], dc['y'][k], oc['x'][k], oc['y'][k],
                      bad.size, ids.size))
    return out, float(err.max() / 2.0 ** -19) if ids.size else 0.0


def witness(st, dc, oc, post_move):
    """A rounding tie that explains why the device and the oracle decided differently in this
    step, or None - the kinds of test_device_step_matches_oracle_step_counts: an individual
    whose two positions (after the movement where the test could read them, `post_move` =
    ids, x, y of the device; else at the end of the step, for those alive on both sides) fall
    into different hash or raster cells; a pair of individuals within RADIUS_TOL of the mating
    radius; a death draw within DEATH_TOL of its probability.  And one kind more, evaluated
    on the oracle's own draws: a dispersal attempt clipped within POS_TOL of the low edge."""
    inv_cs, ncx, ncy = _grid(st)
    pairs = []
    if post_move is not None and st.last_move is not None:
        mv = st.last_move
        od, oo = np.argsort(post_move[0]), np.argsort(mv['ids'])
        pairs.append(('after the movement', post_move[0][od], post_move[1][od], post_move[2][od],
                      mv['ids'][oo], mv['x'][oo], mv['y'][oo]))
    both = np.intersect1d(dc['ids'], oc['ids'])
    kd, ko = np.isin(dc['ids'], both), np.isin(oc['ids'], both)
    pairs.append(('at the end of the step', dc['ids'][kd], dc['x'][kd], dc['y'][kd],
                  oc['ids'][ko], oc['x'][ko], oc['y'][ko]))
    for when, ia, xa, ya, ib, xb, yb in pairs:
        if not np.array_equal(ia, ib):
            continue
        for name, a, b in (('hash cell', O.cell_of(xa, ya, inv_cs, ncx, ncy)[0],
                            O.cell_of(xb, yb, inv_cs, ncx, ncy)[0]),
                           ('raster cell x', xa.astype(np.int64), xb.astype(np.int64)),
                           ('raster cell y', ya.astype(np.int64), yb.astype(np.int64))):
            k = np.nonzero(a != b)[0]
            if k.size:
                return 'id %d %s: %s, device (%r, %r) oracle (%r, %r)' % (
                    ia[k[0]], when, name, xa[k[0]], ya[k[0]], xb[k[0]], yb[k[0]])
    c = census(st)
    dth = st.last_death
    if c['radius']:
        return '%d pairs of individuals within %g of the mating radius' % (c['radius'], RADIUS_TOL)
    if c['death']:
        k = int(np.argmin(np.abs(dth['u'] - dth['p'])))
        return 'id %d: death draw u = %r against p = %r' % (dth['ids'][k], dth['u'][k],
                                                           dth['p'][k])
    if c['low_edge']:
        return '%d dispersal attempts clipped within %g of the low edge' % (c['low_edge'],
                                                                          POS_TOL)
    return None


def reseat_positions(st, dc):
    """the oracle takes over the device's coordinates (and the habitat values there), id by
    id, so that both sides start the next step from the same f32 positions"""
    k = np.searchsorted(dc['ids'], st.id)
    assert np.array_equal(dc['ids'][k], st.id)
    st.x, st.y = dc['x'][k].copy(), dc['y'][k].copy()
    st.e = np.ascontiguousarray(dc['e'].T[k])


def reseat(st, dev, dc, max_id):
    """the oracle re-seated on the device's population after an excused step: every column in
    ascending id order, the step index and the largest id given out from the device"""
    st.x, st.y = dc['x'].copy(), dc['y'].copy()
    st.age, st.sex = dc['age'].astype(np.int32), dc['sex'].astype(np.uint8)
    st.id = dc['ids'].astype(np.int64)
    st.fit = dc['fit'].copy()
    st.e = np.ascontiguousarray(dc['e'].T)
    st.z = np.ascontiguousarray(dc['z'].T)
    st.geno = dc['geno'].copy()
    st.step = int(dev.step_index)
    st.max_id = int(max_id)


def lockstep(name, path):
    """GPU test 1: one handle and one oracle state, N_STEPS steps, compared after each
    -> dict(excused=[(step, witness)], soft=[steps], max_err=largest position error in f32
    spacings at the far edge)"""
    arch = X.make_arch()
    rasts = case_rasters(name)
    dev = handle_for(name)
    st = oracle_for(name)
    nat = X.native()
    max_id = X.N0 - 1
    excused, soft, max_err = [], [], 0.0
    for t in range(N_STEPS):
        tag = 'regime %s, path %s, step %d' % (name, path, t)
        post_move = None
        births_dev = None
        if path == 'step':
            dev.step(False, True)
        else:
            # the queue: the positions after the movement can be read on the way
            dev.age()
            if dev.sp.move:
                dev.move()
                post_move = (dev.download(nat.F_ID), dev.download(nat.F_X),
                             dev.download(nat.F_Y))
            if path == 'queue':
                dev.pop_dynamics(False, True)
            else:
                dev.pop_dynamics_mate(False)
                child, par, keys, starts, _ = dev.last_births()
                o = np.argsort(child, kind='stable')
                births_dev = (child[o], par[o], keys[o], starts[o])
                dev.pop_dynamics_die(False, True)
            dev.step_index = dev.step_index + 1
        _, B, Dth = S.step(st)
        _, b_dev, d_dev = dev.counts()
        max_id += b_dev
        cen = census(st)
        clean = sum(cen.values()) == 0
        if not clean:
            soft.append(t)
        dc = X.by_id(X.download(dev))
        oc = oracle_cols(st)
        try:
            check_columns(dc, rasts, arch, True)
        except AssertionError as err:
            raise AssertionError('%s: %s' % (tag, err)) from None
        diffs = decision_differences(dc, oc, (b_dev, d_dev), (B, Dth), births_dev,
                                     st.last_births)
        if diffs:
            head = '%s (%s, census %s): ' % (tag, 'clean' if clean else 'soft', cen)
            assert not clean, head + 'the decisions differ on a clean step: ' + '; '.join(diffs)
            w = witness(st, dc, oc, post_move)
            assert w is not None, head + 'the decisions differ and no decision of the step ' \
                'sits on a rounding tie: ' + '; '.join(diffs)
            excused.append((t, w))
            assert len(excused) <= 1, '%s: a second excused step in one run: %s' % (tag, excused)
            reseat(st, dev, dc, max_id)
            continue
        assert st.max_id == max_id, (tag, st.max_id, max_id)
        dist = {}
        if st.last_move is not None:
            dist = dict(zip(st.last_move['ids'].tolist(), st.last_move['dist'].tolist()))
        diffs, err = state_differences(
            dc, oc, lambda ids: np.array([dist.get(int(i), 0.0) for i in ids], F))
        max_err = max(max_err, err)
        assert not diffs, '%s (%s, census %s): %s' % (tag, 'clean' if clean else 'soft', cen,
                                                      '; '.join(diffs))
        reseat_positions(st, dc)
    dev.close()
    return dict(excused=excused, soft=soft, max_err=max_err)
