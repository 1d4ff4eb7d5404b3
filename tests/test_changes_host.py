"""Who sees a changed raster, and when - pinned to the reference, then to the oracle.  No GPU.

The reference samples the habitat values of everybody at the end of every mating
(structs/species.py:804) and after every movement (:582-585), so one step after a layer
change everybody's e is the new raster at its cell, whether it moved or not.
tests/golden/g18_change_e.npz is a reference run of a species that stays put under a
layer-change event; the oracle's step (oracle/gnx_step.py) is replayed on the experiment of
tests/_changes.py, the one tests/test_gpu_changes.py runs on the device."""
import numpy as np
import pytest

import gnx_step as S
import _changes as X
from _columns import check_columns
from conftest import load_golden


def test_reference_e_follows_the_raster_of_the_step():
    """the reference's own statement of the rule: after each of 8 main steps (layer 1 changes
    after steps 2, 4 and 6) e[1] of everybody is the raster in force during that step at the
    individual's cell - for a species with movement.move = False"""
    g = load_golden('g18_change_e')
    n_changed = 0
    born_before = None
    for t in range(8):
        rast, ids, x, y, e = (g['%s_%d' % (k, t)] for k in ('rast', 'ids', 'x', 'y', 'e'))
        assert rast.shape == (20, 20) and e.shape == (ids.size, 2) and ids.size >= 50
        np.testing.assert_array_equal(e[:, 1], rast[y.astype(int), x.astype(int)])
        np.testing.assert_array_equal(e[:, 0], 1.0)
        if t > 0:
            prev = g['rast_%d' % (t - 1)]
            if not np.array_equal(prev, rast):
                n_changed += 1
                # the check is about adults: individuals from before this change, whose cell
                # has another value now, and who did not move
                old = np.isin(ids, g['ids_%d' % (t - 1)])
                moved = prev[y.astype(int), x.astype(int)] != rast[y.astype(int), x.astype(int)]
                assert (old & moved).sum() >= 20, (t, (old & moved).sum())
                px = dict(zip(g['ids_%d' % (t - 1)], g['x_%d' % (t - 1)]))
                assert all(px[i] == xx for i, xx in zip(ids[old], x[old]))
        if t == 2:
            born_before = ids
    assert n_changed == 3
    np.testing.assert_array_equal(g['rast_0'], g['start_rast'])
    np.testing.assert_array_equal(g['rast_7'], g['end_rast'])
    assert np.isin(g['ids_7'], born_before).sum() >= 10


@pytest.mark.parametrize('move', [False, True])
def test_oracle_step_resamples_e_after_a_layer_change(move):
    """the oracle's step: layer 1 replaced before step 4, 8 steps; after every step
    e == rasts[:, cy, cx] for everybody and fit is the fitness of those e (check_columns: e
    exact, fit within ulp32 of _columns.fitness_ref).  At each of the 4 checks after the change
    at least 100 individuals from before it are alive, at least 50 of them with a fitness the
    old raster would have made different."""
    arch = X.make_arch()
    old = X.rasters(2)
    new = X.reversed_layer(old, 1)
    st = X.oracle_state(old, arch, move=move)
    before = None
    alive = []
    for t in range(8):
        if t == 4:
            before = st.id.copy()
            e_kept = st.e.copy()
            st.rasts = new
            # the change itself touches nobody's e
            np.testing.assert_array_equal(st.e, e_kept)
        S.step(st)
        cols = X.oracle_cols(st)
        check_columns(cols, st.rasts, arch, True)
        if t >= 4:
            alive.append(X.assert_sharp(cols, before, old, arch,
                                        'oracle, move %d, step %d' % (move, t)))
    assert len(alive) == 4 and min(alive) >= 100, alive


@pytest.mark.parametrize('name', sorted(X.PARAM_CASES))
def test_oracle_every_parameter_change_does_something(name):
    """the condition of test_gpu_changes.py's parameter cases, on the oracle: within 3 steps
    after the change the population differs, in count or in ids, from the one that kept the
    old parameters"""
    arch = X.make_arch()
    base, change = X.PARAM_CASES[name]
    st = X.oracle_state(X.rasters(2), arch, **base)
    for _ in range(3):
        S.step(st)
    assert st.N >= 150, st.N
    kept = X.oracle_with_params(st, arch, **base)
    changed = X.oracle_with_params(st, arch, **dict(base, **change))
    differs = False
    for _ in range(3):
        S.step(kept)
        S.step(changed)
        assert min(kept.N, changed.N) >= 50, (kept.N, changed.N)
        differs = differs or kept.N != changed.N or not np.array_equal(np.sort(kept.id),
                                                                       np.sort(changed.id))
    assert differs, name
