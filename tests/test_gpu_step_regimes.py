"""The device's time step against the step oracle in 24 life-history regimes, on every path
that takes a step.  Needs an MI355X.

What checks the step outside the parameters-file defaults compares the device with itself (a
changed handle with a fresh one, the walk with the function queue), and the per-regime
operator tests do not go through the fused step, the queue halves or the device-driven walk: a
fault shared by the device sides - an age filter off by one in the pair kernels, a swapped
orientation of the sexes, a misplaced max_age or d_min clip, Poisson births from the wrong
stream, the K = 0 branch of the growth term - would pass them all.  Here (1) gnx_step, the
function queue and its split halves each run beside oracle/gnx_step.py for six steps and are
compared after every one of them, decision by decision and column by column
(tests/_step_regimes.py: lockstep), and (2) the walk, device-driven and lazy, must leave bit
for bit what six gnx_step calls leave - which pins both walks to the oracle as well.
tests/test_step_regimes_host.py holds the conditions under which a pass says something."""
import numpy as np
import pytest

import _changes as X
import _step_regimes as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('path', X.STEP_PATHS)
@pytest.mark.parametrize('name', R.NAMES)
def test_step_matches_oracle_in_lockstep(name, path):
    """Six steps, each taken on the device and in the oracle and compared by ascending id:
    births, deaths and ids (on the split path also every newborn's parents in the order
    focal, mate, its recombination keys and start homologues: gnx_last_births can be read
    only between the halves; on the other paths the newborns' genotypes stand for them), age
    and sex exactly, genotypes and z bit for bit, e exactly and fit within ulp32 wherever
    both sides are in the same raster cell, positions within _step_regimes.POS_TOL, and the
    device's columns against the rasters (check_columns).  On a clean step nothing is
    excused; on a soft step a difference in the decisions needs its witness, the oracle is
    re-seated on the device's population and the run goes on; at most one step of a run may
    be excused.

    What it found was in the oracle.  panmixia and panmixia_sexed failed on all three paths in
    their second step, "regime panmixia, path split, step 1 (clean, ...): the decisions differ
    on a clean step: births 63 / 63, deaths 109 / 108 (device / oracle); ... parents (focal,
    mate) differ for 58 of 63 newborns": gnx_step.sort_by_cell sorted by hash cell alone,
    stably, on top of the order the step before had left, where the device - and the rule
    that test_panmixia_pairs and gnx_oracle.pair_order_keys state - orders the slots by (hash
    cell, id).  Only panmixia reads the slot order (the trial's slot picks both partners), and
    the two orders part ways once somebody has changed its cell.  The oracle sorts by (cell,
    id) now; its runs in the 22 other regimes are bit for bit what they were."""
    out = R.lockstep(name, path)
    print('%s, %s: soft steps %s, excused %s, largest position error %.2f f32 spacings '
          '(2^-19), bound %g' % (name, path, out['soft'], out['excused'], out['max_err'],
                                 R.POS_TOL / 2.0 ** -19))


@pytest.mark.parametrize('cap', [X.CAP, X.BIG_CAP], ids=['cap', 'big_cap'])
@pytest.mark.parametrize('name', R.NAMES)
def test_walk_equals_steps(name, cap):
    """walk(3) twice against six gnx_step calls: the same population bit for bit and the same
    (N at the start, births, deaths) step by step.  At CAP the walk is device-driven exactly
    in the regimes the library drives that way; at BIG_CAP it never is, and its steps take
    the lazy mortality exactly where the library has one - the conditions of
    test_layer_change_reaches_e_and_fit, whose species differ only in whether they move."""
    p = R.case_params(name)
    # what the library asks for before it leaves the host-driven step: a species that moves
    # and mates within a radius for the lazy mortality (gnx_l_mortality), and fixed births on
    # top of that for the device-driven step (gnx_dd_eligible) - gnx_walk loops gnx_step for
    # the others
    lazy = bool(p.get('move', True)) and p['mating_radius'] >= 0
    driven = lazy and bool(p.get('n_births_fixed', True))
    A = R.handle_for(name, cap=cap)
    B = R.handle_for(name, cap=cap)
    hist = []
    for _ in range(2):
        A.walk(3, False, True)
        hist.append(np.stack(A.walk_history()))
    hist = np.concatenate(hist, axis=1)
    steps = []
    for _ in range(6):
        n0 = B.N
        B.step(False, True)
        steps.append((n0,) + tuple(B.counts()[1:]))
    tag = 'regime %s, capacity %d' % (name, cap)
    assert hist.T.tolist() == [list(s) for s in steps], (tag, hist.T.tolist(), steps)
    X.assert_same_population(A, B, tag)
    tot, pc = A.totals(), A.path_counts()
    if cap == X.CAP:
        assert (tot['dd_steps'] > 0) == driven, (tag, tot)
    else:
        assert tot['dd_steps'] == 0 and (pc['lazy_mortalities'] > 0) == lazy, (tag, tot, pc)
    A.close()
    B.close()
